"""Multi-rank path on CPU (gloo, world_size 2 and 4): band sharding + one gather reassemble
exactly the single-rank frame.  Strips are rendered by the oracle (the GPU path's checker),
so this covers the sharding/gather logic bench.py runs over RCCL."""
from __future__ import annotations

import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import host_scene, oracle_camera

from raytracinginonesemester_amd import dist as rdist

W, H, SPP, BAND = 64, 45, 4, 8


def _render_rows(y0, y1):
    from oracle import pyoracle as orc

    hs = host_scene("frog.json")
    cam = hs.camera(W, H)
    rgb = orc.render_g(hs.num_triangles, oracle_camera(cam), hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids,
                       hs.materials, hs.lights, spp=SPP, rows=(y0, y1), threads=1)
    return rgb[y0:y1]


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rows = rdist.rows_of(H, BAND, rank, world)
        parts = [_render_rows(y0, y1) for (y0, y1) in rdist.bands_of(H, BAND, rank, world)]
        mine = np.concatenate(parts, axis=0) if parts else np.zeros((0, W, 3), np.float32)
        assert mine.shape[0] == len(rows)
        strip = torch.zeros((rdist.max_strip_rows(H, BAND, world), W, 3), dtype=torch.float32)
        strip[:len(rows)] = torch.from_numpy(mine)
        frame = rdist.gather_frame(strip, H, BAND, world, rank)
        if rank == 0:
            q.put(frame)
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 4])
def test_gloo_band_gather_reassembles_single_rank_frame(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    frame = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    full = _render_rows(0, H)
    assert np.array_equal(frame.view(np.uint32), full.view(np.uint32))


def test_band_assignment_partitions_rows():
    for world in (1, 2, 3, 8):
        seen = sorted(y for r in range(world) for y in rdist.rows_of(1080, 8, r, world))
        assert seen == list(range(1080))
        idx = rdist.strip_index(1080, 8, world)
        assert idx[:, 0].max() == world - 1


def _gpu_p6_worker(rank, world, port, q):
    """One rank of a gloo group sharing cuda:0: render this rank's bands with the HIP kernel in
    strip layout, then the device frame epilogue (quantise, gather bytes, un-permute)."""
    import torch
    import torch.distributed as dist

    import raytracinginonesemester_amd as rt

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hs = host_scene("frog.json")
        cam = hs.camera(W, H)
        ds = rt.DeviceScene.from_host(hs, device=0)
        opts, _jit = ds.make_opts(spp=SPP, max_depth=1, band_rows=BAND, band_index=rank, band_count=world)
        strip = torch.zeros((rdist.max_strip_rows(H, BAND, world), W, 3), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        ds.render_device(cam, opts, strip.data_ptr(), stream=stream)
        p6 = rdist.gather_p6(strip, H, BAND, world, rank, stream=stream)
        flipped = rdist.gather_p6(strip, H, BAND, world, rank, flip_y=True, stream=stream)
        if rank == 0:
            q.put((p6, flipped))
        ds.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_p6_epilogue_on_one_gpu(world):
    import raytracinginonesemester_amd as rt

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_p6_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    p6, flipped = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    full = _render_rows(0, H)
    assert p6 == rt.encode_p6(full)
    assert flipped == rt.encode_p6(full, flip_y=True)


@pytest.mark.gpu
@pytest.mark.parametrize("gather", ["p6", "f32"])
def test_bench_two_ranks_gloo_on_one_gpu(gather):
    """bench.py's N-rank step on the torch.distributed launcher (--comm torch: band shards, async
    gather of the frame's P6 bytes or float strips, un-permute on rank 0, copy to host) rehearsed
    with 2 gloo ranks sharing one GPU: the frame delivered by the timed steps matches the
    reference's c3 image.  (The native RCCL renderer needs one GPU per rank.)"""
    import json
    import subprocess
    import sys

    repo = Path(__file__).resolve().parents[1]
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", str(repo / "bench.py"), "--gpus", "2",
           "--steps", "3", "--warmup", "1", "--comm", "torch", "--backend", "gloo", "--gather-payload", gather,
           "--share-gpu", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(repo))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0
    par = line["parity"]
    if gather == "p6":
        assert par["timed_step_ppm_identical"]
    else:
        assert par["timed_step_rgb_maxabs"] == 0.0
