// rt_scan.hpp — the exclusive scan of per-tile counts behind the stable compactions: the live
// rays of a path step (rt_path_compact_device, rt_path.hpp) and the pixels an adaptive film selects
// (rt_afilm_select_device, rt_frame.hip).  A compaction is three kinds of launch in stream order:
// the unit's own count kernel (one count per PATH_TILE entries), this scan of the counts, and the
// unit's own scatter.  No block waits for another.
// Included inside a device unit's anonymous namespace, after BLOCK (256) is defined.
#pragma once

constexpr int PATH_ROUNDS = 8;
constexpr uint32_t PATH_TILE = BLOCK * PATH_ROUNDS;  // 2048
constexpr int PATH_WAVES = BLOCK / 64;

// The sum of each tile of a[0..n) (the scan's way up).
__global__ __launch_bounds__(BLOCK) void path_tile_sums_kernel(const uint32_t* __restrict__ a, uint32_t n,
                                                               uint32_t* __restrict__ sums) {
    __shared__ uint32_t part[BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * PATH_TILE;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        const uint64_t i = base + (uint32_t)j * BLOCK + threadIdx.x;
        if (i < n) s += a[i];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = BLOCK / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// a[0..n) to its exclusive prefix sums in place, tile by tile: tile b starts at tile_off[b] (null:
// one tile, from 0); total (with one tile; may be null) receives the sum of all.  A thread scans
// PATH_ROUNDS consecutive entries, the block the threads' sums (Hillis-Steele in LDS).
__global__ __launch_bounds__(BLOCK) void path_scan_kernel(uint32_t* __restrict__ a, uint32_t n,
                                                          const uint32_t* __restrict__ tile_off,
                                                          uint32_t* __restrict__ total) {
    __shared__ uint32_t part[2][BLOCK];
    const uint64_t first = (uint64_t)blockIdx.x * PATH_TILE + (uint64_t)threadIdx.x * PATH_ROUNDS;
    uint32_t v[PATH_ROUNDS];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        v[j] = first + (uint32_t)j < n ? a[first + (uint32_t)j] : 0u;
        s += v[j];
    }
    int cur = 0;
    part[0][threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {
        const uint32_t x = part[cur][threadIdx.x] + ((int)threadIdx.x >= d ? part[cur][threadIdx.x - d] : 0u);
        part[cur ^ 1][threadIdx.x] = x;
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = (tile_off != nullptr ? tile_off[blockIdx.x] : 0u) + part[cur][threadIdx.x] - s;
#pragma unroll
    for (int j = 0; j < PATH_ROUNDS; ++j) {
        if (first + (uint32_t)j < n) a[first + (uint32_t)j] = run;
        run += v[j];
    }
    if (total != nullptr && threadIdx.x == BLOCK - 1) *total = part[cur][BLOCK - 1];
}

// Tiles of n entries, and the scratch words of a scan over n entries that recurses through them.
size_t path_tiles(size_t n) { return (n + PATH_TILE - 1) / PATH_TILE; }
size_t path_scan_words(size_t n) {
    size_t words = 0;
    while (n > PATH_TILE) {
        n = path_tiles(n);
        words += n;
    }
    return words;
}

// a[0..n) to exclusive prefix sums in place, the sum to *total: one launch for one tile, else the
// tiles' sums (the next words of scratch), their scan, and the tiles' scans from those offsets.
void path_scan(uint32_t* a, size_t n, uint32_t* scratch, uint32_t* total, hipStream_t st) {
    if (n <= PATH_TILE) {
        hipLaunchKernelGGL(path_scan_kernel, dim3(1), dim3(BLOCK), 0, st, a, uint32_t(n), nullptr, total);
        return;
    }
    const size_t nt = path_tiles(n);
    hipLaunchKernelGGL(path_tile_sums_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, a, uint32_t(n), scratch);
    path_scan(scratch, nt, scratch + nt, total, st);
    hipLaunchKernelGGL(path_scan_kernel, dim3(unsigned(nt)), dim3(BLOCK), 0, st, a, uint32_t(n), scratch, nullptr);
}
