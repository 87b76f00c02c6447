// rt_scene_pack.hpp — the host half of rt_scene_create (rt_scene_pack.cpp): the caller's BVH
// checked and packed into the arrays the kernels read (the layout at the head of
// rt_device.hip), with the facts the launches choose kernels by.  No device call:
// rt_scene_create uploads the result, rt_debug_scene_pack digests it.  Host C++ only.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_records.hpp"

namespace rt {

// The plain facts a scene carries beside its device arrays (rt_scene derives from this; a clone
// copies it whole).
struct SceneMeta {
    size_t P = 0;
    int nmat = 0, nlights = 0;
    uint32_t root_ref = 0;
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    float bmax[3] = {0, 0, 0};  // per axis max |coordinate| over every AABB (inf: some box is unsorted or not finite)
    int ncut = 0;               // boxes of the tile-culling cut (6 floats each in `cut`)
    int cut_sub_log2 = 0;       // 2^cut_sub_log2 boxes below each cut box in `cut2` (0: no second level)
    bool wide = false;          // 4-ary records (wnode)
    bool lane_stack = false;    // binary DFS stack <= LANE_LDS_CAP (traverse_lane_lds)
    bool lane_wide = false;     // 4-ary records whose DFS stack <= LANE_LDS_CAP (traverse_lane_lds_wide)
    bool deep = false;          // the DFS may need more than STACK_CAP entries: MODE_DEEP kernels
    int f_log2 = 2;             // arity of the frustum records in fnode (2: none, the traversal takes wnode)
    int f_bound = 0;            // their DFS stack bound (<= FRUSTUM_STACK unless RT_TUNE_FRUSTUM_STACK_CAP raised it)

    // The traversal (RT_RAYS_VARIANT_*) every caller query on this scene launches under `flags`.
    // The first that applies: DEEP for a deep scene; WIDE, else BINARY, where the per-lane stack
    // of those records fits LDS; else DEEP, which is exact for any tree (a tree that is not deep
    // needs at most STACK_CAP of its 512 entries, so the brute-force completion, and with it the
    // absent tri array, is unreachable).
    int query_variant(int flags) const {
        int variant = RT_RAYS_VARIANT_DEEP;
        if (!deep) {
            if (wide && lane_wide && !(flags & RT_FLAG_BINARY)) variant = RT_RAYS_VARIANT_WIDE;
            else if (lane_stack) variant = RT_RAYS_VARIANT_BINARY;
        }
        return variant;
    }
};

struct PackedArray {
    const char* name;
    const void* data;
    size_t bytes;
};

struct PackedScene {
    SceneMeta meta;  // (nmat and nlights are the caller's to fill)
    int binary_stack = 0, wide_stack = 0;  // DFS stack bounds of the binary and the 4-ary records
    // refs and triangle indices sit in the float arrays as their bit patterns
    std::vector<float> inode, wnode, fnode, qhdr, ibox, leaf, tnorm, cut, cut2, tri;
    std::vector<uint32_t> qent;
    static constexpr size_t kArrays = 11;
    // every array as bytes, in the order of rt_scene's buffer table (rt_device.hip)
    std::array<PackedArray, kArrays> arrays() const {
        auto a = [](const char* name, const auto& v) { return PackedArray{name, v.data(), v.size() * sizeof(v[0])}; };
        return {a("inode", inode), a("wnode", wnode), a("fnode", fnode), a("qent", qent), a("qhdr", qhdr), a("ibox", ibox),
                a("leaf", leaf),   a("tnorm", tnorm), a("cut", cut),     a("cut2", cut2), a("tri", tri)};
    }
};

// Compact node ids: internal nodes and leaves naming a valid triangle numbered in array order.
struct NodeIds {
    std::vector<uint32_t> cid;  // internal index, LEAF_BIT | leaf slot, or NO_REF
    size_t n_int = 0, n_leaf = 0;
};

// What a refit of the packed arrays needs beside them.  Every stored box is the
// box of one tree node; the arrays already hold the topology in compact refs (child refs in
// inode words 12-13, the triangle index in leaf word 3, entry refs in wnode and fnode), and a
// node's current box is its ibox entry or its leaf record's words 10-15.  The plan adds the
// bottom-up schedule and the ref behind each box slot that has none in the arrays.
struct RefitPlan {
    size_t n_int = 0, n_leaf = 0;
    // internal nodes (compact ids) by ascending height, ties by id: level h (leaves are 0) is
    // order[level_off[h - 1], level_off[h]); a node's children sit in lower levels, and the
    // levels shrink towards the root
    std::vector<uint32_t> order, level_off;
    std::vector<uint32_t> frec_node;          // fnode record -> the internal node it expands
    std::vector<uint32_t> cut_ref, cut2_ref;  // the node (compact ref) of every cut / cut2 slot
};

// RT_ERR_ARG for an empty scene, RT_ERR_UNSUPPORTED past 2^30 triangles.
int check_scene_arrays(size_t P, const void* nodes, const void* aabbs, const void* tris);
// The ids, after checking every internal node's children against the array (RT_ERR_ARG).
int classify_nodes(size_t P, const rt_bvh_node* nodes, NodeIds& ids);
// Everything rt_scene_create derives from the caller's arrays; RT_OK or the error it reports.
// plan (optional): also what a refit needs; RT_ERR_UNSUPPORTED then unless the tree is proper
// (check_proper_tree) and the records are not quantised.
int pack_scene(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris, PackedScene& out,
               RefitPlan* plan = nullptr);

// A tree a refit can keep: every one of the 2P-1 nodes reached from node 0, once; every internal
// node with two children; every leaf naming a triangle.  RT_ERR_UNSUPPORTED otherwise (RT_ERR_ARG
// for a child past the array or a cycle).  height (optional): per node, leaves 0.
int check_proper_tree(size_t P, const rt_bvh_node* nodes, std::vector<uint32_t>* height);

// The host restatement of rt_scene_refit_device: new leaf boxes (aabb_of_triangle) and v0 | e1 | e2,
// tnorm (and tri), internal boxes merged bottom-up, then every stored box rewritten from its node,
// root_box and bmax.  RT_ERR_ARG, touching nothing, when a vertex coordinate is not finite.
int refit_packed(PackedScene& pk, const RefitPlan& plan, const rt_triangle* tris);

// The host half of rt_scene_rebuild's host path: RT_ERR_ARG when a vertex coordinate is not finite,
// else pack_scene with a plan of (the tree built over tris, tris).
int rebuild_pack(size_t P, const rt_bvh_node* nodes, const rt_aabb* aabbs, const rt_triangle* tris, PackedScene& out,
                 RefitPlan& plan);

// rt_debug_scene_pack's words: the facts as info[21], and the FNV-1a hash of an array's bytes.
void scene_info_words(const SceneMeta& m, int binary_stack, int wide_stack, int64_t info[21]);
uint64_t fnv1a(const void* data, size_t bytes);

}  // namespace rt
