// rt_records.hpp — host builders of the traversal records rt::pack_scene packs
// (rt_records.cpp): the camera rays' frustum records (2^D-ary expansions of the reference's
// binary tree), their quantised form, the per-node leaf counts the
// greedy record rules weigh and the greedy rule itself; and the constants the packed layout
// shares with the kernels that read it (rt_device.hip).  Host C++ only.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_mi355x.h"

namespace rt {

// Compact node ids (cid) and child refs: LEAF_BIT | leaf slot, internal index, or NO_REF.
constexpr uint32_t LEAF_BIT = 0x80000000u;
constexpr uint32_t NO_REF = 0xFFFFFFFFu;
constexpr int STACK_CAP = 64;     // one entry per lane of the wave stack
constexpr int LANE_LDS_CAP = 32;  // traverse_lane_lds: per-lane stack entries in LDS (frog needs 18)
// traverse_frustum's stack: two VGPRs, entry k in lane k of the first, 64 + k of the second
constexpr int FRUSTUM_STACK = 128;
constexpr size_t kBigSceneBytes = size_t(64) << 20;  // scene data beyond this leaves the L2s (rt_device.hip)

struct FrustumRecords {
    int log2 = 2;
    int bound = 0;  // the DFS stack bound of the records (root record)
    size_t nrec = 0;
    std::vector<float> rec;
};

// Valid leaves under each node (post-order from the root; cid NO_REF: none).
std::vector<uint32_t> subtree_leaves(const rt_bvh_node* nodes, size_t NN, const uint32_t* cid);
// The greedy record rules' weight of a box: its half surface area (negative extents count 0),
// times by rule 2 sqrt(leaves), 3 log2(leaves + 1), 4 leaves; 1e300 when that is not finite.
double box_weight(const rt_aabb& b, int rule, uint32_t leaves);
// The largest-arity frustum records (2^3..2^dmax) whose DFS fits `cap` stack entries.
// rec_nodes (optional): the binary node each record expands, by record index (the refit plan).
FrustumRecords build_frustum_records(const rt_bvh_node* nodes, size_t NN, const uint32_t* cid,
                                     const rt_aabb* aabbs, int dmax, int cap,
                                     std::vector<uint32_t>* rec_nodes = nullptr);
// The records quantised (16-bit grid steps per entry); false when they cannot be.
bool build_quant_records(const FrustumRecords& fr, std::vector<uint32_t>& qent, std::vector<float>& qhdr);

// The rule the 4-ary records, the frustum records and the tile-culling cuts share: while the
// set e[0..n) has fewer than cap entries, replace its internal entry of largest weight (the first
// among equals; none when no weight exceeds -1) by that node's children that have ids — at the
// entry's own position when in_place (the set stays in SearchBVH's push order), else at the end.
// e has room for cap entries, all of them nodes with ids; the new n is returned.
template <class Weight>
int expand_largest(const rt_bvh_node* nodes, const uint32_t* cid, uint32_t* e, int n, int cap, bool in_place,
                   Weight&& weight) {
    while (n < cap) {
        int best = -1;
        double ba = -1.0;
        for (int i = 0; i < n; ++i) {
            if (cid[e[i]] & LEAF_BIT) continue;
            const double a = weight(e[i]);
            if (a > ba) {
                ba = a;
                best = i;
            }
        }
        if (best < 0) break;
        uint32_t kids[2];
        int nk = 0;
        for (const uint32_t c : {nodes[e[best]].left_idx, nodes[e[best]].right_idx})
            if (c != NO_REF && cid[c] != NO_REF) kids[nk++] = c;
        const int at = in_place ? best : n - 1;
        std::copy(e + best + 1, e + n, e + best);  // (n - 1 entries; at most two come back)
        std::copy_backward(e + at, e + n - 1, e + n - 1 + nk);
        std::copy(kids, kids + nk, e + at);
        n += nk - 1;
    }
    return n;
}

}  // namespace rt
