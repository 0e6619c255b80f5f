// join.h -- the traced forest joined into one tree (join.hip), behind pnr_nearest_other / pnr_join_trees / pnr_join_reroot.
#pragma once
#include "call.h"
#include <numeric>
#include <utility>
#include <vector>

namespace pnr {
// The nearest-other search of one call (JoinRule under the pair minimum of pairmin.h): the device buffers (one CallBuf, freed with the
// object) and the packed points.  begin() once, then run() per set of labels: every point i with label[i] >= 0 gets the minimum of d2
// over the points j with label[j] >= 0 and label[j] != label[i], and the smallest j at that minimum (j = -1 and +inf without one, and
// for a negative label).  xyz is taken as it is (the caller has applied zscale).  root: d_out = sqrtf(d2), else d2 itself.  Runs on
// c's stream and returns synchronised.
class JoinSearch {
    pnr_ctx *c_ = nullptr;
    int64_t n_ = 0;
    CallBuf buf_;
    Part<float4> tgt_;
    Part<unsigned long long> key_;
    Part<float> xyz_, d_;
    Part<int> lab_, j_;

public:
    int begin(pnr_ctx *c, const float *xyz, int64_t n, const char *who);
    int run(const int32_t *label, bool root, float *d_out, int32_t *j_out, const char *who);
};

// disjoint sets over 0 .. n - 1 (the host side of the Boruvka rounds of join.hip and geojoin.hip)
struct UnionFind {
    std::vector<int32_t> up;
    explicit UnionFind(int64_t n) : up((size_t)n) { std::iota(up.begin(), up.end(), 0); }
    int32_t find(int32_t a)
    {
        while (up[(size_t)a] != a) a = up[(size_t)a] = up[(size_t)up[(size_t)a]];
        return a;
    }
    bool unite(int32_t a, int32_t b) // the smaller index stays the representative
    {
        a = find(a), b = find(b);
        if (a == b) return false;
        if (a > b) std::swap(a, b);
        up[(size_t)b] = a;
        return true;
    }
};

// the parent links as a union-find; a link inside one set closes a cycle (every node has at most one link of its own)
inline int link_trees(const int32_t *parent, int64_t n, UnionFind &uf, const char *who)
{
    for (int64_t i = 0; i < n; i++) {
        PNR_REQUIRE(parent[i] < n, PNR_E_ARG, "%s: parent[%lld] = %d outside [-1, %lld)", who, (long long)i, parent[i], (long long)n);
        if (parent[i] < 0) continue;
        PNR_REQUIRE(uf.unite((int32_t)i, parent[i]), PNR_E_ARG, "%s: the parent chain of node %lld does not end (a cycle)", who, (long long)i);
    }
    return PNR_OK;
}

// parent[i] in [-1, n) (any negative value = none) without a cycle, or PNR_E_ARG; comp_out[i] (nullable) = the smallest node index of
// i's input tree -- a label >= 0 per tree
int join_input_trees(const int32_t *parent, int64_t n, int32_t *comp_out, const char *who);
// the re-rooting and ordering half of the rule (include/pnr_hip.h); pure host.  n_trees_out is nullable.
int join_reroot(const int32_t *parent, int64_t n, const pnr_bridge *bridges, int64_t nb, int64_t root, int32_t *parent_out, int32_t *order_out,
                int32_t *comp_out, int64_t *n_trees_out);
// Boruvka rounds on c's GPU: the bridges in ascending key order; rounds = the nearest-other passes it took
int join_bridges(pnr_ctx *c, const float *xyz_scaled, const int32_t *parent, int64_t n, float gap, std::vector<pnr_bridge> &bridges, int64_t *n_trees_in,
                 int64_t *rounds);
} // namespace pnr
