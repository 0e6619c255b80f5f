// prune_rule.cpp -- the pruning rule of include/pnr_hip.h as plain sequential host C++: the shared argument checks, one pass over
// the forest in topological order (children before parents for the heights, parents before children for everything else) and the
// order-preserving compaction.  The second statement of the rule beside prune.hip, the baseline of scripts/prune_timing.py.  No HIP
// call, no context: the file builds and runs on its own (make -C pnr_amd/csrc prune_check).
#include "prune.h"
#include "args.h"
#include "join.h"

namespace pnr {

int prune_args(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts *opts, pnr_prune_opts &o)
{
    PNR_REQUIRE(n >= 1 && n <= 0x7fffffffLL && xyz && parent, PNR_E_ARG, "%s: n = %lld nodes (1 to 2^31 - 1) need xyz and parent", who, (long long)n);
    o = opts ? *opts : pnr_prune_opts{1.f, 0.f, 0.f, 0.f};
    PNR_TRY(args::positive(who, "zscale", o.zscale));
    PNR_TRY(args::not_negative(who, "min_length", o.min_length));
    PNR_TRY(args::not_negative(who, "radius_factor", o.radius_factor));
    PNR_TRY(args::not_negative(who, "min_tree", o.min_tree));
    PNR_REQUIRE(args::all_finite(xyz, 3 * n), PNR_E_ARG, "%s: a coordinate is not finite", who);
    PNR_REQUIRE(!radius || args::all_finite(radius, n), PNR_E_ARG, "%s: a radius is not finite", who);
    UnionFind uf(n);
    return link_trees(parent, n, uf, who);
}

int prune_rule(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts &o, pnr_prune_info *info, uint8_t *keep,
               uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg)
{
    const PruneRule rule(o);
    const size_t k = (size_t)n;
    // the children of every node in ascending index (CSR), and the nodes parents first
    std::vector<int64_t> off(k + 1, 0);
    for (int64_t i = 0; i < n; i++)
        if (parent[i] >= 0) off[(size_t)parent[i] + 1]++;
    for (size_t i = 0; i < k; i++) off[i + 1] += off[i];
    std::vector<int32_t> child((size_t)off[k]), topo;
    {
        std::vector<int64_t> fill(off.begin(), off.end() - 1);
        for (int64_t i = 0; i < n; i++)
            if (parent[i] >= 0) child[(size_t)fill[(size_t)parent[i]]++] = (int32_t)i;
    }
    topo.reserve(k);
    for (int64_t i = 0; i < n; i++)
        if (parent[i] < 0) topo.push_back((int32_t)i);
    for (size_t at = 0; at < topo.size(); at++)
        for (int64_t e = off[(size_t)topo[at]]; e < off[(size_t)topo[at] + 1]; e++) topo.push_back(child[(size_t)e]);
    PNR_REQUIRE(topo.size() == k, PNR_E_ARG, "%s: %lld nodes hang on no root (a cycle)", who, (long long)(k - topo.size()));
    // 1: the edges
    std::vector<uint32_t> q(k, 0), H(k, 0), P(k, 0);
    for (int64_t i = 0; i < n; i++) {
        if (parent[i] < 0) continue;
        const double e = rule.edge(xyz + 3 * i, xyz + 3 * (int64_t)parent[i]);
        PNR_REQUIRE(e < PRUNE_LIMIT, PNR_E_ARG, PNR_PRUNE_RANGE_TEXT, who);
        q[(size_t)i] = (uint32_t)e;
    }
    // 2, 3: the heights and the continuing children, children first; cont[p] = -1 for a leaf
    std::vector<int32_t> cont(k, -1);
    for (size_t at = k; at-- > 0;) {
        const int32_t c = topo[at], p = parent[c];
        if (p < 0) continue;
        const uint64_t s = (uint64_t)q[(size_t)c] + H[(size_t)c];
        PNR_REQUIRE(s < (1ull << 32), PNR_E_ARG, PNR_PRUNE_RANGE_TEXT, who);
        const int32_t b = cont[(size_t)p];
        if (b < 0 || s > H[(size_t)p] || (s == H[(size_t)p] && c < b)) cont[(size_t)p] = c, H[(size_t)p] = (uint32_t)s;
    }
    // 4, 5, 6: parents first
    std::vector<int32_t> ord(k, 0), sg(k, 0);
    std::vector<uint8_t> gone(k, 0);
    pnr_prune_info r{};
    r.n = n;
    for (size_t at = 0; at < k; at++) {
        const int32_t i = topo[at], p = parent[i];
        const size_t u = (size_t)i;
        const int64_t kids = off[u + 1] - off[u];
        r.n_leaves += kids == 0, r.n_branch += kids >= 2;
        bool head = true;
        if (p < 0) {
            r.n_roots++;
            sg[u] = i;
            gone[u] = rule.cut_tree(H[u]);
            r.n_removed_trees += gone[u];
        } else {
            const uint64_t far = (uint64_t)P[(size_t)p] + q[u];
            PNR_REQUIRE(far < (1ull << 32), PNR_E_ARG, PNR_PRUNE_RANGE_TEXT, who);
            P[u] = (uint32_t)far;
            head = cont[(size_t)p] != i;
            sg[u] = head ? i : sg[(size_t)p];
            ord[u] = ord[(size_t)p] + (head ? 1 : 0);
            gone[u] = gone[(size_t)p] || (head && rule.cut(q[u] + H[u], radius ? radius[p] : 0.f));
        }
        r.n_segments += head, r.n_removed += gone[u], r.n_removed_segments += head && gone[u];
        r.length_in += q[u], r.length_out += gone[u] ? 0 : q[u];
        r.h_max = std::max(r.h_max, H[u]), r.order_max = std::max(r.order_max, ord[u]);
    }
    for (size_t i = 0; i < k; i++) {
        if (keep) keep[i] = !gone[i];
        if (height) height[i] = H[i];
        if (path) path[i] = P[i];
        if (order) order[i] = ord[i];
        if (seg) seg[i] = sg[i];
    }
    if (info) *info = r;
    return PNR_OK;
}

int prune_apply(const int32_t *parent, const uint8_t *keep, int64_t n, int32_t *new_index_out, int32_t *parent_out, int64_t *m)
{
    static const char *who = "pnr_prune_apply";
    PNR_REQUIRE(n >= 1 && n <= 0x7fffffffLL && parent && keep && m, PNR_E_ARG, "%s: n = %lld nodes (1 to 2^31 - 1) need parent, keep and m", who, (long long)n);
    std::vector<int32_t> idx((size_t)n);
    int32_t count = 0;
    for (int64_t i = 0; i < n; i++) {
        PNR_REQUIRE(parent[i] < n, PNR_E_ARG, "%s: parent[%lld] = %d outside [-1, %lld)", who, (long long)i, parent[i], (long long)n);
        PNR_REQUIRE(!keep[i] || parent[i] < 0 || keep[parent[i]], PNR_E_ARG, "%s: node %lld is kept, its parent %d is removed", who, (long long)i, parent[i]);
        idx[(size_t)i] = keep[i] ? count++ : -1;
    }
    for (int64_t i = 0; parent_out && i < n; i++)
        if (keep[i]) parent_out[idx[(size_t)i]] = parent[i] < 0 ? -1 : idx[(size_t)parent[i]];
    if (new_index_out) std::copy(idx.begin(), idx.end(), new_index_out);
    *m = count;
    return PNR_OK;
}

} // namespace pnr
