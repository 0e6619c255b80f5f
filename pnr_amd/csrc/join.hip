// join.hip -- the nearest point of ANOTHER tree behind pnr_nearest_other / pnr_join_trees, under the pair minimum of pairmin.h, and the host
// half of the join.  The rule (include/pnr_hip.h): per pair dx = x_i - x_j (likewise y, z), d2 = (dx*dx + dy*dy) + dz*dz -- bit-symmetric
// in (i, j), negation is exact --; per point the minimum of d2 over the points of a different, non-negative label and the smallest j at
// that minimum.  Every operation is one IEEE f32 operation (the build has -ffp-contract=off).
//
// join_prep packs a point as one float4 (x, y, z, the bits of its label), so a target is ONE scalar 16-byte load per wave and the vector
// unit only does the dozen operations of the pair.  A point of negative label takes no part, and one without a partner reports -1.
// Below the search: the host side -- input trees, Boruvka's rounds over the passes, re-rooting and ordering.
#include "join.h"
#include "pairmin.h"
#include <cmath>
#include <cstring>
#include <numeric>

namespace {

constexpr int JTPB = pnr::PAIR_TPB;

__global__ __launch_bounds__(JTPB) void join_prep(const float *__restrict__ xyz, const int *__restrict__ label, int n, float4 *__restrict__ tgt)
{
    const int i = blockIdx.x * JTPB + threadIdx.x;
    if (i >= n) return;
    tgt[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float(label[i]));
}

struct JoinRule {
    const float4 *__restrict__ tgt; // (join_prep)
    using Point = float4;
    __device__ Point point(int i) const { return tgt[i]; }
    __device__ bool live(const Point &p) const { return __float_as_int(p.w) >= 0; }
    __device__ int first(int) const { return -1; }
    __device__ bool pair(const Point &p, int j, float &d2) const
    {
        const float4 T = tgt[j];
        const int lj = __float_as_int(T.w);
        const float dx = p.x - T.x, dy = p.y - T.y, dz = p.z - T.z;
        d2 = (dx * dx + dy * dy) + dz * dz;
        return lj >= 0 && lj != __float_as_int(p.w);
    }
};

} // namespace

namespace pnr {

int JoinSearch::begin(pnr_ctx *c, const float *xyz, int64_t n, const char *who)
{
    c_ = c;
    n_ = n;
    // device buffers of the call: the packed points | the packed minima | xyz | the labels | d | j
    const size_t k = (size_t)n;
    tgt_ = buf_.add<float4>(k), key_ = buf_.add<unsigned long long>(k), xyz_ = buf_.add<float>(3 * k);
    lab_ = buf_.add<int>(k), d_ = buf_.add<float>(k), j_ = buf_.add<int>(k);
    const int rc = buf_.alloc(who);
    if (rc) return rc;
    Call call(c, who);
    call.up(xyz_, xyz);
    return call.ok() ? PNR_OK : call.finish(); // (not synchronised: run() follows on the same stream)
}

int JoinSearch::run(const int32_t *label, bool root, float *d_out, int32_t *j_out, const char *who)
{
    pnr_ctx *const c = c_;
    const long long n = n_;
    Call call(c, who);
    call.up(lab_, label);
    call.fill(key_, 0xff);
    int launches = 0;
    c->tic();
    call.launch(join_prep, dim3((unsigned)((n + JTPB - 1) / JTPB)), dim3(JTPB), xyz_, lab_, (int)n, tgt_);
    if (call.ok()) call.note(pair_sweep(call.stream(), JoinRule{tgt_}, n, n, c->opt.join_split, c->opt.join_pairs_per_launch, key_, &launches));
    call.launch(pair_finish, dim3((unsigned)((n + JTPB - 1) / JTPB)), dim3(JTPB), key_, (int)n, root ? 1 : 0, d_, j_);
    c->toc("join", 2 + launches);
    call.down(d_out, d_);
    call.down(j_out, j_);
    return call.finish();
}

// ---- the host side ----
namespace {
struct Key { // (bits(d2), lo, hi), compared lexicographically
    uint32_t bits;
    int32_t lo, hi;
    bool operator<(const Key &o) const { return bits != o.bits ? bits < o.bits : lo != o.lo ? lo < o.lo : hi < o.hi; }
    bool operator==(const Key &o) const { return bits == o.bits && lo == o.lo && hi == o.hi; }
};
} // namespace

int join_input_trees(const int32_t *parent, int64_t n, int32_t *comp_out, const char *who)
{
    UnionFind uf(n);
    const int rc = link_trees(parent, n, uf, who);
    if (rc) return rc;
    if (comp_out)
        for (int64_t i = 0; i < n; i++) comp_out[i] = uf.find((int32_t)i);
    return PNR_OK;
}

int join_bridges(pnr_ctx *c, const float *xyz, const int32_t *parent, int64_t n, float gap, std::vector<pnr_bridge> &bridges, int64_t *n_trees_in, int64_t *rounds)
{
    static const char *who = "pnr_join_trees";
    UnionFind uf(n);
    int rc = link_trees(parent, n, uf, who);
    if (rc) return rc;
    int64_t live = 0;
    for (int64_t i = 0; i < n; i++) live += parent[i] < 0;
    *n_trees_in = live;
    *rounds = 0;
    bridges.clear();
    if (live < 2) return PNR_OK;
    const float g2 = gap * gap;
    JoinSearch search;
    if ((rc = search.begin(c, xyz, n, who))) return rc;
    std::vector<int32_t> label((size_t)n), jj((size_t)n);
    std::vector<float> d2((size_t)n);
    std::vector<char> dead((size_t)n, 0); // per representative: its best edge exceeds the gap -- it can never be joined
    std::vector<Key> best((size_t)n), edges, all;
    while (live >= 2) {
        for (int64_t i = 0; i < n; i++) {
            const int32_t r = uf.find((int32_t)i);
            label[(size_t)i] = dead[(size_t)r] ? -1 : r;
        }
        if ((rc = search.run(label.data(), false, d2.data(), jj.data(), who))) return rc;
        ++*rounds;
        // per component the smallest key: for a fixed i the smallest j is the smallest key, so the per-node result suffices
        for (int64_t i = 0; i < n; i++)
            if (label[(size_t)i] == (int32_t)i) best[(size_t)i].lo = -1;
        for (int64_t i = 0; i < n; i++) {
            const int32_t j = jj[(size_t)i], r = label[(size_t)i];
            if (j < 0 || r < 0) continue;
            uint32_t bits;
            std::memcpy(&bits, &d2[(size_t)i], 4);
            const Key k{bits, std::min((int32_t)i, j), std::max((int32_t)i, j)};
            Key &b = best[(size_t)r];
            if (b.lo < 0 || k < b) b = k;
        }
        edges.clear();
        for (int64_t r = 0; r < n; r++) {
            if (label[(size_t)r] != (int32_t)r || best[(size_t)r].lo < 0) continue;
            float v;
            std::memcpy(&v, &best[(size_t)r].bits, 4);
            if (gap > 0.f && !(v <= g2)) dead[(size_t)r] = 1, live--;
            else edges.push_back(best[(size_t)r]);
        }
        if (edges.empty()) break;
        std::sort(edges.begin(), edges.end());
        edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
        for (const Key &k : edges)
            if (uf.unite(k.lo, k.hi)) all.push_back(k), live--;
    }
    std::sort(all.begin(), all.end());
    for (const Key &k : all) {
        float v;
        std::memcpy(&v, &k.bits, 4);
        bridges.push_back(pnr_bridge{k.lo, k.hi, std::sqrt(v)});
    }
    return PNR_OK;
}

int join_reroot(const int32_t *parent, int64_t n, const pnr_bridge *bridges, int64_t nb, int64_t root, int32_t *parent_out, int32_t *order_out, int32_t *comp_out,
                int64_t *n_trees_out)
{
    static const char *who = "pnr_join_reroot";
    UnionFind uf(n);
    const int rc = link_trees(parent, n, uf, who);
    if (rc) return rc;
    PNR_REQUIRE(root < n, PNR_E_ARG, "%s: root = %lld outside [-1, %lld)", who, (long long)root, (long long)n);
    // the input trees: node count and root per representative
    std::vector<int32_t> in_rep((size_t)n), in_size((size_t)n, 0);
    for (int64_t i = 0; i < n; i++) in_size[(size_t)(in_rep[(size_t)i] = uf.find((int32_t)i))]++;
    for (int64_t k = 0; k < nb; k++) {
        const pnr_bridge &b = bridges[k];
        PNR_REQUIRE(b.lo >= 0 && b.lo < n && b.hi >= 0 && b.hi < n, PNR_E_ARG, "%s: bridge %lld = (%d, %d) outside [0, %lld)", who, (long long)k, b.lo, b.hi, (long long)n);
        PNR_REQUIRE(uf.unite(b.lo, b.hi), PNR_E_ARG, "%s: bridge %lld = (%d, %d) joins two nodes of one tree", who, (long long)k, b.lo, b.hi);
    }
    // neighbours of every node in ascending order (CSR)
    std::vector<int64_t> off((size_t)n + 1, 0);
    auto each_edge = [&](auto &&f) {
        for (int64_t i = 0; i < n; i++)
            if (parent[i] >= 0) f((int32_t)i, parent[i]);
        for (int64_t k = 0; k < nb; k++) f(bridges[k].lo, bridges[k].hi);
    };
    each_edge([&](int32_t a, int32_t b) { off[(size_t)a + 1]++, off[(size_t)b + 1]++; });
    for (int64_t i = 0; i < n; i++) off[(size_t)i + 1] += off[(size_t)i];
    std::vector<int32_t> nbr((size_t)off[(size_t)n]);
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    each_edge([&](int32_t a, int32_t b) { nbr[(size_t)fill[(size_t)a]++] = b, nbr[(size_t)fill[(size_t)b]++] = a; });
    for (int64_t i = 0; i < n; i++) std::sort(nbr.begin() + off[(size_t)i], nbr.begin() + off[(size_t)i + 1]);
    // per output component: its size and its root -- `root` where given, else the input root of its largest input tree (ties: the smallest root)
    std::vector<int32_t> size((size_t)n, 0), top((size_t)n, -1);
    for (int64_t i = 0; i < n; i++) size[(size_t)uf.find((int32_t)i)]++;
    for (int64_t i = 0; i < n; i++) { // input roots in ascending order: only a strictly larger tree replaces an earlier one
        if (parent[i] >= 0) continue;
        int32_t &t = top[(size_t)uf.find((int32_t)i)];
        if (t < 0 || in_size[(size_t)in_rep[(size_t)i]] > in_size[(size_t)in_rep[(size_t)t]]) t = (int32_t)i;
    }
    const int32_t root_comp = root >= 0 ? uf.find((int32_t)root) : -1;
    if (root >= 0) top[(size_t)root_comp] = (int32_t)root;
    std::vector<int32_t> comps;
    for (int64_t i = 0; i < n; i++)
        if (uf.find((int32_t)i) == (int32_t)i) comps.push_back((int32_t)i);
    std::sort(comps.begin(), comps.end(), [&](int32_t a, int32_t b) {
        if ((a == root_comp) != (b == root_comp)) return a == root_comp;
        if (size[(size_t)a] != size[(size_t)b]) return size[(size_t)a] > size[(size_t)b];
        return top[(size_t)a] < top[(size_t)b];
    });
    if (n_trees_out) *n_trees_out = (int64_t)comps.size();
    // depth-first pre-order from every root, children in ascending index
    std::vector<int32_t> par((size_t)n, -1), stack;
    int64_t pos = 0;
    for (size_t ci = 0; ci < comps.size(); ci++) {
        stack.assign(1, top[(size_t)comps[ci]]);
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            if (order_out) order_out[pos] = v;
            if (comp_out) comp_out[v] = (int32_t)ci;
            pos++;
            for (int64_t k = off[(size_t)v + 1]; k-- > off[(size_t)v];) {
                const int32_t u = nbr[(size_t)k];
                if (u == par[(size_t)v]) continue;
                par[(size_t)u] = v;
                stack.push_back(u);
            }
        }
    }
    if (parent_out) std::memcpy(parent_out, par.data(), (size_t)n * 4);
    return PNR_OK;
}

} // namespace pnr
