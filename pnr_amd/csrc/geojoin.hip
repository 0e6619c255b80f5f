// geojoin.hip -- the traced forest joined along the signal (pnr_geodesic_bridges, pnr_join_expand).  The rule (include/pnr_hip.h): the
// sources are the sample points of the forest, labelled with their trees; D and L are the geodesic keys; every pair of 26-neighbours p,
// q = p + o (o among the last 13 of the offset order) with L(p) != L(q) is a meet edge of weight W = D(p) + wt(p, q) + D(q) and key
// (W, p, o - 13); the bridges are the unique minimum spanning forest of the trees under that key (Mehlhorn 1988: a minimum spanning tree of
// the graph of touching Voronoi cells is one of the complete graph of pairwise geodesic distances, so the one geodesic pass suffices).
//
// Boruvka's rounds over the settled keys, which stay on the device (the hook of pnr_geodesic_run).  Trees are numbered 0 .. T - 1 in
// ascending label order, so the keys carry the tree number and order as the labels do.  The host keeps the union-find; per round it
// uploads comp[tree] = the current component, or -1 for one that has left the search, and two kernels sweep all tiles:
//   gj_meet_w  for every meet edge between two different live components within the limit: best_w[c] = min(W), both sides.
//   gj_meet_e  for every such edge with W == best_w[c]: best_e[c] = min((13 p + (o - 13)) << 22 | c'), c' the component on the other
//              side (below 2^22; the edge decides it, so the order is that of 13 p + (o - 13) < 2^36).
// Together they give each component its minimum edge under the full key, and whom it meets there; the host unites.  A component whose
// best_w stayed all ones has no edge within the limit and leaves; the loop ends when a round finds nothing.
// A work-group stages D, the component and the byte of a tile of GEO_TX x GEO_TY x GEO_TZ voxels with the halo the 13 offsets reach
// (x: -1 .. TX, y: -1 .. TY, z: 0 .. TZ) in LDS, so a key is read once per tile and not once per pair; the
// cost of a byte is looked up where two components meet, which is rare.  A thread owns a z column; its
// candidates go through two registers (the last two components it met), then a 64-slot LDS table (component -> minimum; a full
// neighbourhood falls through to the global atomic), and the table is flushed with at most 64 global 64-bit atomic minima per tile: a
// large Voronoi face costs its tiles two atomics each.  Minima over fixed sets: tiling, launch cuts, rounds and arrival order change no bit.
// Below the kernels: the host side -- sources, the rounds, the bridges' paths through the target stage of the geodesic call, attachment,
// and the expansion.
#include "geojoin.h"
#include "call.h"
#include "grid.h"
#include "tilework.h"
#include "distance.h"
#include "join.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

namespace {

using pnr::GEO_TX;
using pnr::GEO_TY;
using pnr::GEO_TZ;
using Dims = pnr::GeoDims;
using Lens = pnr::GeoLens;
typedef unsigned long long u64;

constexpr u64 NONE = ~0ull;
constexpr int JX = GEO_TX + 2, JY = GEO_TY + 2, JZ = GEO_TZ + 1, JCELLS = JX * JY * JZ;
constexpr int JTPB = GEO_TX * GEO_TY; // threads of a work-group
constexpr int SLOTS = 64;             // of the LDS table (a power of two)
constexpr int PROBES = 4;
constexpr int OTHER_BITS = 22;        // the other side's component in best_e (trees < 2^22 = PNR_JOIN_MAX_N)
constexpr int32_t FIRST_CAP = 256;      // voxels of a bridge's walk in the first target stage; only a longer one is walked again with the full cap
static_assert(JTPB % 64 == 0 && JTPB <= 1024 && JTPB >= SLOTS, "whole waves, and a thread per slot");
static_assert(PNR_JOIN_MAX_N <= 1 << OTHER_BITS, "a tree number fits the low bits of best_e");

struct MeetArgs {
    const uint8_t *V;
    const u64 *key;
    const uint16_t *ctab;
    const int *comp; // tree -> its current component, -1: it has left the search
    u64 *best;       // best_w (gj_meet_w) or best_e (gj_meet_e)
    const u64 *best_w;
    Dims d;
    int t, trees;
    long long tile0; // the first tile of this launch
    u64 limit;       // 0: none
    Lens len;
};

struct Tile {
    unsigned d[JCELLS];
    int comp[JCELLS]; // -1: outside, impassable, unreached, or of a component that has left
    unsigned char val[JCELLS];
    int slot_comp[SLOTS];
    u64 slot_val[SLOTS];
};

__device__ inline void table_put(Tile &s, u64 *best, int comp, u64 v)
{
    unsigned at = ((unsigned)comp * 2654435761u) >> 26;
    for (int k = 0; k < PROBES; k++, at = (at + 1) & (SLOTS - 1)) {
        const int old = atomicCAS(&s.slot_comp[at], -1, comp);
        if (old == -1 || old == comp) {
            atomicMin(&s.slot_val[at], v);
            return;
        }
    }
    atomicMin(&best[comp], v); // (more components in one tile than the table takes)
}

// the last two components a thread met
struct Pair {
    int c0 = -1, c1 = -1;
    u64 v0 = NONE, v1 = NONE;
};
__device__ inline void pair_put(Pair &a, Tile &s, u64 *best, int comp, u64 v)
{
    if (comp == a.c0) a.v0 = min(a.v0, v);
    else if (comp == a.c1) a.v1 = min(a.v1, v);
    else {
        if (a.c1 >= 0) table_put(s, best, a.c1, a.v1);
        a.c1 = a.c0, a.v1 = a.v0, a.c0 = comp, a.v0 = v;
    }
}

template <bool EDGE>
__device__ inline void meet(const MeetArgs &a, Tile &s)
{
    const Dims d = a.d;
    const pnr::TileAt o = pnr::tile_origin((unsigned)(a.tile0 + blockIdx.x), d.ntx, d.nty, GEO_TX, GEO_TY, GEO_TZ);
    const int x0 = o.x0, y0 = o.y0, z0 = o.z0;
    if (threadIdx.x < SLOTS) s.slot_comp[threadIdx.x] = -1, s.slot_val[threadIdx.x] = NONE;
    // (the component of a tree is the same word for most cells of a tile; the cost of a byte is looked up where two components meet, which is rare)
#pragma unroll
    for (int it = 0; it < (JCELLS + JTPB - 1) / JTPB; it++) {
        const int cell = it * JTPB + (int)threadIdx.x;
        if (cell >= JCELLS) break;
        const int gx = x0 + cell % JX - 1, gy = y0 + cell / JX % JY - 1, gz = z0 + cell / (JX * JY);
        unsigned dd = 0;
        int cc = -1;
        unsigned char val = 0;
        if (gx >= 0 && gx < d.w && gy >= 0 && gy < d.h && gz < d.l) {
            const long long g = pnr::voxel_index(d.w, d.h, gx, gy, gz);
            const u64 k = a.key[g];
            val = a.V[g];
            if ((int)val >= a.t && k != NONE && (unsigned)k < (unsigned)a.trees) dd = (unsigned)(k >> 32), cc = a.comp[(unsigned)k];
        }
        s.d[cell] = dd, s.comp[cell] = cc, s.val[cell] = val;
    }
    __syncthreads();
    const int lx = threadIdx.x % GEO_TX, ly = threadIdx.x / GEO_TX;
    Pair acc;
#pragma unroll
    for (int z = 0; z < GEO_TZ; z++) {
        const int own = (z * JY + ly + 1) * JX + lx + 1;
        const int cp = s.comp[own];
        if (cp < 0) continue;
        const long long p = pnr::voxel_index(d.w, d.h, x0 + lx, y0 + ly, z0 + z);
        unsigned costp = 0; // (0: not looked up yet; a cost is at least 1)
        u64 wp = 0;
#pragma unroll
        for (int k = 14; k < 27; k++) { // the last 13 of the offset order: q has the larger linear index
            const int dx = k % 3 - 1, dy = k / 3 % 3 - 1, dz = k / 9 - 1;
            const int q = own + (dz * JY + dy) * JX + dx;
            const int cq = s.comp[q];
            if (cq < 0 || cq == cp) continue;
            if (!costp) {
                costp = a.ctab[s.val[own]];
                if (EDGE) wp = a.best_w[cp];
            }
            const u64 W = (u64)s.d[own] + (u64)(a.len.v[k] * (costp + a.ctab[s.val[q]])) + s.d[q]; // (the edge is at most 2^31 - 1: checked by the host)
            if (a.limit && W > a.limit) continue;
            if (!EDGE) {
                pair_put(acc, s, a.best, cp, W);
                pair_put(acc, s, a.best, cq, W);
            } else {
                const u64 e = (u64)(13 * p + (k - 14)) << OTHER_BITS;
                if (W == wp) pair_put(acc, s, a.best, cp, e | (unsigned)cq);
                if (W == a.best_w[cq]) pair_put(acc, s, a.best, cq, e | (unsigned)cp);
            }
        }
    }
    if (acc.c0 >= 0) table_put(s, a.best, acc.c0, acc.v0);
    if (acc.c1 >= 0) table_put(s, a.best, acc.c1, acc.v1);
    __syncthreads();
    if (threadIdx.x < SLOTS && s.slot_comp[threadIdx.x] >= 0) atomicMin(&a.best[s.slot_comp[threadIdx.x]], s.slot_val[threadIdx.x]);
}

__global__ __launch_bounds__(JTPB) void gj_meet_w(MeetArgs a)
{
    __shared__ Tile s;
    meet<false>(a, s);
}

__global__ __launch_bounds__(JTPB) void gj_meet_e(MeetArgs a)
{
    __shared__ Tile s;
    meet<true>(a, s);
}

struct Edge { // the key (W, p, o - 13) as (w, e = 13 p + (o - 13)), and the two components it joined
    uint64_t w, e;
    int32_t c0, c1;
    bool operator<(const Edge &o) const { return w != o.w ? w < o.w : e < o.e; }
    bool operator==(const Edge &o) const { return w == o.w && e == o.e; }
};

// the centre voxel of the radius rule: the function the device calls
inline int64_t centre(const Dims &d, const float *p) { return pnr::centre_voxel(d.w, d.h, d.l, p[0], p[1], p[2]); }

// what the hook leaves for the second half of the call
struct Rounds {
    int64_t trees = 0, n_src = 0;
    uint64_t limit = 0;
    unsigned weight_min = 0; // the smallest edge weight of the call: a path of cost D has at most D / weight_min steps
    const float *src_xyz = nullptr;
    std::vector<Edge> edges; // the bridges in ascending key order
    int64_t rounds = 0;
    Dims d{};
    // the targets: the bridges' p voxels | their q voxels | the sources; every walk first with the cap first_cap, the cut ones again with `cap`
    std::vector<float> at, at_long;
    std::vector<uint32_t> d_at;
    std::vector<int32_t> l_at, path_len, long_len, long_of; // long_of[target]: its row in long_vox, or -1
    std::vector<int64_t> path_vox, long_vox;
    int32_t cap = 0, first_cap = 0;
    // the walk of target i: its voxels and their number (negative: cut at the cap of the call)
    const int64_t *walk(size_t i, int32_t &len) const
    {
        const int32_t at_long_row = long_of[i];
        len = at_long_row < 0 ? path_len[i] : long_len[(size_t)at_long_row];
        return at_long_row < 0 ? &path_vox[i * (size_t)first_cap] : &long_vox[(size_t)at_long_row * (size_t)cap];
    }
};

int meet_rounds(pnr_ctx *c, const char *who, const pnr_geo_keys &k, Rounds &r)
{
    const Dims d = k.d;
    const int64_t tiles = d.tiles(), T = r.trees;
    const int64_t per_launch = pnr::tiles_per_launch(c->opt.geojoin_tiles_per_launch);
    const int launches = (int)((tiles + per_launch - 1) / per_launch);
    pnr::CallBuf buf; // (freed when the rounds are over)
    const auto d_comp = buf.add<int>((size_t)T);
    const auto d_w = buf.add<u64>((size_t)T), d_e = buf.add<u64>((size_t)T);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::UnionFind uf(T);
    std::vector<int32_t> comp((size_t)T);
    std::vector<char> gone((size_t)T, 0); // per representative: no edge within the limit -- it can never be joined
    std::vector<u64> bw((size_t)T), be((size_t)T);
    std::vector<Edge> found;
    r.edges.clear();
    r.rounds = 0;
    while (T >= 2) { // (until a round finds nothing)
        for (int64_t t = 0; t < T; t++) {
            const int32_t rep = uf.find((int32_t)t);
            comp[(size_t)t] = gone[(size_t)rep] ? -1 : rep;
        }
        pnr::Call call(c, who);
        call.up(d_comp, comp.data());
        call.fill(d_w, 0xff);
        call.fill(d_e, 0xff);
        MeetArgs a{k.V, k.key, k.ctab, d_comp.get(), d_w.get(), d_w.get(), d, k.t, (int)T, 0, r.limit, k.len};
        c->tic();
        for (a.tile0 = 0; a.tile0 < tiles; a.tile0 += per_launch) call.launch(gj_meet_w, dim3((unsigned)std::min<int64_t>(per_launch, tiles - a.tile0)), dim3(JTPB), a);
        c->toc("geojoin_meet_w", launches);
        a.best = d_e.get();
        c->tic();
        for (a.tile0 = 0; a.tile0 < tiles; a.tile0 += per_launch) call.launch(gj_meet_e, dim3((unsigned)std::min<int64_t>(per_launch, tiles - a.tile0)), dim3(JTPB), a);
        c->toc("geojoin_meet_e", launches);
        call.down(bw.data(), d_w);
        call.down(be.data(), d_e);
        if ((rc = call.finish())) return rc;
        r.rounds++;
        found.clear();
        for (int64_t t = 0; t < T; t++) {
            if (comp[(size_t)t] != (int32_t)t) continue; // (a live representative)
            if (bw[(size_t)t] == NONE) {
                gone[(size_t)t] = 1;
                continue;
            }
            const int64_t other = (int64_t)(be[(size_t)t] & ((1u << OTHER_BITS) - 1));
            PNR_REQUIRE(be[(size_t)t] != NONE && other < T && comp[(size_t)other] == (int32_t)other && other != t, PNR_E_HIP, "%s: round %lld left component %lld without its edge",
                        who, (long long)r.rounds, (long long)t);
            found.push_back(Edge{bw[(size_t)t], be[(size_t)t] >> OTHER_BITS, (int32_t)std::min(t, other), (int32_t)std::max(t, other)});
        }
        if (found.empty()) break;
        std::sort(found.begin(), found.end());
        found.erase(std::unique(found.begin(), found.end()), found.end());
        for (const Edge &e : found)
            if (uf.unite(e.c0, e.c1)) r.edges.push_back(e);
    }
    std::sort(r.edges.begin(), r.edges.end());
    return PNR_OK;
}

// the hook of the geodesic call: the rounds, then the bridges' two voxels and the sources through the target stage
int settled(void *user, pnr_ctx *c, const char *who, const pnr_geo_keys &k, pnr_geo_call &g)
{
    Rounds &r = *(Rounds *)user;
    r.d = k.d;
    int rc = meet_rounds(c, who, k, r);
    if (rc) return rc;
    const Dims d = k.d;
    const size_t K = r.edges.size(), m = 2 * K + (size_t)r.n_src;
    r.at.resize(3 * m);
    uint64_t w_max = 0;
    for (size_t i = 0; i < K; i++) {
        const int64_t p = (int64_t)(r.edges[i].e / 13);
        const int kk = (int)(r.edges[i].e % 13) + 14;
        const int x = (int)(p % d.w), y = (int)(p / d.w % d.h), z = (int)(p / ((int64_t)d.w * d.h));
        float *a = &r.at[3 * i], *b = &r.at[3 * (K + i)]; // (exact: the extents are below 2^24)
        a[0] = (float)x, a[1] = (float)y, a[2] = (float)z;
        b[0] = (float)(x + kk % 3 - 1), b[1] = (float)(y + kk / 3 % 3 - 1), b[2] = (float)(z + kk / 9 - 1);
        w_max = std::max(w_max, r.edges[i].w);
    }
    if (r.n_src) std::memcpy(&r.at[6 * K], r.src_xyz, sizeof(float) * 3 * (size_t)r.n_src);
    // W >= D(p), D(q), and a step costs at least weight_min: no path has more voxels than this (never more than the cap of the call)
    r.cap = (int32_t)std::min<uint64_t>(PNR_GEO_MAX_PATH, r.weight_min ? w_max / r.weight_min + 2 : PNR_GEO_MAX_PATH);
    r.d_at.assign(m, 0);
    r.l_at.assign(m, -1);
    r.path_len.assign(2 * K, 0);
    r.first_cap = std::min(FIRST_CAP, r.cap);
    r.path_vox.resize(2 * K * (size_t)r.first_cap);
    r.long_of.assign(2 * K, -1);
    pnr_geo_call t{};
    t.at_xyz = r.at.data(), t.m = (int64_t)m, t.m_no_path = r.n_src, t.d_at = r.d_at.data(), t.label_at = r.l_at.data();
    t.path_cap = K ? r.first_cap : 0, t.path_len = r.path_len.data(), t.path_vox = r.path_vox.data();
    if ((rc = pnr_geo_targets(c, who, k, t))) return rc;
    // the walks that did not fit, with the cap of the call
    for (size_t i = 0; i < 2 * K && r.cap > FIRST_CAP; i++)
        if (r.path_len[i] < 0) {
            r.long_of[i] = (int32_t)(r.at_long.size() / 3);
            r.at_long.insert(r.at_long.end(), &r.at[3 * i], &r.at[3 * i] + 3);
        }
    if (!r.at_long.empty()) {
        const size_t nl = r.at_long.size() / 3;
        r.long_len.assign(nl, 0);
        r.long_vox.resize(nl * (size_t)r.cap);
        pnr_geo_call u{};
        u.at_xyz = r.at_long.data(), u.m = (int64_t)nl, u.path_cap = r.cap, u.path_len = r.long_len.data(), u.path_vox = r.long_vox.data();
        if ((rc = pnr_geo_targets(c, who, k, u))) return rc;
    }
    g.at_xyz = nullptr, g.m = 0; // (the stage has run)
    return PNR_OK;
}

} // namespace

int pnr_geojoin_run(pnr_ctx *c, const float *xyz, const int32_t *parent, int64_t n, const pnr_geojoin_opts &o, pnr_geojoin_info *info, std::vector<pnr_geo_bridge> &bridges,
                    std::vector<int64_t> &chain)
{
    static const char *who = "pnr_geodesic_bridges";
    bridges.clear();
    chain.clear();
    c->geojoin_rounds = 0;
    // the trees, numbered in ascending label order
    std::vector<int32_t> label((size_t)n), tree_of((size_t)n, -1);
    int rc = pnr::join_input_trees(parent, n, label.data(), who);
    if (rc) return rc;
    Rounds r;
    for (int64_t i = 0; i < n; i++)
        if (label[(size_t)i] == (int32_t)i) tree_of[(size_t)i] = (int32_t)r.trees++;
    // the sources
    int64_t np = 0;
    if ((rc = pnr::tree_sample(xyz, parent, n, 1.f, o.step, nullptr, nullptr, 0, &np))) return rc;
    PNR_REQUIRE(np <= PNR_RADIUS_MAX_N, PNR_E_ARG, "%s: %lld sample points (at most 2^28): raise the step", who, (long long)np);
    std::vector<float> pts((size_t)np * 3);
    std::vector<int32_t> owner((size_t)np), src_tree((size_t)np);
    if ((rc = pnr::tree_sample(xyz, parent, n, 1.f, o.step, pts.data(), owner.data(), np, &np))) return rc;
    for (int64_t k = 0; k < np; k++) src_tree[(size_t)k] = tree_of[(size_t)label[(size_t)owner[(size_t)k]]];
    PNR_REQUIRE(c->w < (1 << 24) && c->h < (1 << 24) && c->l < (1 << 24), PNR_E_ARG, "%s: an extent of %lld x %lld x %lld is 2^24 or more (voxel coordinates must be exact in f32)",
                who, (long long)c->w, (long long)c->h, (long long)c->l);
    r.n_src = np, r.src_xyz = pts.data(), r.limit = o.limit;
    unsigned cmin = 0xffff, lmin = ~0u;
    for (int v = 0; v < 256; v++) cmin = std::min<unsigned>(cmin, o.cost ? o.cost[v] : (unsigned)(256 - v));
    {
        const float zd = c->prm.zdist; // the smallest of the step lengths of geodesic.hip: (1, 0, 0) or (0, 0, 1)
        const float fz = rintf(32.0f * sqrtf(0.f + (zd * 1.f) * (zd * 1.f)));
        lmin = fz >= 0.f && fz < 32.f && c->l > 1 ? (unsigned)fz : 32u;
    }
    r.weight_min = lmin * 2 * cmin;
    const pnr_geo_opts go{o.thr, o.limit == 0 || o.limit > 0x7fffffffull ? 0x7fffffffu : (uint32_t)o.limit, o.cost};
    pnr_geo_info gi{};
    pnr_geo_call g{};
    g.src_xyz = pts.data(), g.src_label = src_tree.data(), g.n_src = np, g.info = &gi, g.hook = settled, g.hook_user = &r;
    if ((rc = pnr_geodesic_run(c, who, go, g))) return rc;
    c->geojoin_rounds = r.rounds;
    // the trees that take part, and the first sample point of every source voxel's tree on it
    const size_t K = r.edges.size();
    const Dims d = r.d;
    std::vector<char> part((size_t)r.trees, 0);
    std::unordered_map<int64_t, int32_t> first_at;
    for (int64_t k = 0; k < np; k++)
        if (r.d_at[2 * K + (size_t)k] == 0 && r.l_at[2 * K + (size_t)k] == src_tree[(size_t)k]) {
            part[(size_t)src_tree[(size_t)k]] = 1;
            first_at.emplace(centre(d, &pts[3 * (size_t)k]), (int32_t)k);
        }
    int64_t lost = 0, inserted = 0;
    for (int64_t t = 0; t < r.trees; t++) lost += !part[(size_t)t];
    uint64_t w_max = 0;
    for (size_t i = 0; i < K; i++) {
        int32_t lp = 0, lq = 0;
        const int64_t *vp = r.walk(i, lp), *vq = r.walk(K + i, lq);
        PNR_REQUIRE(lp >= 0 && lq >= 0, PNR_E_ARG, "%s: the path of bridge %zu was cut at the cap of %d voxels (PNR_GEO_MAX_PATH)", who, i, r.cap);
        PNR_REQUIRE(lp > 0 && lq > 0 && r.l_at[i] != r.l_at[K + i], PNR_E_HIP, "%s: bridge %zu has no path to its two trees", who, i);
        const auto ia = first_at.find(vp[lp - 1]), ib = first_at.find(vq[lq - 1]);
        PNR_REQUIRE(ia != first_at.end() && ib != first_at.end(), PNR_E_HIP, "%s: bridge %zu ends on a voxel without a source", who, i);
        const int64_t p = (int64_t)(r.edges[i].e / 13);
        bridges.push_back(pnr_geo_bridge{owner[(size_t)ia->second], owner[(size_t)ib->second], p, (int32_t)(r.edges[i].e % 13) + 13, lp + lq, r.edges[i].w, (int64_t)chain.size()});
        for (int32_t j = lp; j-- > 0;) chain.push_back(vp[j]);
        chain.insert(chain.end(), vq, vq + lq);
        inserted += lp + lq - 2;
        w_max = std::max(w_max, r.edges[i].w);
    }
    if (info) *info = pnr_geojoin_info{r.trees, lost, r.trees - (int64_t)K, (int64_t)K, inserted, gi.n_src, gi.n_src_dropped, w_max, gi.thr_used, (int32_t)std::min<int64_t>(r.rounds, INT32_MAX)};
    return PNR_OK;
}

int pnr_geojoin_expand(const float *xyz, const int32_t *parent, int64_t n, const pnr_geo_bridge *bridges, int64_t nb, const int64_t *path_vox, int64_t n_path, int64_t w, int64_t h,
                       int64_t l, float *xyz_out, int32_t *parent_out, int32_t *bridge_of, int64_t cap_nodes, int64_t *n_nodes, pnr_bridge *join_out)
{
    static const char *who = "pnr_join_expand";
    const int64_t N = w * h * l;
    int64_t total = n;
    for (int64_t k = 0; k < nb; k++) {
        const pnr_geo_bridge &b = bridges[k];
        PNR_REQUIRE(b.a >= 0 && b.a < n && b.b >= 0 && b.b < n && b.a != b.b, PNR_E_ARG, "%s: bridge %lld = (%d, %d) outside [0, %lld)", who, (long long)k, b.a, b.b, (long long)n);
        PNR_REQUIRE(b.path_len >= 2 && b.path_off >= 0 && b.path_off <= n_path - b.path_len, PNR_E_ARG, "%s: bridge %lld: a path of %d voxels from %lld, of %lld in all", who,
                    (long long)k, b.path_len, (long long)b.path_off, (long long)n_path);
        for (int32_t j = 0; j < b.path_len; j++)
            PNR_REQUIRE(path_vox[b.path_off + j] >= 0 && path_vox[b.path_off + j] < N, PNR_E_ARG, "%s: bridge %lld: voxel %lld outside the %lld voxels of the grid", who, (long long)k,
                        (long long)path_vox[b.path_off + j], (long long)N);
        total += b.path_len - 2;
        PNR_REQUIRE(total <= PNR_JOIN_MAX_N, PNR_E_ARG, "%s: more than 2^22 nodes with the inserted ones", who);
    }
    *n_nodes = total;
    const bool fits = total <= cap_nodes;
    if (fits && xyz_out) std::memcpy(xyz_out, xyz, sizeof(float) * 3 * (size_t)n);
    if (fits && parent_out)
        for (int64_t i = 0; i < n; i++) parent_out[i] = parent[i] < 0 ? -1 : parent[i];
    int64_t at = n;
    for (int64_t k = 0; k < nb; k++) {
        const pnr_geo_bridge &b = bridges[k];
        int32_t prev = b.a;
        for (int32_t j = 1; j + 1 < b.path_len; j++, at++) {
            const int64_t g = path_vox[b.path_off + j];
            if (fits && xyz_out) xyz_out[3 * at] = (float)(g % w), xyz_out[3 * at + 1] = (float)(g / w % h), xyz_out[3 * at + 2] = (float)(g / (w * h));
            if (fits && parent_out) parent_out[at] = prev;
            if (fits && bridge_of) bridge_of[at - n] = (int32_t)k;
            prev = (int32_t)at;
        }
        if (join_out) join_out[k] = pnr_bridge{std::min(prev, b.b), std::max(prev, b.b), (float)((double)b.w / 64.0)};
    }
    return PNR_OK;
}
