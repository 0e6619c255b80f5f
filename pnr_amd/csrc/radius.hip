// radius.hip -- SWC node radii measured from the traced 8-bit volume (pnr_measure_radii).  The rule (include/pnr_hip.h):
//   centre c = (int) fminf(fmaxf(v + 0.5f, 0), n - 1) per coordinate; shell O_k = offsets with (k-1)^2 < d2 <= k^2,
//   d2 = (float)(dx^2 + dy^2) + (zd dz)(zd dz) in f32; voxels outside the volume are not counted; background = V < t with t given,
//   the global mean, or rel_pct of the maximum over O_0 u O_1; k* = the last shell up to which 1000 bg <= bg_permille tot held for
//   every ball O_0 u ... u O_j.
//
// The shells are a host table (build_radius_table: one packed word per offset, raster order inside a shell, shell start indices),
// built once per (rmax, zdist, 2-D) and kept on the device.  One wave measures one node: its lanes stride over the offsets of the
// current shell, gather V with bounds tests, and two ballots / popcounts per 64 offsets keep tot and bg in scalar registers, so the
// test at every shell end is wave-uniform and the wave leaves at the first failing shell -- most nodes stop within a handful of
// shells, nothing like a (2 rmax + 1)^3 cube is ever staged.  The nodes are handed to the waves in the order of the 8^3 cells
// their centres lie in (a host sort; the outputs stay in input order), so that neighbouring waves gather from the same lines.
// The global mean is the byte sum of volume.hip (pnr_mean_threshold).
#include "radius.h"
#include "call.h"
#include "grid.h"
#include "volume.h"
#include <cmath>
#include <cstring>

namespace pnr {

void build_radius_table(float zd, int rmax, bool is2d, RadiusTable &t)
{
    const int rz = is2d ? 0 : rmax;
    const float lim = (float)(rmax * rmax);
    // shell of an offset, -1 = none
    auto shell = [&](int dx, int dy, int dz) -> int {
        if (dx == 0 && dy == 0 && dz == 0) return 0;
        const float d2 = (float)(dx * dx + dy * dy) + (zd * (float)dz) * (zd * (float)dz);
        if (!(d2 > 0.f && d2 <= lim)) return -1; // (also a d2 that is not finite)
        int k = std::max(1, (int)std::ceil(std::sqrt(d2)));
        while (k > 1 && d2 <= (float)((k - 1) * (k - 1))) k--;
        while (d2 > (float)(k * k)) k++;
        return k <= rmax ? k : -1;
    };
    std::vector<int64_t> cnt((size_t)rmax + 2, 0);
    for (int pass = 0; pass < 2; pass++) {
        for (int dz = -rz; dz <= rz; dz++)
            for (int dy = -rmax; dy <= rmax; dy++)
                for (int dx = -rmax; dx <= rmax; dx++) {
                    const int k = shell(dx, dy, dz);
                    if (k < 0) continue;
                    if (pass == 0) cnt[(size_t)k + 1]++;
                    else t.off[(size_t)cnt[(size_t)k]++] = (uint32_t)(dx + 64) | (uint32_t)(dy + 64) << 8 | (uint32_t)(dz + 64) << 16;
                }
        if (pass == 0) {
            for (int k = 0; k <= rmax; k++) cnt[(size_t)k + 1] += cnt[(size_t)k];
            t.start.assign(cnt.begin(), cnt.end()); // (at most 129^3 offsets)
            t.off.assign((size_t)cnt[(size_t)rmax + 1], 0u);
        }
    }
}

} // namespace pnr

namespace {

constexpr int RTPB = 256;          // threads of a work-group: four waves = four nodes
constexpr int RWAVES = RTPB / 64;
constexpr int RUNROLL = 4;         // 64-offset groups of a shell whose gathers are issued together

struct RadArgs {
    const uint8_t *img;
    int w, h, l;
    const uint32_t *off; // the shells (radius.h)
    const int *start;
    const float *xyz;    // n x 3
    const int *order;    // node measured by wave i
    int n;
    int rmax, t_abs, rel_pct, bg_permille;
    int *k_out;
};

__global__ __launch_bounds__(RTPB) void rad_measure(RadArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * RWAVES + (threadIdx.x >> 6);
    if (wv >= a.n) return; // (the whole wave)
    const int node = __builtin_amdgcn_readfirstlane(a.order[wv]);
    const float px = a.xyz[3 * (long long)node], py = a.xyz[3 * (long long)node + 1], pz = a.xyz[3 * (long long)node + 2];
    if (!pnr::finite3(px, py, pz)) {
        if (lane == 0) a.k_out[node] = -1;
        return;
    }
    const int cx = pnr::centre_axis(px, a.w), cy = pnr::centre_axis(py, a.h), cz = pnr::centre_axis(pz, a.l);
    // offset i of the table around the centre: inside the volume? v = its voxel
    auto probe = [&](int i, bool live, unsigned &v) -> bool {
        v = 0;
        if (!live) return false;
        const unsigned o = a.off[i];
        const int x = cx + (int)(o & 255u) - 64, y = cy + (int)((o >> 8) & 255u) - 64, z = cz + (int)((o >> 16) & 255u) - 64;
        const bool inb = (unsigned)x < (unsigned)a.w && (unsigned)y < (unsigned)a.h && (unsigned)z < (unsigned)a.l;
        if (inb) v = a.img[pnr::voxel_index(a.w, a.h, x, y, z)];
        return inb;
    };
    int t = a.t_abs;
    if (a.rel_pct > 0) { // per node: rel_pct of the maximum over O_0 u O_1 (at most 7 voxels), rounded up, at least 1
        unsigned m = 0;
        const int s1 = a.start[2];
        for (int base = 0; base < s1; base += 64) {
            unsigned v;
            probe(base + lane, base + lane < s1, v);
            m = max(m, v);
        }
        for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
        t = max(1, (a.rel_pct * (int)m + 99) / 100);
    }
    unsigned tot = 0, bg = 0; // of the ball O_0 u ... u O_k: wave-uniform
    int k = 0;
    for (; k <= a.rmax; k++) {
        const int s0 = a.start[k], s1 = a.start[k + 1];
        for (int base = s0; base < s1; base += 64 * RUNROLL) {
            unsigned v[RUNROLL];
            bool inb[RUNROLL];
#pragma unroll
            for (int u = 0; u < RUNROLL; u++) {
                const int i = base + 64 * u + lane;
                inb[u] = probe(i, i < s1, v[u]);
            }
#pragma unroll
            for (int u = 0; u < RUNROLL; u++) {
                tot += (unsigned)__popcll(__ballot(inb[u]));
                bg += (unsigned)__popcll(__ballot(inb[u] && (int)v[u] < t));
            }
        }
        if (1000ull * bg > (unsigned long long)a.bg_permille * tot) break;
    }
    // the test failed at shell k: k* = k - 1 (0 when it failed at shell 0 or 1); it never failed: rmax
    if (lane == 0) a.k_out[node] = k > a.rmax ? a.rmax : max(0, k - 1);
}

} // namespace

int pnr_radius_run(pnr_ctx *c, const float *xyz, int64_t n, const pnr_radius_opts &o, int32_t *k_out, int32_t *thr_used)
{
    static const char *who = "pnr_measure_radii";
    pnr::Call call(c, who);
    const bool is2d = c->l == 1;
    // the shells of (rmax, zdist, 2-D), kept in the context: the table of the last call, or a new one.  Another rmax gets buffers of
    // exactly its size; the 2-D and the 3-D table of one rmax share what the larger needs (dev_alloc only grows), so a change of
    // volume alone frees nothing
    uint32_t zbits;
    std::memcpy(&zbits, &c->prm.zdist, 4);
    int rc = PNR_OK;
    if (c->rad_rmax != o.rmax || c->rad_zbits != zbits || c->rad_2d != is2d) {
        pnr::RadiusTable t;
        pnr::build_radius_table(c->prm.zdist, o.rmax, is2d, t);
        if (c->rad_rmax != o.rmax) c->d_rad_off.reset(), c->d_rad_start.reset();
        c->rad_rmax = 0;
        if ((rc = pnr::dev_alloc(c->d_rad_off, t.off.size(), who, "for the shell table"))) return rc;
        if ((rc = pnr::dev_alloc(c->d_rad_start, t.start.size(), who, "for the shell table"))) return rc;
        call.up(c->d_rad_off.get(), t.off.data(), t.off.size());
        call.up(c->d_rad_start.get(), t.start.data(), t.start.size());
        if ((rc = call.finish())) return rc; // (the host table ends here)
        c->rad_rmax = o.rmax, c->rad_zbits = zbits, c->rad_2d = is2d;
    }
    // device buffers of the call: the sum | the positions | the order of the nodes | k
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_sum = buf.add<unsigned long long>(1);
    const auto d_xyz = buf.add<float>((size_t)n * 3);
    const auto d_ord = buf.add<int>((size_t)n), d_k = buf.add<int>((size_t)n);
    if ((rc = buf.alloc(who))) return rc;
    int t_abs = o.rel_pct ? 0 : o.thr;
    if (t_abs < 0 && (rc = pnr_mean_threshold(c, who, "radius", c->d_img, c->N, d_sum, &t_abs))) return rc; // the global mean
    if (thr_used) *thr_used = t_abs;
    if (n > 0) {
        // the order of the 8^3 cells of the centres (positions that are not measured last); it changes no result
        std::vector<std::pair<uint64_t, int>> cell((size_t)n);
        const uint64_t nx8 = (uint64_t)(c->w + 7) >> 3, ny8 = (uint64_t)(c->h + 7) >> 3;
        auto centre = [](float v, int64_t ext) { return (uint64_t)pnr::centre_axis(v, (int)ext); };
        for (int64_t i = 0; i < n; i++) {
            const float *p = xyz + 3 * i;
            uint64_t id = ~0ull;
            if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))
                id = ((centre(p[2], c->l) >> 3) * ny8 + (centre(p[1], c->h) >> 3)) * nx8 + (centre(p[0], c->w) >> 3);
            cell[(size_t)i] = {id, (int)i};
        }
        std::sort(cell.begin(), cell.end());
        std::vector<int> order((size_t)n);
        for (int64_t i = 0; i < n; i++) order[(size_t)i] = cell[(size_t)i].second;
        call.up(d_xyz, xyz);
        call.up(d_ord, order.data());
        const RadArgs a{c->d_img, (int)c->w, (int)c->h, (int)c->l, c->d_rad_off.get(), c->d_rad_start.get(), d_xyz, d_ord, (int)n, o.rmax, t_abs, o.rel_pct, o.bg_permille, d_k};
        call.timed("radius", rad_measure, dim3((unsigned)((n + RWAVES - 1) / RWAVES)), dim3(RTPB), a);
        call.down(k_out, d_k);
        return call.finish(); // (the host vectors above end here)
    }
    return PNR_OK;
}
