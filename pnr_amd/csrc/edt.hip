// edt.hip -- the exact anisotropic Euclidean distance transform of the traced u8 volume (pnr_distance_transform).  The rule
// (include/pnr_hip.h): foreground V >= t; for a foreground voxel p, D2(p) = min(cap, min over the background voxels q inside the volume of
// (float)(dx^2 + dy^2) + (zd (float)dz) (zd (float)dz)), cap = (float)(rmax^2); background voxels get 0.
//
// Why three separable passes give the same bits.  dx^2 + dy^2 < 2^24 is exact in f32, and for a fixed dz the rounded sum fl(a + c) is
// non-decreasing in a, so the minimum over a plane may be taken in integers before the one f32 addition:
//   gx(x, y, z) = min over the background x' of the row of (x - x')^2
//   gy(x, y, z) = min over y' of gx(x, y', z) + (y - y')^2
//   D2(x, y, z) = min over z' of (float)gy(x, y, z') + zt2[|z - z'|],   zt2[k] = (zd (float)k) (zd (float)k)
// A minimum does not depend on order, and min(cap, .) commutes with the later minima (they only add non-negative terms), so gx and gy
// are clamped at rmax^2: a row or plane without background simply holds the clamp.
//
//   edt_x      one wave per row, in words of EDT_WX voxels: __ballot(V < t) is the word's background mask, the nearest set bit below /
//              above a lane comes from clz / ctz of the masked word, and the last / next background position outside the word is
//              carried along the row.  A backward sweep leaves every word's carry from the right (one int per word, written and read
//              back by the same lane), the forward sweep carries the left one and writes min(|dx|, rmax) as u16: every load and store
//              is a wave of consecutive addresses.
//   edt_y      a thread per voxel, threads along x: best = gx^2; k = 1, 2, ... to both sides while k^2 < best.  Exact and bounded: a
//              candidate at distance k is at least k^2.  Its cost is the distance found.  Writes gy (u32, at most rmax^2 <= 2^20).
//   edt_z      the same along z in f32: stops when zt2[k] >= best (zt2 is non-decreasing and every candidate is at least zt2[k]); since
//              zd >= 1, zt2[rmax] >= cap >= best, so k never passes rmax.  zt2 is a host table in f32 under this file's flags.
//   edt_stats  n_fg (D2 > 0: a foreground voxel is at least 1 away from any background), n_capped, and the maximum with its smallest
//              index as one 64-bit atomic maximum of (bits(D2) << 32) | ~index per work-group (D2 >= +0: its bits order like its value).
//   edt_sample D2 at the centre voxels of the radius rule.
// Background voxels write 0 and do no work.  Device memory of a call: 4 N bytes that hold gx (u16) and then D2, 4 N bytes that hold the
// row carries of the x pass and then gy, the table, four words, and the points.
#include "edt.h"
#include "call.h"
#include "grid.h"
#include "volume.h"
#include <cstring>

namespace {

using pnr::EDT_ROWS;
using pnr::EDT_TPB;
using pnr::EDT_WX;

constexpr int XTPB = EDT_ROWS * 64; // threads of a work-group of the x pass: one wave per row
static_assert(EDT_WX == 64, "a word of the x pass is one ballot of a wave");
static_assert(EDT_TPB % 64 == 0 && EDT_TPB <= 1024, "whole waves");

struct XArgs {
    const uint8_t *V;
    uint16_t *gx; // N
    int *carry;   // rows x words: the nearest background x to the right of the word, -1 = none
    long long rows;
    int w, words, t, rmax;
};

__global__ __launch_bounds__(XTPB) void edt_x(XArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * EDT_ROWS + (threadIdx.x >> 6);
    if (row >= a.rows) return; // (the whole wave)
    const uint8_t *v = a.V + row * a.w;
    uint16_t *g = a.gx + row * a.w;
    int *carry = a.carry + row * a.words;
    int next = -1;
    for (int j = a.words - 1; j >= 0; j--) {
        const long long x = (long long)j * EDT_WX + lane;
        const unsigned long long m = __ballot(x < a.w && (int)v[x] < a.t);
        if (lane == (j & 63)) carry[j] = next; // (read back by this lane below)
        if (m) next = j * EDT_WX + __ffsll(m) - 1;
    }
    int last = -1;
    for (int j = 0; j < a.words; j++) {
        const long long x = (long long)j * EDT_WX + lane;
        const bool inside = x < a.w;
        const bool bg = inside && (int)v[x] < a.t;
        const unsigned long long m = __ballot(bg);
        int own = 0;
        if (lane == (j & 63)) own = carry[j];
        next = __shfl(own, j & 63, 64);
        if (inside) {
            int d = 0;
            if (!bg) {
                const unsigned long long below = m & ((1ull << lane) - 1ull), above = m >> lane; // (bit `lane` itself is clear)
                int left = a.rmax, right = a.rmax;
                if (below) left = lane - (63 - __clzll(below));
                else if (last >= 0) left = (int)min(x - last, (long long)a.rmax);
                if (above) right = __ffsll(above) - 1;
                else if (next >= 0) right = (int)min((long long)next - x, (long long)a.rmax);
                d = min(min(left, right), a.rmax);
            }
            g[x] = (uint16_t)d;
        }
        if (m) last = j * EDT_WX + 63 - __clzll(m);
    }
}

__global__ __launch_bounds__(EDT_TPB) void edt_y(const uint16_t *gx, unsigned *gy, int w, int h, long long N)
{
    const long long i = (long long)blockIdx.x * EDT_TPB + threadIdx.x;
    if (i >= N) return;
    const unsigned g = gx[i];
    unsigned best = g * g;
    if (best > 1u) { // (1: no k with k^2 < best)
        const int y = (int)((i / w) % h);
        for (int k = 1; (unsigned)(k * k) < best; k++) {
            const bool up = k <= y, down = k < h - y;
            if (!up && !down) break;
            if (up) {
                const unsigned q = gx[i - (long long)k * w];
                best = min(best, q * q + (unsigned)(k * k));
            }
            if (down) {
                const unsigned q = gx[i + (long long)k * w];
                best = min(best, q * q + (unsigned)(k * k));
            }
        }
    }
    gy[i] = best;
}

__global__ __launch_bounds__(EDT_TPB) void edt_z(const unsigned *gy, float *d2, const float *zt2, long long plane, int l, int rmax, long long N)
{
    const long long i = (long long)blockIdx.x * EDT_TPB + threadIdx.x;
    if (i >= N) return;
    float best = (float)gy[i];
    if (best > 0.f) {
        const int z = (int)(i / plane);
        for (int k = 1; k <= rmax; k++) {
            const float t = zt2[k];
            if (t >= best) break;
            const bool up = k <= z, down = k < l - z;
            if (!up && !down) break;
            if (up) best = fminf(best, (float)gy[i - (long long)k * plane] + t);
            if (down) best = fminf(best, (float)gy[i + (long long)k * plane] + t);
        }
    }
    d2[i] = best;
}

// out: n_fg | n_capped | the maximum of (bits(D2) << 32) | ~index over the foreground (zeroed by the host)
__global__ __launch_bounds__(EDT_TPB) void edt_stats(const float *d2, long long N, float cap, unsigned long long *out)
{
    __shared__ unsigned long long part[3 * (EDT_TPB / 64)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long n_fg = 0, n_cap = 0, key = 0;
    const long long stride = (long long)gridDim.x * EDT_TPB;
    for (long long base = (long long)blockIdx.x * EDT_TPB; base < N; base += stride) { // (wave-uniform: the ballots see whole waves)
        const long long i = base + threadIdx.x;
        const float d = i < N ? d2[i] : 0.f;
        n_fg += (unsigned long long)__popcll(__ballot(d > 0.f));
        n_cap += (unsigned long long)__popcll(__ballot(d > 0.f && d == cap));
        if (d > 0.f) key = max(key, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)~(unsigned)i);
    }
    for (int s = 32; s >= 1; s >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, s, 64));
    if (lane == 0) part[3 * wave] = n_fg, part[3 * wave + 1] = n_cap, part[3 * wave + 2] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < EDT_TPB / 64; i++) n_fg += part[3 * i], n_cap += part[3 * i + 1], key = max(key, part[3 * i + 2]);
        if (n_fg) atomicAdd(&out[0], n_fg);
        if (n_cap) atomicAdd(&out[1], n_cap);
        if (key) atomicMax(&out[2], key);
    }
}

__global__ __launch_bounds__(EDT_TPB) void edt_sample(const float *d2, const float *xyz, long long n, int w, int h, int l, float *at)
{
    const long long i = (long long)blockIdx.x * EDT_TPB + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    at[i] = pnr::finite3(px, py, pz) ? d2[pnr::centre_voxel(w, h, l, px, py, pz)] : -1.f;
}

} // namespace

int pnr_edt_run(pnr_ctx *c, const char *who, const pnr_edt_opts &o, pnr_edt_info *info, float *d2_out, const float *xyz, int64_t n, float *d2_at)
{
    const int64_t N = c->N;
    const int w = (int)c->w, h = (int)c->h, l = (int)c->l;
    const int64_t rows = (int64_t)h * l, words = (w + EDT_WX - 1) / EDT_WX; // (rows * words <= N)
    const int64_t xblocks = (rows + EDT_ROWS - 1) / EDT_ROWS, vblocks = (N + EDT_TPB - 1) / EDT_TPB;
    PNR_REQUIRE(xblocks < (1LL << 31) && vblocks < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    // device buffers of the call: gx, then D2 | the row carries, then gy | zt2 | the byte sum | the statistics | the positions | D2 there
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_a = buf.add<float>((size_t)N);
    const auto d_b = buf.add<unsigned>((size_t)N);
    const auto d_zt = buf.add<float>((size_t)o.rmax + 1);
    const auto d_sum = buf.add<unsigned long long>(1), d_st = buf.add<unsigned long long>(3);
    const auto d_xyz = buf.add<float>((size_t)n * 3), d_at = buf.add<float>((size_t)n);
    int rc = buf.alloc(who);
    if (rc) return rc;
    int t = o.thr;
    if (o.thr < 0 && (rc = pnr_mean_threshold(c, who, "edt_threshold", c->d_img, N, d_sum, &t))) return rc; // the global mean
    const float zd = c->prm.zdist, cap = (float)(o.rmax * o.rmax);
    std::vector<float> zt2((size_t)o.rmax + 1);
    for (int k = 0; k <= o.rmax; k++) zt2[(size_t)k] = (zd * (float)k) * (zd * (float)k);
    pnr::Call call(c, who);
    call.up(d_zt, zt2.data());
    uint16_t *d_gx = (uint16_t *)d_a.get();
    unsigned *d_gy = d_b;
    float *d_d2 = d_a;
    call.timed("edt_x", edt_x, dim3((unsigned)xblocks), dim3(XTPB), XArgs{c->d_img, d_gx, (int *)d_b.get(), (long long)rows, w, (int)words, t, o.rmax});
    call.timed("edt_y", edt_y, dim3((unsigned)vblocks), dim3(EDT_TPB), (const uint16_t *)d_gx, d_gy, w, h, (long long)N);
    call.timed("edt_z", edt_z, dim3((unsigned)vblocks), dim3(EDT_TPB), (const unsigned *)d_gy, d_d2, (const float *)d_zt.get(), (long long)w * h, l, o.rmax, (long long)N);
    unsigned long long st[3] = {0, 0, 0};
    if (info) {
        call.fill(d_st, 0);
        call.timed("edt_stats", edt_stats, dim3(pnr::grid_blocks(vblocks)), dim3(EDT_TPB), (const float *)d_d2, (long long)N, cap, d_st.get());
        call.down(st, d_st);
    }
    if (n > 0) {
        call.up(d_xyz, xyz);
        call.timed("edt_sample", edt_sample, dim3((unsigned)((n + EDT_TPB - 1) / EDT_TPB)), dim3(EDT_TPB), (const float *)d_d2, (const float *)d_xyz.get(), (long long)n, w, h, l,
                   d_at.get());
        call.down(d2_at, d_at);
    }
    if (d2_out) call.down(d2_out, (const float *)d_d2, (size_t)N);
    if ((rc = call.finish())) return rc; // (zt2 ends here)
    if (info) {
        const int64_t n_fg = (int64_t)st[0];
        uint32_t bits = (uint32_t)(st[2] >> 32);
        float d2_max = 0.f;
        std::memcpy(&d2_max, &bits, 4);
        *info = pnr_edt_info{N, n_fg, (int64_t)st[1], n_fg ? (int64_t)(uint32_t)~(uint32_t)st[2] : -1, n_fg ? d2_max : 0.f, t};
    }
    return PNR_OK;
}
