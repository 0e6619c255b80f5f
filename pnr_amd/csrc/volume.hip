// volume.hip -- a u16 channel windowed to the u8 volume the pipeline traces (pnr_set_volume_u16).  The rule (include/pnr_hip.h):
//   window [lo, hi]: given, or the samples of ranks k_lo = floor(N * sat_lo_ppm / 1e6) and k_hi = N - 1 - floor(N * sat_hi_ppm / 1e6)
//   of the sorted channel (default: [min, max]);
//   hi > lo: out = (510 a + d) div 2d with a = clamp(v, lo, hi) - lo, d = hi - lo (255 a / d rounded half up); hi == lo: 255 above lo, else 0.
//
// [min, max]: one read pass, a wave / work-group reduction and one integer atomic max per work-group for each end (the minimum is
// kept as 65535 - min, so that both words start at 0).  Any other rank pair: an exact two-pass radix select -- a 256-bin histogram
// of the high bytes (a private LDS copy per wave, one u64 atomic per bin and work-group: 2^32 voxels overflow u32 counters), a
// one-work-group select of the coarse bins of k_lo / k_hi and the ranks left inside them, 2 x 256 fine bins of the low bytes of the
// voxels in those two bins, a second select.  The window stays on the device until the map kernel has read it; the host reads its
// two words once at the end.
//
// A histogram wave counts the voxels of one bin (the bin of the stack's first voxel: the background of a dark stack) in a register
// instead of LDS: a wave whose 64 lanes all add to the same LDS word is serialised 64-fold.
//
// Below it: the exact byte sum of a u8 volume (vol_sum: one grid-stride u64 reduction, one atomic per work-group) and the threshold
// rule "thr = -1" of the radii, the coverage and the components that rests on it (pnr_mean_threshold).
#include "volume.h"
#include "call.h"
#include "grid.h"
#include "hist.h"

namespace {

constexpr int TPB = 256;            // threads of the min / max and the map kernels
constexpr int HTPB = pnr::HIST_TPB;  // threads of a histogram work-group (hist.h)
using pnr::MAX_BLOCKS;
constexpr int MAX_HBLOCKS = 512;

// device state of one call: the window (win[0] = 65535 - lo, win[1] = hi), the selected bins and the ranks left in them, the bins
struct VolState {
    unsigned win[2];
    unsigned pad[2];
    long long sel[4];                 // coarse bin of k_lo, of k_hi; rank of k_lo in its bin, of k_hi in its bin
    unsigned long long coarse[256];
    unsigned long long fine[512];     // [0, 256): low bytes of the voxels in k_lo's coarse bin; [256, 512): in k_hi's (if another bin)
};

// the channel's samples: nchan == 1 splits [0, n) into a scalar head up to the first 16-byte boundary, nvec 8-sample vectors and
// a scalar tail
struct Src {
    const uint16_t *p;
    long long n, head, nvec;
    int nchan, ch;
};

// f(v) for every voxel this thread owns (grid-stride)
template <class F>
__device__ __forceinline__ void visit(const Src &s, F &&f)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (s.nchan == 1) {
        const uint4 *v = (const uint4 *)(s.p + s.head);
        for (long long g = gid; g < s.nvec; g += stride) {
            const uint4 q = v[g];
            f(q.x & 0xffffu); f(q.x >> 16); f(q.y & 0xffffu); f(q.y >> 16);
            f(q.z & 0xffffu); f(q.z >> 16); f(q.w & 0xffffu); f(q.w >> 16);
        }
        if (gid < s.head) f(s.p[gid]);
        const long long t0 = s.head + 8 * s.nvec;
        if (gid < s.n - t0) f(s.p[t0 + gid]);
    } else {
        const long long nc = s.nchan;
        long long i = gid;
        for (; i + 3 * stride < s.n; i += 4 * stride) { // four loads in flight per thread
            const unsigned a = s.p[i * nc + s.ch], b = s.p[(i + stride) * nc + s.ch];
            const unsigned c = s.p[(i + 2 * stride) * nc + s.ch], d = s.p[(i + 3 * stride) * nc + s.ch];
            f(a); f(b); f(c); f(d);
        }
        for (; i < s.n; i += stride) f(s.p[i * nc + s.ch]);
    }
}

__device__ __forceinline__ unsigned wave_max(unsigned x)
{
    for (int d = 32; d >= 1; d >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, d, 64));
    return x;
}

__global__ __launch_bounds__(TPB) void vol_minmax(Src s, VolState *st)
{
    __shared__ unsigned part[2][TPB / 64];
    unsigned inv = 0, mx = 0; // max of 65535 - v, max of v
    visit(s, [&](unsigned v) { inv = max(inv, 65535u - v); mx = max(mx, v); });
    inv = wave_max(inv);
    mx = wave_max(mx);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { part[0][w] = inv; part[1][w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TPB / 64; k++) { inv = max(inv, part[0][k]); mx = max(mx, part[1][k]); }
        atomicMax(&st->win[0], inv);
        atomicMax(&st->win[1], mx);
    }
}

// the histogram of hist.h over the channel's samples
template <int NB, class K>
__device__ __forceinline__ void histogram(const Src &s, K &&key, int hot, unsigned long long *out)
{
    pnr::histogram<NB>([&](auto &&f) { visit(s, f); }, key, hot, out);
}

__global__ __launch_bounds__(HTPB) void vol_hist_coarse(Src s, VolState *st)
{
    const int hot = (int)(s.p[s.ch] >> 8);
    histogram<256>(s, [](unsigned v) { return (int)(v >> 8); }, hot, st->coarse);
}

__global__ __launch_bounds__(HTPB) void vol_hist_fine(Src s, VolState *st)
{
    const unsigned blo = (unsigned)st->sel[0], bhi = (unsigned)st->sel[1];
    auto key = [blo, bhi](unsigned v) {
        const unsigned hb = v >> 8;
        return hb == blo ? (int)(v & 255u) : (hb == bhi ? 256 + (int)(v & 255u) : -1);
    };
    histogram<512>(s, key, key(s.p[s.ch]), st->fine);
}

// one work-group of 256: the bin of 256 that holds rank k of the counts, and the rank left inside it
__device__ void find_rank(const unsigned long long *bins, long long k, unsigned long long *scan, long long *bin_out, long long *rank_out)
{
    const int t = threadIdx.x;
    const unsigned long long c = bins[t];
    scan[t] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned long long y = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += y;
        __syncthreads();
    }
    const unsigned long long incl = scan[t], excl = incl - c, kk = (unsigned long long)k;
    if (excl <= kk && kk < incl) {
        *bin_out = t;
        *rank_out = (long long)(kk - excl);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void vol_select_coarse(VolState *st, long long k_lo, long long k_hi)
{
    __shared__ unsigned long long scan[256];
    find_rank(st->coarse, k_lo, scan, &st->sel[0], &st->sel[2]);
    find_rank(st->coarse, k_hi, scan, &st->sel[1], &st->sel[3]);
}

__global__ __launch_bounds__(256) void vol_select_fine(VolState *st)
{
    __shared__ unsigned long long scan[256];
    __shared__ long long res[4];
    const long long blo = st->sel[0], bhi = st->sel[1];
    find_rank(st->fine, st->sel[2], scan, &res[0], &res[2]);
    find_rank(st->fine + (bhi == blo ? 0 : 256), st->sel[3], scan, &res[1], &res[3]);
    if (threadIdx.x == 0) {
        st->win[0] = 65535u - (unsigned)(blo * 256 + res[0]);
        st->win[1] = (unsigned)(bhi * 256 + res[1]);
    }
}

// out[i] = the rule for voxel i; VEC: nchan == 1 and a 16-byte aligned source (8 samples per load); groups of 8 voxels, 8-byte stores
template <bool VEC>
__global__ __launch_bounds__(TPB) void vol_map(Src s, const VolState *st, unsigned flo, unsigned fhi, uint8_t *out)
{
    const unsigned lo = st ? 65535u - st->win[0] : flo, hi = st ? st->win[1] : fhi;
    const int d = (int)hi - (int)lo, den = 2 * d;
    const float rcp = d > 0 ? 1.f / (float)den : 0.f;
    auto m = [&](unsigned v) -> unsigned {
        if (d == 0) return v > lo ? 255u : 0u;
        const int a = (int)min(max(v, lo), hi) - (int)lo;
        const int num = 510 * a + d;                     // < 2^25
        int q = (int)((float)num * rcp);                 // within 1 of num / den
        const int r = num - q * den;
        q += (r >= den) - (r < 0);
        return (unsigned)q;
    };
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    const long long ng = s.n >> 3, nc = s.nchan;
    for (long long g = gid; g < ng; g += stride) {
        unsigned x[8];
        if (VEC) {
            const uint4 q = ((const uint4 *)s.p)[g];
            x[0] = q.x & 0xffffu; x[1] = q.x >> 16; x[2] = q.y & 0xffffu; x[3] = q.y >> 16;
            x[4] = q.z & 0xffffu; x[5] = q.z >> 16; x[6] = q.w & 0xffffu; x[7] = q.w >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = s.p[(8 * g + j) * nc + s.ch];
        }
        uint2 o;
        o.x = m(x[0]) | m(x[1]) << 8 | m(x[2]) << 16 | m(x[3]) << 24;
        o.y = m(x[4]) | m(x[5]) << 8 | m(x[6]) << 16 | m(x[7]) << 24;
        ((uint2 *)out)[g] = o;
    }
    const long long t0 = 8 * ng;
    if (gid < s.n - t0) out[t0 + gid] = (uint8_t)m(s.p[(t0 + gid) * nc + s.ch]);
}

// sum of the bytes p[0, n): scalar head up to the first 16-byte boundary, 16-byte vectors, scalar tail
__global__ __launch_bounds__(TPB) void vol_sum(const uint8_t *p, long long n, long long head, long long nvec, unsigned long long *out)
{
    __shared__ unsigned long long part[TPB / 64];
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned long long s = 0;
    const uint4 *v = (const uint4 *)(p + head);
    auto bytes = [](unsigned x) { const unsigned y = (x & 0x00ff00ffu) + ((x >> 8) & 0x00ff00ffu); return (y & 0xffffu) + (y >> 16); };
    for (long long g = gid; g < nvec; g += stride) {
        const uint4 q = v[g];
        s += bytes(q.x) + bytes(q.y) + bytes(q.z) + bytes(q.w);
    }
    if (gid < head) s += p[gid];
    const long long t0 = head + 16 * nvec;
    if (gid < n - t0) s += p[t0 + gid]; // (fewer than 16 left)
    for (int d = 32; d >= 1; d >>= 1) s += (unsigned long long)__shfl_xor((long long)s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TPB / 64; k++) s += part[k];
        if (s) atomicAdd(out, s);
    }
}

unsigned blocks_for(long long work, int tpb, int cap) { return pnr::grid_blocks((work + tpb - 1) / tpb, cap); }

} // namespace

int pnr_volume_u16_run(pnr_ctx *c, const uint16_t *d_src, int nchan, int channel, const pnr_window &win, int32_t *lo_out, int32_t *hi_out)
{
    static const char *who = "pnr_set_volume_u16";
    const long long N = c->N;
    int rc = pnr::dev_alloc(c->d_img_owned, (size_t)N, who, "for the 8-bit volume");
    if (rc) return rc;
    const bool fixed = win.lo >= 0, minmax = !fixed && win.sat_lo_ppm == 0 && win.sat_hi_ppm == 0;
    pnr::DevBuf<VolState> b_st; // (freed when the call returns: every path below has drained the stream or failed to)
    if (!fixed && (rc = pnr::dev_alloc(b_st, 1, who, "of window state"))) return rc;
    VolState *d_st = b_st.get();
    pnr::Call call(c, who);
    if (d_st) call.fill(d_st, 0, 1);
    Src s{d_src, N, 0, 0, nchan, channel};
    const uintptr_t addr = (uintptr_t)d_src;
    if (nchan == 1) {
        s.head = std::min<long long>(N, (long long)(((16 - (addr & 15)) & 15) >> 1));
        s.nvec = (N - s.head) >> 3;
    }
    const long long work = nchan == 1 ? std::max(s.nvec, s.head + 8) : N; // threads' worth of work of the read passes
    int launches = 1;
    c->tic();
    if (minmax) {
        call.launch(vol_minmax, dim3(blocks_for(work, TPB, MAX_BLOCKS)), dim3(TPB), s, d_st);
        launches++;
    } else if (!fixed) {
        // k_lo <= k_hi < N: sat_lo_ppm + sat_hi_ppm < 1e6 (checked by the caller); N * ppm < 2^63 for any stack a device can hold
        const long long k_lo = N * (long long)win.sat_lo_ppm / 1000000, k_hi = N - 1 - N * (long long)win.sat_hi_ppm / 1000000;
        const unsigned hb = blocks_for(work, HTPB, MAX_HBLOCKS);
        call.launch(vol_hist_coarse, dim3(hb), dim3(HTPB), s, d_st);
        call.launch(vol_select_coarse, dim3(1), dim3(256), d_st, k_lo, k_hi);
        call.launch(vol_hist_fine, dim3(hb), dim3(HTPB), s, d_st);
        call.launch(vol_select_fine, dim3(1), dim3(256), d_st);
        launches += 4;
    }
    call.launch(nchan == 1 && (addr & 15) == 0 ? vol_map<true> : vol_map<false>, dim3(blocks_for(N >> 3, TPB, MAX_BLOCKS)), dim3(TPB), s, d_st, (unsigned)win.lo,
                (unsigned)win.hi, c->d_img_owned.get());
    c->toc("volume", launches);
    unsigned w2[2] = {65535u - (unsigned)win.lo, (unsigned)win.hi};
    if (d_st) call.down(w2, d_st->win, 2);
    if ((rc = call.finish())) return rc;
    if (lo_out) *lo_out = (int32_t)(65535u - w2[0]);
    if (hi_out) *hi_out = (int32_t)w2[1];
    return PNR_OK;
}

int pnr_byte_sum_run(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, unsigned long long *d_sum, unsigned long long *sum)
{
    const long long head = std::min<long long>(N, (long long)((16 - ((uintptr_t)V & 15)) & 15)), nvec = (N - head) >> 4;
    pnr::Call call(c, who);
    call.fill(d_sum, 0, 1);
    call.timed(group, vol_sum, dim3(blocks_for(std::max<long long>(nvec, 16), TPB, MAX_BLOCKS)), dim3(TPB), V, (long long)N, head, nvec, d_sum);
    call.down(sum, d_sum, 1);
    return call.finish();
}

int pnr_mean_threshold(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, unsigned long long *d_word, int *t)
{
    unsigned long long sum = 0;
    const int rc = pnr_byte_sum_run(c, who, group, V, N, d_word, &sum);
    if (!rc) *t = (int)std::max<unsigned long long>(1, sum / (unsigned long long)N);
    return rc;
}
