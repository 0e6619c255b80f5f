// threshold.hip -- the device half of the thresholds (include/pnr_hip.h): the 256-bin histogram of the u8 volume behind
// pnr_auto_threshold, and the box sums of the local threshold (pnr_local_threshold[_volume]).  Neither writes the volume.
//
// Histogram (thr_hist).  One read of the N bytes in 16-byte loads, a scalar head up to the first 16-byte boundary and a scalar
// tail, as vol_sum takes an unaligned device pointer; the counting is hist.h's: per-wave private LDS bins, the bin of the first
// voxel in a register, one u64 atomic per bin and work-group.  Bytes moved: N read, 2 KiB written.
//
// Local threshold.  Separable running sums over the box (rx, ry, rz) cut to the volume, three passes per slab of planes:
//   lt_x: a work-group owns rows; a chunk of LT_XCH voxels and its halo (8 samples per lane) is summed to exclusive prefixes in LDS
//     (registers, a wave scan, the four wave totals), and the window sum is the difference of two prefixes: u16 (129 * 255).
//   lt_y: a lane owns one column of a plane (neighbouring lanes = neighbouring x: coalesced) and carries the running sum down it:
//     one sample in, one out per voxel; u32 (129^2 * 255) into the ring.
//   lt_z: a lane owns one z column of the slab; its running sum over the ring's planes is carried from slab to slab in a plane of
//     u32, so that a plane of x-y sums is written once and read twice.  The comparison in signed 64-bit and the output byte are
//     fused into it, with the three counters of the info (one u64 atomic each per work-group).
// The ring holds the s + 2 rz + 1 planes a slab of s planes reads: every plane goes through lt_x and lt_y once, whatever s is.
// Bytes moved per voxel: lt_x 1 read + 2 written, lt_y 4 read (the second touch of a sample comes from the cache at best) + 4
// written, lt_z 8 + 1 read + 1 written: 21 N against the floor of 2 N; the top-hat's six in-place passes move 13 N.
#include "threshold.h"
#include "call.h"
#include "grid.h"
#include "hist.h"

namespace {

using i64 = long long;
using u64 = unsigned long long;

constexpr int TPB = 256;
constexpr int HTPB = pnr::HIST_TPB;
constexpr int MAX_HBLOCKS = 512;
constexpr int MAX_ROW_BLOCKS = 8192;
constexpr int LT_PER = 8;                          // samples of a chunk and its halo per lane
constexpr int LT_LEN = LT_PER * TPB;               // = LT_XCH + 2 * PNR_LOCAL_MAX_R
static_assert(LT_XCH + 2 * PNR_LOCAL_MAX_R == LT_LEN, "a chunk and its halo are eight samples per lane");

__global__ __launch_bounds__(HTPB) void thr_hist(const uint8_t *p, i64 n, i64 head, i64 nvec, u64 *out)
{
    auto visit = [&](auto &&f) {
        const i64 gid = (i64)blockIdx.x * blockDim.x + threadIdx.x, stride = (i64)gridDim.x * blockDim.x;
        const uint4 *v = (const uint4 *)(p + head);
        auto word = [&](unsigned x) { f(x & 255u); f((x >> 8) & 255u); f((x >> 16) & 255u); f(x >> 24); };
        for (i64 g = gid; g < nvec; g += stride) {
            const uint4 q = v[g];
            word(q.x); word(q.y); word(q.z); word(q.w);
        }
        if (gid < head) f(p[gid]);
        const i64 t0 = head + 16 * nvec;
        if (gid < n - t0) f(p[t0 + gid]); // (fewer than 16 left)
    };
    pnr::histogram<256>(visit, [](unsigned v) { return (int)v; }, (int)p[0], out);
}

// slot of prefix i in LDS: lane t writes the prefixes 8 t .. 8 t + 7, a stride of 8 words; one word of padding per 64 spreads them
__device__ __forceinline__ int pslot(int i) { return i + (i >> 6); }

// Sx[row * w + x] = the sum of src[row * w + x'] over |x' - x| <= r, x' in [0, w); rows are owned by work-groups (grid-stride)
__global__ __launch_bounds__(TPB) void lt_x(const uint8_t *__restrict__ src, uint16_t *__restrict__ Sx, int w, i64 nrows, int r)
{
    __shared__ unsigned P[LT_LEN + 1 + (LT_LEN >> 6) + 1]; // P[pslot(i)] = the sum of the chunk's samples [0, i)
    __shared__ unsigned wtot[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, K = 2 * r + 1;
    for (i64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const uint8_t *s = src + row * w;
        uint16_t *d = Sx + row * w;
        for (int c0 = 0; c0 < w; c0 += LT_XCH) {
            const int cw = min(LT_XCH, w - c0), len = cw + 2 * r; // sample k = the voxel c0 - r + k (0 outside the row)
            unsigned v[LT_PER], run = 0;
#pragma unroll
            for (int j = 0; j < LT_PER; j++) {
                const int k = LT_PER * tid + j, pos = c0 - r + k;
                v[j] = k < len && pos >= 0 && pos < w ? s[pos] : 0u;
                run += v[j];
            }
            unsigned incl = run; // inclusive scan of the lanes' totals over the wave
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const unsigned y = (unsigned)__shfl_up((int)incl, dlt, 64);
                if (lane >= dlt) incl += y;
            }
            if (lane == 63) wtot[wv] = incl;
            __syncthreads();
            unsigned base = incl - run;
            for (int k = 0; k < wv; k++) base += wtot[k];
#pragma unroll
            for (int j = 0; j < LT_PER; j++) {
                P[pslot(LT_PER * tid + j)] = base;
                base += v[j];
            }
            if (tid == TPB - 1) P[pslot(LT_LEN)] = base;
            __syncthreads();
            for (int j = tid; j < cw; j += TPB) d[c0 + j] = (uint16_t)(P[pslot(j + K)] - P[pslot(j)]); // (j + K <= len <= LT_LEN)
            __syncthreads();
        }
    }
}

// line u = (plane u / w, column u % w) of the np planes at Sx; their first plane is plane za of the volume.  The running sum over
// |y' - y| <= r goes to plane (za + u / w) % C of the ring.
__global__ __launch_bounds__(TPB) void lt_y(const uint16_t *__restrict__ Sx, unsigned *__restrict__ ring, int w, int h, i64 nlines, i64 za, int C, int r)
{
    const i64 u = (i64)blockIdx.x * TPB + threadIdx.x;
    if (u >= nlines) return;
    const i64 pz = u / w, x = u - pz * w, plane = (i64)w * h;
    const uint16_t *s = Sx + pz * plane + x;
    unsigned *d = ring + ((za + pz) % C) * plane + x;
    unsigned run = 0;
    for (int y = 0; y < min(r, h); y++) run += s[(i64)y * w];
    for (int y = 0; y < h; y++) {
        if (y + r < h) run += s[(i64)(y + r) * w];
        if (y - r - 1 >= 0) run -= s[(i64)(y - r - 1) * w];
        d[(i64)y * w] = run;
    }
}

struct LtArgs {
    const uint8_t *V;
    uint8_t *out;
    const unsigned *ring;
    unsigned *carry; // per column: the z window sum of plane z0 - 1
    u64 *st;         // n_kept, sum_in, sum_out
    int w, h, l, C;
    int z0, z1;      // the slab's planes
    int rx, ry, rz;
    int offset, scale, floor, binary;
};

__global__ __launch_bounds__(TPB) void lt_z(LtArgs a)
{
    __shared__ u64 part[3][TPB / 64];
    const i64 plane = (i64)a.w * a.h, i = (i64)blockIdx.x * TPB + threadIdx.x;
    u64 kept = 0, sin = 0, sout = 0;
    if (i < plane) {
        const int y = (int)(i / a.w), x = (int)(i - (i64)y * a.w);
        const i64 nxy = (i64)(min(x + a.rx, a.w - 1) - max(x - a.rx, 0) + 1) * (min(y + a.ry, a.h - 1) - max(y - a.ry, 0) + 1);
        unsigned run;
        if (a.z0 == 0) { // the window of plane -1: the planes [0, rz) of the volume
            run = 0;
            for (int z = 0; z < min(a.rz, a.l); z++) run += a.ring[(i64)(z % a.C) * plane + i];
        } else {
            run = a.carry[i];
        }
        for (int z = a.z0; z < a.z1; z++) {
            if (z + a.rz < a.l) run += a.ring[(i64)((z + a.rz) % a.C) * plane + i];
            if (z - a.rz - 1 >= 0) run -= a.ring[(i64)((z - a.rz - 1) % a.C) * plane + i];
            const i64 n = nxy * (min(z + a.rz, a.l - 1) - max(z - a.rz, 0) + 1), v = a.V[(i64)z * plane + i];
            const bool keep = v >= a.floor && 256 * n * v >= (i64)a.scale * (i64)run + 256 * (i64)a.offset * n;
            const unsigned o = keep ? (a.binary ? 255u : (unsigned)v) : 0u;
            a.out[(i64)z * plane + i] = (uint8_t)o;
            kept += keep, sin += (u64)v, sout += o;
        }
        a.carry[i] = run;
    }
    u64 red[3] = {kept, sin, sout};
    for (int k = 0; k < 3; k++)
        for (int d = 32; d >= 1; d >>= 1) red[k] += (u64)__shfl_xor((i64)red[k], d, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) part[k][threadIdx.x >> 6] = red[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 t = 0;
        for (int k = 0; k < TPB / 64; k++) t += part[threadIdx.x][k];
        if (t) atomicAdd(&a.st[threadIdx.x], t);
    }
}

} // namespace

int pnr_hist_run(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, uint64_t *hist)
{
    const i64 head = std::min<i64>(N, (i64)((16 - ((uintptr_t)V & 15)) & 15)), nvec = (N - head) >> 4;
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_hist = buf.add<u64>(256);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.fill(d_hist, 0);
    const i64 work = std::max<i64>(nvec, 16); // threads' worth of work: the vectors, or the head and the tail
    call.timed(group, thr_hist, dim3(pnr::grid_blocks((work + HTPB - 1) / HTPB, MAX_HBLOCKS)), dim3(HTPB), V, (i64)N, head, nvec, d_hist.get());
    call.down(hist, d_hist);
    return call.finish();
}

int pnr_local_run(pnr_ctx *c, const char *who, const pnr_local_vol &vol, const pnr_local_opts &o, pnr_local_info *info, uint8_t *out, pnr::DevBuf<uint8_t> *keep)
{
    const int w = (int)vol.w, h = (int)vol.h, l = (int)vol.l;
    const i64 plane = (i64)w * h, N = plane * l;
    const uint8_t *const V = vol.V;
    const int rz = l == 1 ? 0 : (int)((float)o.r / c->prm.zdist); // one IEEE division
    const i64 slab_vox = c->opt.lt_slab_vox > 0 ? c->opt.lt_slab_vox : LT_SLAB_VOX;
    const int slab = (int)std::max<i64>(1, std::min<i64>(l, slab_vox / plane));
    const int C = (int)std::min<i64>(l, (i64)slab + 2 * (i64)rz + 1), xplanes = (int)std::min<i64>(l, (i64)slab + rz);
    const i64 zblocks = (plane + TPB - 1) / TPB, yblocks = ((i64)w * xplanes + TPB - 1) / TPB;
    PNR_REQUIRE(zblocks < (1LL << 31) && yblocks < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    pnr::DevBuf<uint8_t> result; // (freed when the call returns, or handed to the caller)
    int rc = pnr::dev_alloc(result, (size_t)N, who, "for the thresholded volume");
    if (rc) return rc;
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_sx = buf.add<uint16_t>((size_t)(plane * xplanes));
    const auto d_ring = buf.add<unsigned>((size_t)(plane * C));
    const auto d_carry = buf.add<unsigned>((size_t)plane);
    const auto d_st = buf.add<u64>(3);
    if ((rc = buf.alloc(who))) return rc;
    pnr::Call call(c, who);
    call.fill(d_st, 0);
    int launches = 0;
    c->tic();
    i64 done = 0; // planes [0, done) of the volume have their x-y sums in the ring
    for (int z0 = 0; z0 < l; z0 += slab) {
        const int z1 = std::min(l, z0 + slab);
        const i64 upto = std::min<i64>(l, (i64)z1 + rz), np = upto - done; // (np <= slab + rz: the first slab's)
        if (np > 0) {
            const i64 nrows = np * h, nlines = np * w;
            call.launch(lt_x, dim3((unsigned)std::min<i64>(nrows, MAX_ROW_BLOCKS)), dim3(TPB), V + done * plane, d_sx.get(), w, nrows, o.r);
            call.launch(lt_y, dim3((unsigned)((nlines + TPB - 1) / TPB)), dim3(TPB), (const uint16_t *)d_sx.get(), d_ring.get(), w, h, nlines, done, C, o.r);
            launches += 2;
            done = upto;
        }
        call.launch(lt_z, dim3((unsigned)zblocks), dim3(TPB),
                    LtArgs{V, result.get(), d_ring.get(), d_carry.get(), d_st.get(), w, h, l, C, z0, z1, o.r, o.r, rz, o.offset, o.scale_256, o.floor, o.binary});
        launches++;
    }
    c->toc("local_threshold", launches);
    u64 st[3] = {0, 0, 0};
    call.down(st, d_st);
    if (out) call.down(out, (const uint8_t *)result.get(), (size_t)N);
    if ((rc = call.finish())) return rc;
    if (info) *info = pnr_local_info{N, (int64_t)st[0], st[1], st[2], o.r, o.r, rz, 0};
    if (keep) *keep = std::move(result);
    return PNR_OK;
}
