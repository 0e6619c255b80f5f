// filter.hip -- pre-filters of the traced u8 volume (pnr_filter_volume).  The rule (include/pnr_hip.h):
//   median 2 / 3: the sample of rank 4 of the 3 x 3 window in the slice / of rank 13 of the 3 x 3 x 3 window, coordinates clamped to
//     the edge;
//   top-hat R: e = min of V over the box (R, R, (int)((float)R / zdist)) cut to the volume, o = max of e over the same box,
//     out = V - o; median first.
//
// Median.  A work-group owns MED_TX x MED_TY voxels in x-y and marches down MED_ZC planes.  Every plane of the tile (with a halo of
// one voxel, coordinates clamped) goes through LDS once; a lane owns four voxels of a row (one 32-bit word) and keeps the three
// rows around it of the three live planes in registers, so that a plane is fetched from LDS once for the three outputs along z it
// belongs to.  The bytes are unpacked to pairs of 16-bit halves (voxels 0, 2 and voxels 1, 3 of the word; the left and right
// neighbours are the same pairs shifted by one half), and the selection runs on v_pk_min_u16 / v_pk_max_u16: one instruction
// compares two voxels.  The selection is the forgetful one: of n / 2 + 2 samples the minimum and the maximum cannot be the median
// of n, so they are dropped and the next sample comes in -- 15, 14, ... 3 live samples for 27 (6, 5, 4, 3 for 9), about 150
// compare-exchanges per pair of voxels, no sample is ever sorted that cannot matter.  The unpacked rows are shared by the two
// pairs of a word and by three steps of the march; partial sorts are not shared between neighbouring windows.
//
// Top-hat.  Six separable passes -- running minimum along x, y, z, running maximum along x, y, z (the z passes only where the box
// has a z extent) -- with the subtraction fused into the last one.  Every pass can run in place, so the whole chain needs one
// working buffer: the first pass reads the input and writes the buffer, the others work inside it.
//   x: a work-group owns whole rows and takes them in chunks of TH_CH voxels: the chunk and the box's halo in LDS (voxels outside
//     the row are the identity), the window minima of lengths 1, 2, 4, ... P <= 2R + 1 by doubling, the result from two overlapping
//     windows of length P.  The raw tail of a chunk is carried to the next one in LDS, which is what makes the pass safe in place.
//   y, z: a lane owns one line and streams down it (neighbouring lanes = neighbouring x: coalesced), van Herk / Gil-Werman: the
//     line is cut into segments of 2r + 1; out[j - r] = op(prefix of the segment of j up to j, suffix of the segment before it
//     from j - 2r).  The suffixes of one segment are a private column of 2r + 1 bytes in LDS, turned from raw samples into suffixes
//     once per segment: three LDS accesses and two min / max per voxel whatever r is.  A line is read r samples ahead of where it
//     is written, so this pass works in place too.
#include "filter.h"
#include "call.h"

namespace {

using i64 = long long;
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

constexpr int TPB = 256;
constexpr int MED_TXW = MED_TX / 4;          // lanes (words) of a tile row
constexpr int MED_LW = MED_TXW + 2;          // ... plus one halo word on either side (one byte of each is used)
constexpr int MED_LR = MED_TY + 2;
constexpr int MED_WORDS = MED_LW * MED_LR;
static_assert(MED_TXW * MED_TY == TPB, "one lane per word of the tile");
static_assert(MED_WORDS <= 2 * TPB, "a plane of the tile is staged in two words per lane");
constexpr int TH_LEN = TH_CH + 2 * PNR_TOPHAT_MAX_R;
constexpr int TH_KMAX = 2 * PNR_TOPHAT_MAX_R + 1;
constexpr int MAX_ROW_BLOCKS = 8192;

__device__ __forceinline__ us2 as_us2(unsigned v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ unsigned as_u32(us2 v) { return __builtin_bit_cast(unsigned, v); }

__device__ __forceinline__ void cex(us2 &a, us2 &b)
{
    const us2 lo = __builtin_elementwise_min(a, b);
    b = __builtin_elementwise_max(a, b);
    a = lo;
}

// the minimum of a[0, N) to a[0], the maximum to a[N - 1]
template <int N>
__device__ __forceinline__ void minmax(us2 *a)
{
    constexpr int H = (N + 1) / 2; // the lower partners (and the middle one of an odd N), the upper partners (and the middle one)
#pragma unroll
    for (int i = 0; i < N / 2; i++) cex(a[i], a[N - 1 - i]);
#pragma unroll
    for (int i = 1; i < H; i++) cex(a[0], a[i]);
#pragma unroll
    for (int i = N - H; i < N - 1; i++) cex(a[i], a[N - 1]);
}

// N live samples in a[0, N), in[NEXT] the next one of NT: neither the minimum nor the maximum of the live ones is the median of all
template <int N, int NEXT, int NT>
struct Forget {
    static __device__ __forceinline__ us2 run(us2 *a, const us2 *in)
    {
        minmax<N>(a);
        if constexpr (N == 3) {
            static_assert(NEXT == NT, "every sample has come in");
            return a[1];
        } else {
            a[0] = in[NEXT];
            return Forget<N - 1, NEXT + 1, NT>::run(a, in);
        }
    }
};

template <int NT>
__device__ __forceinline__ us2 median_of(const us2 *in)
{
    constexpr int N0 = NT / 2 + 2;
    us2 a[N0];
#pragma unroll
    for (int i = 0; i < N0; i++) a[i] = in[i];
    return Forget<N0, N0, NT>::run(a, in);
}

// a row of the lane's word and its neighbours as pairs of halves: voxels (-1, 1), (0, 2), (1, 3), (2, 4)
struct Row {
    us2 lm, e, o, rp;
};

// word `idx` of the staged plane `p` (a plane of the volume) of the tile at (x0, y0): coordinates clamped to the edge
__device__ __forceinline__ unsigned med_load(const uint8_t *p, int idx, int x0, int y0, int w, int h)
{
    const int row = idx / MED_LW, wx = idx - row * MED_LW;
    const int gy = min(max(y0 + row - 1, 0), h - 1);
    const uint8_t *rp = p + (i64)gy * w;
    if (wx == 0) return (unsigned)rp[max(x0 - 1, 0)] << 24;
    if (wx == MED_LW - 1) return rp[min(x0 + MED_TX, w - 1)];
    const int xs = x0 + 4 * (wx - 1);
    if (xs + 3 < w && (((uintptr_t)(rp + xs)) & 3) == 0) return *(const unsigned *)(rp + xs);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) v |= (unsigned)rp[min(xs + j, w - 1)] << (8 * j);
    return v;
}

// M3: 3 x 3 x 3 (27 samples), else 3 x 3 in the slice (9 samples).  Grid: tiles_x * tiles_y * ceil(l / MED_ZC) work-groups.
template <bool M3>
__global__ __launch_bounds__(TPB) void median_k(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int w, int h, int l, int tiles_x, int tiles_y)
{
    __shared__ unsigned tile[2][MED_WORDS];
    i64 b = blockIdx.x;
    const int bx = (int)(b % tiles_x);
    b /= tiles_x;
    const int by = (int)(b % tiles_y), bz = (int)(b / tiles_y);
    const int x0 = bx * MED_TX, y0 = by * MED_TY, z0 = bz * MED_ZC, z1 = min(z0 + MED_ZC, l);
    const int tid = threadIdx.x, tx = tid & (MED_TXW - 1), ty = tid / MED_TXW;
    const i64 plane = (i64)w * h;
    unsigned st[2];
    int buf = 0;

    auto fetch = [&](int z) { // the lane's share of plane z (clamped) into registers
        const uint8_t *p = src + (i64)min(max(z, 0), l - 1) * plane;
        st[0] = med_load(p, tid, x0, y0, w, h);
        st[1] = tid + TPB < MED_WORDS ? med_load(p, tid + TPB, x0, y0, w, h) : 0u;
    };
    auto stage = [&](Row (&r)[3]) { // ... through LDS into the three rows around the lane's word
        tile[buf][tid] = st[0];
        if (tid + TPB < MED_WORDS) tile[buf][tid + TPB] = st[1];
        __syncthreads(); // (the buffer written next was last read before the barrier of the step before this one)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned *q = &tile[buf][(ty + k) * MED_LW + tx];
            const unsigned L = q[0], C = q[1], R = q[2];
            const unsigned e = C & 0x00ff00ffu, o = (C >> 8) & 0x00ff00ffu;
            r[k].e = as_us2(e);
            r[k].o = as_us2(o);
            r[k].lm = as_us2((L >> 24) | (o << 16));
            r[k].rp = as_us2((e >> 16) | ((R & 0xffu) << 16));
        }
        buf ^= 1;
    };
    auto store = [&](int z, us2 ma, us2 mb) {
        const int x = x0 + 4 * tx, y = y0 + ty;
        if (y >= h || x >= w) return;
        const unsigned word = as_u32(ma) | (as_u32(mb) << 8);
        uint8_t *o = dst + (i64)z * plane + (i64)y * w + x;
        if (x + 3 < w && (((uintptr_t)o) & 3) == 0) {
            *(unsigned *)o = word;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x + j < w) o[j] = (uint8_t)(word >> (8 * j));
        }
    };

    if (M3) {
        Row P[3][3];
        fetch(z0 - 1);
        stage(P[0]);
        fetch(z0);
        stage(P[1]);
        fetch(z0 + 1);
        for (int z = z0; z < z1; z++) {
            stage(P[2]);
            if (z + 1 < z1) fetch(z + 2); // in flight during the selection
            us2 in[27];
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    in[9 * p + 3 * k] = P[p][k].lm;
                    in[9 * p + 3 * k + 1] = P[p][k].e;
                    in[9 * p + 3 * k + 2] = P[p][k].o;
                }
            const us2 ma = median_of<27>(in);
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int k = 0; k < 3; k++) in[9 * p + 3 * k] = P[p][k].rp; // (e, o, rp): the windows of voxels 1 and 3
            const us2 mb = median_of<27>(in);
            store(z, ma, mb);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                P[0][k] = P[1][k];
                P[1][k] = P[2][k];
            }
        }
    } else {
        Row P[3];
        fetch(z0);
        for (int z = z0; z < z1; z++) {
            stage(P);
            if (z + 1 < z1) fetch(z + 1);
            us2 in[9];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                in[3 * k] = P[k].lm;
                in[3 * k + 1] = P[k].e;
                in[3 * k + 2] = P[k].o;
            }
            const us2 ma = median_of<9>(in);
#pragma unroll
            for (int k = 0; k < 3; k++) in[3 * k] = P[k].rp;
            const us2 mb = median_of<9>(in);
            store(z, ma, mb);
        }
    }
}

template <bool MAX>
__device__ __forceinline__ unsigned op(unsigned a, unsigned b)
{
    return MAX ? max(a, b) : min(a, b);
}

// running min / max of half-width r along x; rows are owned by work-groups (grid-stride), src == dst is allowed
template <bool MAX>
__global__ __launch_bounds__(TPB) void th_x(const uint8_t *src, uint8_t *dst, int w, i64 nrows, int r)
{
    __shared__ uint8_t sa[TH_LEN], sb[TH_LEN], carry[2 * PNR_TOPHAT_MAX_R];
    constexpr unsigned ID = MAX ? 0u : 255u;
    const int K = 2 * r + 1, tid = threadIdx.x;
    for (i64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const uint8_t *s = src + row * w;
        uint8_t *d = dst + row * w;
        for (int c0 = 0; c0 < w; c0 += TH_CH) {
            const int cw = min(TH_CH, w - c0), len = cw + 2 * r; // sa[k] = the raw voxel c0 - r + k
            for (int k = tid; k < len; k += TPB) {
                unsigned v;
                if (c0 > 0 && k < 2 * r) {
                    v = carry[k]; // (may have been overwritten in the row already)
                } else {
                    const int pos = c0 - r + k;
                    v = pos >= 0 && pos < w ? s[pos] : ID;
                }
                sa[k] = (uint8_t)v;
            }
            __syncthreads();
            if (cw == TH_CH)
                for (int k = tid; k < 2 * r; k += TPB) carry[k] = sa[TH_CH + k];
            uint8_t *cur = sa, *nxt = sb;
            int p = 1;
            while (2 * p <= K) { // windows of length 2p from two of length p
                for (int k = tid; k < len; k += TPB) nxt[k] = (uint8_t)op<MAX>(cur[k], k + p < len ? cur[k + p] : ID);
                __syncthreads();
                uint8_t *t = cur;
                cur = nxt;
                nxt = t;
                p *= 2;
            }
            for (int j = tid; j < cw; j += TPB) d[c0 + j] = (uint8_t)op<MAX>(cur[j], cur[j + K - p]);
            __syncthreads();
        }
    }
}

// running min / max of half-width r along a strided axis of n samples: line u starts at (u / inner) * outer + u % inner, its
// stride is inner.  SUB: dst = M - result.  src == dst is allowed.  One lane per line, no barrier.
template <bool MAX, bool SUB>
__global__ __launch_bounds__(TPB) void th_col(const uint8_t *src, uint8_t *dst, const uint8_t *M, i64 nlines, i64 inner, i64 outer, int n, int r)
{
    __shared__ uint8_t T[TH_KMAX * TPB];
    constexpr unsigned ID = MAX ? 0u : 255u;
    constexpr int U = 8;
    const i64 u = (i64)blockIdx.x * TPB + threadIdx.x;
    if (u >= nlines) return;
    const i64 base = (u / inner) * outer + u % inner, stride = inner;
    const int K = 2 * r + 1;
    uint8_t *t = T + threadIdx.x; // slot o at t[o * TPB]: the suffix from offset o of the segment before the current one
    for (int o = 0; o < K; o++) t[o * TPB] = (uint8_t)ID;
    unsigned pre = ID;
    int pos = 0; // offset of j in its segment
    const int total = n + r;
    for (int j0 = 0; j0 < total; j0 += U) {
        unsigned v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = j0 + k < n ? src[base + (i64)(j0 + k) * stride] : ID;
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int j = j0 + k;
            if (j < total) {
                pre = pos == 0 ? v[k] : op<MAX>(pre, v[k]);
                const unsigned tail = pos + 1 < K ? t[(pos + 1) * TPB] : ID;
                const unsigned res = op<MAX>(pre, tail);
                t[pos * TPB] = (uint8_t)v[k];
                if (j >= r) {
                    const i64 i = base + (i64)(j - r) * stride;
                    dst[i] = (uint8_t)(SUB ? M[i] - res : res);
                }
                if (++pos == K) { // the raw samples of this segment become its suffixes
                    unsigned acc = t[(K - 1) * TPB];
                    for (int o = K - 2; o >= 0; o--) {
                        acc = op<MAX>(acc, t[o * TPB]);
                        t[o * TPB] = (uint8_t)acc;
                    }
                    pos = 0;
                }
            }
        }
    }
}

template <bool MAX>
int launch_x(pnr::Call &call, const uint8_t *src, uint8_t *dst, int w, i64 nrows, int r)
{
    call.launch(th_x<MAX>, dim3((unsigned)std::min<i64>(nrows, MAX_ROW_BLOCKS)), dim3(TPB), src, dst, w, nrows, r);
    return 1;
}

template <bool MAX>
int launch_col(pnr::Call &call, const uint8_t *src, uint8_t *dst, const uint8_t *M, i64 nlines, i64 inner, i64 outer, int n, int r)
{
    call.launch(M ? th_col<MAX, true> : th_col<MAX, false>, dim3((unsigned)((nlines + TPB - 1) / TPB)), dim3(TPB), src, dst, M, nlines, inner, outer, n, r);
    return 1;
}

} // namespace

int pnr_filter_run(pnr_ctx *c, const pnr_filter_opts &o, pnr::DevBuf<uint8_t> &result)
{
    static const char *who = "pnr_filter_volume";
    const int w = (int)c->w, h = (int)c->h, l = (int)c->l;
    const i64 N = c->N, plane = (i64)w * h;
    const int tiles_x = (w + MED_TX - 1) / MED_TX, tiles_y = (h + MED_TY - 1) / MED_TY;
    const i64 med_blocks = (i64)tiles_x * tiles_y * ((l + MED_ZC - 1) / MED_ZC);
    const i64 col_blocks = (std::max((i64)w * l, plane) + TPB - 1) / TPB;
    PNR_REQUIRE(med_blocks < (1LL << 31) && col_blocks < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    const bool both = o.median && o.tophat_r;
    pnr::DevBuf<uint8_t> bA, bB; // A: the first stage's output; B: the top-hat's buffer behind a median
    int rc = pnr::dev_alloc(bA, (size_t)N, who, "for the filtered volume");
    if (!rc && both) rc = pnr::dev_alloc(bB, (size_t)N, who, "for the top-hat scratch");
    if (rc) return rc;
    uint8_t *const A = bA.get(), *const B = bB.get();
    const uint8_t *V = c->d_img;
    uint8_t *out = A;
    int launches = 0;
    pnr::Call call(c, who);
    c->tic();
    if (o.median) {
        call.launch(o.median == 3 ? median_k<true> : median_k<false>, dim3((unsigned)med_blocks), dim3(TPB), V, A, w, h, l, tiles_x, tiles_y);
        launches++;
        V = A;
    }
    if (o.tophat_r) {
        const int R = o.tophat_r;
        const int rz = l == 1 ? 0 : (int)((float)R / c->prm.zdist); // one IEEE division
        uint8_t *W = both ? B : A;
        out = W;
        const i64 nrows = (i64)h * l;
        launches += launch_x<false>(call, V, W, w, nrows, R);
        launches += launch_col<false>(call, W, W, nullptr, (i64)w * l, w, plane, h, R);
        if (rz) launches += launch_col<false>(call, W, W, nullptr, plane, plane, 0, l, rz);
        launches += launch_x<true>(call, W, W, w, nrows, R);
        launches += launch_col<true>(call, W, W, rz ? nullptr : V, (i64)w * l, w, plane, h, R);
        if (rz) launches += launch_col<true>(call, W, W, V, plane, plane, 0, l, rz);
    }
    c->toc("filter", launches);
    if ((rc = call.finish())) return rc;
    result = std::move(out == A ? bA : bB); // (the other buffer is freed here)
    return PNR_OK;
}
