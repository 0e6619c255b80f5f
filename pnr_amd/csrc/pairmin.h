// pairmin.h -- the all-pairs minimum that distance.hip (points x segments) and join.hip (points x points of other trees) share: per
// point i the minimum of d2(i, j) over the j that count, and the smallest j at that minimum.  What d2 is and which pairs count is the
// RULE of the user (DistRule, JoinRule); everything here is the same for both.
//
// pair_min has one thread per point with the point in registers; the index j of its loop is the same in every lane, so what the rule
// reads of j arrives through scalar loads (none per lane) and the vector unit only does the operations of the pair -- no vector load,
// no LDS, nothing per lane inside the loop.  blockIdx.y cuts the j into slices, so that a few thousand points still fill the chip;
// every thread ends with ONE 64-bit atomicMin on (bits(d2) << 32) | j -- d2 >= +0, so its bit pattern orders like its value, and the
// low word makes the smallest j win a tie.  The result therefore does not depend on the slices or on how the (points x j) rectangle
// is cut into launches: pair_tiles bounds a launch by a pair budget, so that no single kernel occupies the GPU for seconds.
// pair_finish unpacks the keys.
//
// A rule is passed to the kernel by value and supplies:
//   struct Point;                                   what a thread keeps of its point
//   Point point(int i) const;                       ... and how it is loaded
//   bool live(const Point &) const;                 does the point take part at all (its key stays untouched otherwise)
//   int first(int j0) const;                        the index a thread reports whose minimum stays +inf: j0 of its slice, or -1 = none
//   bool pair(const Point &, int j, float &d2) const;  d2 of the pair; false: the pair does not count
#pragma once
#include "ctx.h"

namespace pnr {

constexpr int PAIR_TPB = 256;               // threads of a work-group = points of a block row
constexpr int MIN_SPLIT = 64;               // automatic slices hold at least this many j: one atomic per 64 pairs at the most
constexpr int TARGET_BLOCKS = 2048;         // automatic slices: work-groups of a launch that fill 256 CUs eight deep
constexpr long long AUTO_PAIRS = 1ll << 34; // pairs per launch: some 10 ms

// one launch: points [p0, p1) x j in [s0, s1) in slices of `split`, on a grid of gx x gy work-groups
struct PairTile {
    long long p0, p1, s0, s1, split, gx, gy;
};

// The n x m rectangle in launches of at most `budget` pairs (whole block rows; at least one row by one j), rows outer, j inner; f(tile)
// is called for each in turn and ends the walk by returning false.  split_opt / budget_opt: the options *_split and
// *_pairs_per_launch (0 = automatic).  Pure host code.
template <class F>
void pair_tiles(long long n, long long m, long long split_opt, long long budget_opt, F &&f)
{
    const long long budget = budget_opt > 0 ? budget_opt : AUTO_PAIRS;
    const long long rows_fit = budget / m / PAIR_TPB * PAIR_TPB;
    const long long rows = std::min<long long>(std::max<long long>(rows_fit, PAIR_TPB), (n + PAIR_TPB - 1) / PAIR_TPB * PAIR_TPB);
    const long long segs = rows_fit >= PAIR_TPB ? m : std::max<long long>(1, budget / PAIR_TPB);
    for (long long p0 = 0; p0 < n; p0 += rows)
        for (long long s0 = 0; s0 < m; s0 += segs) {
            const long long p1 = std::min<long long>(p0 + rows, n), s1 = std::min<long long>(s0 + segs, m), ms = s1 - s0;
            const long long gx = (p1 - p0 + PAIR_TPB - 1) / PAIR_TPB;
            long long split = split_opt;
            if (split <= 0) { // enough slices to fill the chip, of at least MIN_SPLIT j
                const long long slices = std::max<long long>(1, std::min<long long>((TARGET_BLOCKS + gx - 1) / gx, ms / MIN_SPLIT));
                split = (ms + slices - 1) / slices;
            }
            split = std::max<long long>(split, (ms + 65534) / 65535); // (gridDim.y)
            if (!f(PairTile{p0, p1, s0, s1, split, gx, (ms + split - 1) / split})) return;
        }
}

// points [p0, p1) x j in [s0, s1); blockIdx.y = the slice of `split` j
template <class Rule>
__global__ __launch_bounds__(PAIR_TPB) void pair_min(Rule r, int p0, int p1, int s0, int s1, int split, unsigned long long *__restrict__ key)
{
    const int i = p0 + blockIdx.x * PAIR_TPB + threadIdx.x;
    const int j0 = s0 + blockIdx.y * split, j1 = min(j0 + split, s1);
    const typename Rule::Point P = r.point(min(i, p1 - 1)); // (the lanes past the last point run along on it and write nothing)
    float best = INFINITY;
    int bj = r.first(j0);
#pragma unroll 4
    for (int j = j0; j < j1; j++) { // j is wave-uniform: scalar loads
        float d2;
        if (r.pair(P, j, d2) && d2 < best) best = d2, bj = j; // (ascending j: the first of equals stays)
    }
    if (i < p1 && r.live(P)) atomicMin(&key[i], (unsigned long long)__float_as_uint(best) << 32 | (unsigned)bj);
}

// root: d = sqrtf(d2), else d2; a point without a partner (its key untouched, or its minimum still +inf at index -1): +inf and j = -1
static __global__ __launch_bounds__(PAIR_TPB) void pair_finish(const unsigned long long *__restrict__ key, int n, int root, float *__restrict__ d, int *__restrict__ j)
{
    const int i = blockIdx.x * PAIR_TPB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    const int bj = (int)(unsigned)k;
    const float d2 = __uint_as_float((unsigned)(k >> 32));
    d[i] = bj < 0 ? INFINITY : root ? sqrtf(d2) : d2;
    j[i] = bj;
}

// pair_min<Rule> over every tile of the n x m rectangle on st, up to the first launch that fails; *launches = how many it made
template <class Rule>
hipError_t pair_sweep(hipStream_t st, const Rule &r, long long n, long long m, long long split_opt, long long budget_opt, unsigned long long *key, int *launches)
{
    hipError_t e = hipSuccess;
    *launches = 0;
    pair_tiles(n, m, split_opt, budget_opt, [&](const PairTile &t) {
        hipLaunchKernelGGL(pair_min<Rule>, dim3((unsigned)t.gx, (unsigned)t.gy), dim3(PAIR_TPB), 0, st, r, (int)t.p0, (int)t.p1, (int)t.s0, (int)t.s1, (int)t.split, key);
        e = hipGetLastError();
        ++*launches;
        return e == hipSuccess;
    });
    return e;
}

} // namespace pnr
