// hist.h -- the exact histogram of one work-group, written once for its two users: the radix select of the 16-bit windowing
// (volume.hip: 256 coarse and 2 x 256 fine bins of a u16 channel) and the 256 bins of the u8 volume (threshold.hip).
//
// A work-group of HIST_TPB threads keeps a private copy of the NB bins per wave in LDS (u32: a wave's share of a launch is far
// below 2^32 voxels), so that an LDS atomic is contended by the 64 lanes of one wave only.  The voxels of one bin -- `hot`, the
// bin of the stack's first voxel: the background of a dark stack -- are counted in a register instead: a wave whose 64 lanes
// all add to the same LDS word is serialised 64-fold.  At the end the copies are added up and every non-empty bin costs one u64
// atomic per work-group (2^32 voxels overflow u32 counters).
#pragma once
#include <hip/hip_runtime.h>

namespace pnr {

constexpr int HIST_TPB = 1024;            // threads of a histogram work-group
constexpr int HIST_WAVES = HIST_TPB / 64; // ... one private LDS copy of the bins per wave

__device__ __forceinline__ unsigned wave_sum_u32(unsigned x)
{
    for (int d = 32; d >= 1; d >>= 1) x += (unsigned)__shfl_xor((int)x, d, 64);
    return x;
}

// visit(f): calls f(v) for every voxel this thread owns; key(v) -> bin in [0, NB) or -1 (not counted); hot: the bin counted in
// registers (-1: none); out: NB u64 totals in device memory
template <int NB, class V, class K>
__device__ __forceinline__ void histogram(V &&visit, K &&key, int hot, unsigned long long *out)
{
    __shared__ unsigned h[HIST_WAVES][NB];
    for (int k = threadIdx.x; k < HIST_WAVES * NB; k += HIST_TPB) (&h[0][0])[k] = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    unsigned nhot = 0;
    visit([&](unsigned v) {
        const int b = key(v);
        if (b == hot) nhot++;
        else if (b >= 0) atomicAdd(&h[w][b], 1u);
    });
    if (hot >= 0) {
        nhot = wave_sum_u32(nhot);
        if ((threadIdx.x & 63) == 0) atomicAdd(&h[w][hot], nhot);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < NB; b += HIST_TPB) {
        unsigned long long t = 0;
        for (int k = 0; k < HIST_WAVES; k++) t += h[k][b];
        if (t) atomicAdd(&out[b], t);
    }
}

} // namespace pnr
