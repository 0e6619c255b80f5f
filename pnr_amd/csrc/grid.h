// grid.h -- the rules the volume tools share, each written once: the centre voxel of a position (the radius rule of include/pnr_hip.h),
// a tile's place and a voxel's linear index, the host scan of the chunk counts of a raster-order compaction, and the size of a
// grid-stride launch.  Users: radius, edt, tilework (morph, watershed, geodesic), geojoin, components, thin, render, volume, threshold.  Small inline functions.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pnr {

// ---- the centre voxel: c = (int) min(max(v + 0.5, 0), extent - 1) per axis, for positions whose three floats are finite ----
__host__ __device__ inline bool finite3(float x, float y, float z)
{
    auto finite = [](float f) { return (__builtin_bit_cast(unsigned, f) & 0x7f800000u) != 0x7f800000u; };
    return finite(x) && finite(y) && finite(z);
}
__host__ __device__ inline int centre_axis(float v, int extent) { return (int)fminf(fmaxf(v + 0.5f, 0.f), (float)(extent - 1)); }
__host__ __device__ inline long long voxel_index(int w, int h, int x, int y, int z) { return ((long long)z * h + y) * w + x; }
__host__ __device__ inline long long centre_voxel(int w, int h, int l, float px, float py, float pz)
{
    return voxel_index(w, h, centre_axis(px, w), centre_axis(py, h), centre_axis(pz, l));
}

// ---- a volume's extents and its tiles along every axis (built and checked by tile_dims, tilework.h) ----
struct TileDims {
    int w, h, l, ntx, nty, ntz;
    int64_t tiles() const { return (int64_t)ntx * nty * ntz; }
};

// ---- tile number (x fastest) -> its place in the tile grid and its first voxel; fewer than 2^31 tiles ----
struct TileAt {
    int tx, ty, tz;
    int x0, y0, z0;
};
__host__ __device__ inline TileAt tile_origin(unsigned tile, int tiles_x, int tiles_y, int TX, int TY, int TZ)
{
    const unsigned per_z = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned tz = tile / per_z, r = tile - tz * per_z, ty = r / (unsigned)tiles_x, tx = r - ty * (unsigned)tiles_x;
    return TileAt{(int)tx, (int)ty, (int)tz, (int)tx * TX, (int)ty * TY, (int)tz * TZ};
}

// ---- at most `cap` work-groups, at least one ----
constexpr int MAX_BLOCKS = 2048; // grid-stride loops beyond this many work-groups: 256 CUs eight deep
inline unsigned grid_blocks(long long wanted, long long cap = MAX_BLOCKS) { return (unsigned)std::max<long long>(1, std::min(wanted, cap)); }

// ---- the host half of the raster-order compactions (thin_count / thin_list, cc_flatten / cc_number): the per-chunk counts become
// their exclusive scan; returns their sum ----
inline int64_t exclusive_scan_counts(std::vector<unsigned> &counts)
{
    int64_t K = 0;
    for (auto &v : counts) {
        const unsigned n = v;
        v = (unsigned)K;
        K += n;
    }
    return K;
}

} // namespace pnr
