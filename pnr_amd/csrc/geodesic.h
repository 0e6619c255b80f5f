// geodesic.h -- the gray-weighted geodesic distance through the traced 8-bit volume (geodesic.hip), behind pnr_geodesic_distance.
#pragma once
#include "ctx.h"
#include "grid.h"

namespace pnr {

// the tile of one work-group of the relaxation: GEO_TX x GEO_TY threads, each owns the GEO_TZ voxels of a z column; with its halo of 1
// the tile's keys (u64) and costs (u16) are (GEO_TX + 2) (GEO_TY + 2) (GEO_TZ + 2) 10 = 20400 bytes of LDS
constexpr int GEO_TX = 32;
constexpr int GEO_TY = 8;
constexpr int GEO_TZ = 4;
// voxels (threads) per work-group of the source, statistics, split, sample and path kernels (= TILE_TPB: the extent check of tilework.h)
constexpr int GEO_TPB = 256;

using GeoDims = TileDims; // in tiles of GEO_TX x GEO_TY x GEO_TZ
// the 26 step lengths by (dz + 1) 9 + (dy + 1) 3 + (dx + 1): the offset order with the centre (0) in the middle
struct GeoLens {
    unsigned v[27];
};

} // namespace pnr

struct pnr_geo_call;
// What the hook of a call sees once the relaxation has settled: the device keys (D << 32) | label of every voxel (all ones: unreached),
// the volume, the threshold t, the cost table on the device, the dimensions and the step lengths.  Everything lives until the call returns.
struct pnr_geo_keys {
    const uint8_t *V;
    const unsigned long long *key;
    const uint16_t *ctab;
    int t;
    pnr::GeoDims d;
    pnr::GeoLens len;
};
// Runs on the context's stream after the relaxation and before the statistics and the target stage.  It may replace the targets of g
// (at_xyz, m, m_no_path, d_at, label_at, path_cap, path_len, path_vox; m = 0: none) -- whatever they point at must live until
// pnr_geodesic_run returns -- and may run the target stage itself (pnr_geo_targets).
typedef int (*pnr_geo_hook)(void *user, pnr_ctx *c, const char *who, const pnr_geo_keys &k, pnr_geo_call &g);

// What one call hands over besides the context: the sources, the targets and the host outputs of pnr_geodesic_distance (all checked by
// the caller; every output is nullable).  The last m_no_path targets are sampled but not walked.
struct pnr_geo_call {
    const float *src_xyz;
    const int32_t *src_label;
    int64_t n_src;
    pnr_geo_info *info;
    uint32_t *d_out;
    int32_t *label_out;
    const float *at_xyz;
    int64_t m;
    uint32_t *d_at;
    int32_t *label_at;
    int32_t path_cap;
    int32_t *path_len;
    int64_t *path_vox;
    pnr_geo_hook hook;
    void *hook_user;
    int64_t m_no_path;
};
// The target stage on settled keys, on c's stream: d_at / label_at of the g.m targets, and the walks of the first g.m - g.m_no_path of them
// (path_cap > 0).  Its device buffers are freed before it returns, synchronised.  pnr_geodesic_run ends in it; a hook may call it as well.
int pnr_geo_targets(pnr_ctx *c, const char *who, const pnr_geo_keys &k, const pnr_geo_call &g);
// The keys of the context's volume under the rule of include/pnr_hip.h, on c's stream.  Every device buffer is freed before the call
// returns; c->geo_rounds / c->geo_visits hold the rounds and tile visits of the call.
int pnr_geodesic_run(pnr_ctx *c, const char *who, const pnr_geo_opts &o, const pnr_geo_call &g);
