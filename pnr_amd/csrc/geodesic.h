// geodesic.h -- the gray-weighted geodesic distance through the traced 8-bit volume (geodesic.hip), behind pnr_geodesic_distance.
#pragma once
#include "ctx.h"

namespace pnr {

// the tile of one work-group of the relaxation: GEO_TX x GEO_TY threads, each owns the GEO_TZ voxels of a z column; with its halo of 1
// the tile's keys (u64) and costs (u16) are (GEO_TX + 2) (GEO_TY + 2) (GEO_TZ + 2) 10 = 20400 bytes of LDS
constexpr int GEO_TX = 32;
constexpr int GEO_TY = 8;
constexpr int GEO_TZ = 4;
// voxels (threads) per work-group of the source, compaction, statistics, split, sample and path kernels
constexpr int GEO_TPB = 256;

} // namespace pnr

// What one call hands over besides the context: the sources, the targets and the host outputs of pnr_geodesic_distance (all checked by
// the caller; every output is nullable).
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
};
// The keys of the context's volume under the rule of include/pnr_hip.h, on c's stream.  Every device buffer is freed before the call
// returns; c->geo_rounds / c->geo_visits hold the rounds and tile visits of the call.
int pnr_geodesic_run(pnr_ctx *c, const char *who, const pnr_geo_opts &o, const pnr_geo_call &g);
