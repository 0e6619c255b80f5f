// watershed.h -- the marker-controlled watershed of the traced 8-bit volume (watershed.hip), behind pnr_watershed.
#pragma once
#include "ctx.h"

namespace pnr {

// the tile of one work-group of the two relaxations: WS_TX x WS_TY threads, each owns the WS_TZ voxels of a z column (the morph tile)
constexpr int WS_TX = 32;
constexpr int WS_TY = 8;
constexpr int WS_TZ = 8;
// voxels (threads) per work-group of the init and finish kernels (= TILE_TPB: the extent check of tilework.h)
constexpr int WS_TPB = 256;

} // namespace pnr

// the markers of a call, in exactly one of the two forms (checked by the caller): a host volume of N labels (> 0: a label, 0: none; n_pos of
// them are positive), or n_src points with their labels (NULL: 1 .. n_src)
struct pnr_ws_markers {
    const int32_t *vol;
    int64_t n_pos;
    const float *src_xyz;
    const int32_t *src_label;
    int64_t n_src;
};

// One watershed of the context's volume under the rule of include/pnr_hip.h, on c's stream.  o is checked and its connectivity resolved
// by the caller (4, 8, 6 or 26); relief: N host bytes or NULL (255 - V).  info, label_out (N host int32) and level_out (N host bytes) are
// nullable.  Every device buffer of the call is freed before it returns; c->ws_rounds / c->ws_visits hold the rounds and tile visits of
// the two passes together.  V is never written.
int pnr_watershed_run(pnr_ctx *c, const char *who, const pnr_watershed_opts &o, const uint8_t *relief, const pnr_ws_markers &m, pnr_watershed_info *info, int32_t *label_out,
                      uint8_t *level_out);
