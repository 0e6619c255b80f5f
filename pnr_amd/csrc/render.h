// render.h -- a tree rendered into the stack (render.hip), behind pnr_render_tree / pnr_tree_coverage and the tap pnr_render_items.
#pragma once
#include "ctx.h"
#include <functional>

namespace pnr {

constexpr int RENDER_AUTO_PIECE = 16;                  // option render_piece = 0: xy voxels of axis per piece
constexpr long long RENDER_AUTO_BOX = 1ll << 15;       // option render_box = 0: voxels per item (128 per lane of a work-group)
constexpr long long RENDER_AUTO_ITEMS = 1ll << 18;     // option render_items_per_launch = 0

// the constants of the rule (include/pnr_hip.h) for every segment, on the host in f32 (the library's host code is built with
// -ffp-contract=off as well): three float4 per segment -- (a, r), (ab, ra), (dr, 0, 0, 0) -- as rn_scatter reads them
struct RenderTree {
    std::vector<float> seg; // n x 12
    float zscale = 1.f;
    int64_t n = 0;
};
// validates the tree by the rule's argument list and fills t; `who` prefixes the message
int render_prepare(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts &o, RenderTree &t);

// one work item: segment `seg` against the voxels [x0, x1] x [y0, y1] x [z0, z1] (inclusive, inside the grid)
struct RenderItem {
    int64_t seg, x0, y0, z0, x1, y1, z1;
};
// The items of the tree on the grid w x h x l in segment order: every segment is cut along its axis into pieces of at most `piece`
// xy voxels, each piece gets the integer box of its axis sub-interval grown by max(ra, rb) + 1 (z divided by zscale), clipped to the
// grid, and a box of more than `box` voxels is cut into sub-boxes.  piece, box <= 0: automatic.  f(item) returns false to end the
// walk.  Pure host code.
void render_items(const RenderTree &t, int64_t w, int64_t h, int64_t l, int64_t piece, int64_t box, const std::function<bool(const RenderItem &)> &f);

} // namespace pnr

// Renders the prepared tree on the grid w x h x l on c's stream.  V (device, nullable): the volume of the coverage counts; thr: the
// option of the rule (-1: the mean of V).  Host outputs, all nullable: label_out / mask_out / residual_out (N each), cov (the six
// counts and thr_used; the ratios are the caller's), seg_vox / seg_fg / seg_sum (n each).  Every device buffer
// is freed before the call returns.
int pnr_render_run(pnr_ctx *c, const char *who, const pnr::RenderTree &t, int64_t w, int64_t h, int64_t l, const uint8_t *V, int thr, int32_t *label_out,
                   uint8_t *mask_out, uint8_t *residual_out, pnr_coverage *cov, int64_t *seg_vox, int64_t *seg_fg, int64_t *seg_sum);
