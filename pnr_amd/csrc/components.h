// components.h -- 3-D connected components of the traced 8-bit volume (components.hip), behind pnr_label_components /
// pnr_despeckle_volume.
#pragma once
#include "ctx.h"

namespace pnr {

// the tile of one work-group of the local, merge and statistics kernels: CC_TX x CC_TY voxels per slice, one slice per thread and step
constexpr int CC_TX = 32;
constexpr int CC_TY = 8;
constexpr int CC_TZ = 4;
// voxels per work-group of the flatten and number kernels (one raster-order chunk; a wave owns a contiguous quarter of it)
constexpr int CC_CHUNK = 4096;

} // namespace pnr

// The components of {V >= t} of the context's volume under the rule of include/pnr_hip.h, on c's stream; the arguments are checked
// by the caller.  Host outputs, all nullable: info, label_out (N), comps (the first min(cap, n_comp)).  despeckled (nullable): receives a
// device buffer of N bytes with the components below min_size cleared.  Every other device buffer is freed before the call returns.
int pnr_components_run(pnr_ctx *c, const char *who, const pnr_components_opts &o, pnr_components_info *info, int32_t *label_out, pnr_component *comps,
                       int64_t cap, pnr::DevBuf<uint8_t> *despeckled);
