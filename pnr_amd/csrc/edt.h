// edt.h -- the exact anisotropic Euclidean distance transform of the traced 8-bit volume (edt.hip), behind pnr_distance_transform.
#pragma once
#include "ctx.h"

namespace pnr {

// the x pass: a wave walks one row in words of EDT_WX voxels (one ballot each), a work-group takes EDT_ROWS rows
constexpr int EDT_WX = 64;
constexpr int EDT_ROWS = 4;
// the y, z, statistics and sample kernels: threads along x, EDT_TPB consecutive voxels (linear index) per work-group
constexpr int EDT_TPB = 256;

} // namespace pnr

// D2 of {V >= t} of the context's volume under the rule of include/pnr_hip.h, on c's stream; the arguments are checked by the caller.
// Host outputs, all nullable: info, d2_out (N), d2_at (n, with xyz n x 3).  Every device buffer is freed before the call returns.
int pnr_edt_run(pnr_ctx *c, const char *who, const pnr_edt_opts &o, pnr_edt_info *info, float *d2_out, const float *xyz, int64_t n, float *d2_at);
