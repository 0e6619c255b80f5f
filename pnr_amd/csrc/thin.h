// thin.h -- topological thinning of the traced 8-bit volume to a curve skeleton (thin.hip), behind pnr_skeletonize, and
// the skeleton's voxels as a forest, behind pnr_skeleton_forest.
#pragma once
#include "ctx.h"
#include <vector>

namespace pnr {

// the tile of one work-group of the mark and pass kernels; every extent is even, so a voxel's subfield is that of its place in the tile,
// and a work-group of THIN_TX / 2 x THIN_TY / 2 x THIN_TZ / 2 threads has one voxel of a subfield per thread
constexpr int THIN_TX = 32;
constexpr int THIN_TY = 8;
constexpr int THIN_TZ = 8;
// voxels per work-group of the count and list kernels (one raster-order chunk; a wave owns a contiguous quarter of it)
constexpr int THIN_CHUNK = 4096;

// The k voxels vox (linear indices of a w x h x l grid, any order; node i = vox[i]) as a forest, behind pnr_skeleton_forest: Kruskal over the
// 26-adjacent pairs under (len2, lo, hi); every key is distinct, so the forest is unique.  edges: sorted by (lo, hi), d = the step length.
// Pure host code; k and the grid are checked by the caller.  PNR_E_ARG: a voxel outside the grid or listed twice.
int skeleton_forest(const char *who, const int64_t *vox, int64_t k, int64_t w, int64_t h, int64_t l, std::vector<pnr_bridge> &edges);

} // namespace pnr

// The skeleton of {V >= t} of the context's volume under the rule of include/pnr_hip.h, on c's stream; the arguments are checked by the
// caller.  Host outputs, all nullable: info, skel_out (N), vox_out and deg_out (the first min(cap, n_skel)).  Every device buffer is
// freed before the call returns.
int pnr_thin_run(pnr_ctx *c, const char *who, const pnr_thin_opts &o, pnr_thin_info *info, uint8_t *skel_out, int64_t *vox_out, uint8_t *deg_out, int64_t cap);
