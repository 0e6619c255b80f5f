// radius.h -- SWC node radii measured from the traced 8-bit volume (radius.hip), behind pnr_measure_radii.
#pragma once
#include "ctx.h"

namespace pnr {
// The shells of the rule (include/pnr_hip.h), concatenated in ascending k, raster order (dz, dy, dx) inside a shell:
// off[i] = (dx + 64) | (dy + 64) << 8 | (dz + 64) << 16; shell k = off[start[k], start[k + 1]), k = 0..rmax.  Pure host code.
struct RadiusTable {
    std::vector<uint32_t> off;
    std::vector<int32_t> start; // rmax + 2 entries
};
void build_radius_table(float zdist, int rmax, bool is2d, RadiusTable &t);
} // namespace pnr

// Measures the n positions xyz (host, n x 3) on c's volume and stream with the validated options `o`; k_out: host, n.  thr_used
// (nullable): the threshold of the absolute mode, 0 in the relative mode.  The offset table is cached in the context; every other
// device buffer is freed before the call returns.
int pnr_radius_run(pnr_ctx *c, const float *xyz, int64_t n, const pnr_radius_opts &o, int32_t *k_out, int32_t *thr_used);
