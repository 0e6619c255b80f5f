// filter.h -- the pre-filters of the traced 8-bit volume (filter.hip), behind pnr_filter_volume: a 3 x 3 (x 3) median and a flat-box
// top-hat background subtraction.
#pragma once
#include "ctx.h"

// The tile of the median kernel: a work-group of 256 computes MED_TX x MED_TY voxels of a plane (MED_TX / 4 lanes of four
// voxels each in x) and marches down MED_ZC planes.  tests/test_gpu_filter.py reads these four lines for its tile-boundary shape.
constexpr int MED_TX = 128;
constexpr int MED_TY = 8;
constexpr int MED_ZC = 32;
// The x pass of the top-hat works on chunks of TH_CH voxels of a row (plus the halo of the box) in LDS.
constexpr int TH_CH = 2048;

// Filters c's volume (c->d_img, never written) with the validated options `o` (at least one stage on) on c's stream into a new
// device buffer of c->N bytes, moved into `result`.  At most one more buffer of N bytes lives during the
// call.  A failed allocation returns PNR_E_NOMEM; on any failure nothing is returned and the context is untouched.
int pnr_filter_run(pnr_ctx *c, const pnr_filter_opts &o, pnr::DevBuf<uint8_t> &result);
