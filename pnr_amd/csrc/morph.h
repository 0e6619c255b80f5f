// morph.h -- grey-level morphological reconstruction of the traced 8-bit volume (morph.hip), behind pnr_morph_reconstruct and
// pnr_morph_volume.
#pragma once
#include "ctx.h"

namespace pnr {

// the tile of one work-group of the relaxation: MORPH_TX x MORPH_TY threads, each owns the MORPH_TZ voxels of a z column; with its halo
// of 1 the tile's state and mask bytes are (MORPH_TX + 2) (MORPH_TY + 2) (MORPH_TZ + 2) 2 = 6800 bytes of LDS
constexpr int MORPH_TX = 32;
constexpr int MORPH_TY = 8;
constexpr int MORPH_TZ = 8;
// voxels (threads) per work-group of the init and finish kernels (= TILE_TPB: the extent check of tilework.h)
constexpr int MORPH_TPB = 256;

} // namespace pnr

// One reconstruction of the context's volume under the rule of include/pnr_hip.h, on c's stream.  o is checked and its connectivity
// resolved by the caller (4, 8, 6 or 26); marker: N host bytes for ops 1 and 2, else NULL.  info and out (N host bytes) are nullable.
// keep (nullable): receives the device volume of the result, for the caller to make it the context's; every other device buffer of the
// call -- and without keep that one too -- is freed before the call returns.  c->morph_rounds / c->morph_visits hold the rounds and tile
// visits of the call.  V is never written.
int pnr_morph_run(pnr_ctx *c, const char *who, const pnr_morph_opts &o, const uint8_t *marker, pnr_morph_info *info, uint8_t *out, pnr::DevBuf<uint8_t> *keep);
