// threshold.h -- thresholds of the traced 8-bit volume: the rules on its 256-bin histogram (threshold_rule.cpp, pure host), the
// histogram and the box sums of the local threshold on the device (threshold.hip); behind pnr_threshold_from_hist,
// pnr_auto_threshold, pnr_local_threshold and pnr_local_threshold_volume.
#pragma once
#include "ctx.h"

// The x pass of the local threshold takes a row in chunks of LT_XCH voxels (plus the box's halo on either side: LT_XCH + 2 *
// PNR_LOCAL_MAX_R = 2048 = 8 samples for each of 256 lanes).  The passes work on slabs of as many whole planes as hold at most
// LT_SLAB_VOX voxels (at least one plane; option "lt_slab_vox" lowers it).  tests/test_gpu_threshold.py reads these two lines.
constexpr int LT_XCH = 1920;
constexpr long long LT_SLAB_VOX = 1LL << 24;

namespace pnr {

// The rule of include/pnr_hip.h on the 256 counts: arguments (texts as `who`'s), then *info.  Pure host.
int threshold_rule(const char *who, const uint64_t *hist, const pnr_threshold_opts *opts, pnr_threshold_info *info);
// the reference's maxentropy_th (toolbox.cpp:657-737) on the histogram; every count below 2^31 (pnr_soma, PNR_THR_MAXENTROPY).  Both
// callers ask maxentropy_bins_fit first: PNR_OK, or PNR_E_ARG and "<who>: maxentropy needs every bin below 2^31, bin B holds N".
unsigned char maxentropy_from_hist(const unsigned long long *h);
int maxentropy_bins_fit(const char *who, const unsigned long long *h);

} // namespace pnr

// hist[256] (host) = the exact histogram of the N bytes at V (device memory) on c's stream, synchronised on return; the kernel is
// timed under `group`.  The 2 KiB of device bins are freed before it returns.  V is never written.
int pnr_hist_run(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, uint64_t *hist);

// a u8 volume in device memory: voxel (x, y, z) at V[(z * h + y) * w + x]; sides from 1, w * h below 2^31
struct pnr_local_vol {
    const uint8_t *V;
    int64_t w, h, l;
};
inline pnr_local_vol pnr_local_vol_of(const pnr_ctx *c) { return pnr_local_vol{c->d_img, c->w, c->h, c->l}; }

// The local threshold of the volume `vol` (never written; zdist is c's) with the validated options `o` on c's stream.  info and out (N host
// bytes) are nullable; keep (nullable) receives the device volume of the result.  Device memory of a call beyond the N bytes of
// the result: (6 s + 10 rz + 8) w h bytes, s = max(1, min(l, LT_SLAB_VOX / (w h))) planes -- the u16 x sums of the planes a slab
// adds (s + rz at most), a ring of s + 2 rz + 1 planes of u32 x-y sums, one plane of u32 running sums -- and 24 bytes of counters,
// freed before the call returns.  On any failure nothing is returned and the context is untouched.
int pnr_local_run(pnr_ctx *c, const char *who, const pnr_local_vol &vol, const pnr_local_opts &o, pnr_local_info *info, uint8_t *out, pnr::DevBuf<uint8_t> *keep);
