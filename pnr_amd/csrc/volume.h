// volume.h -- 16-bit (and multi-channel) stacks windowed to the 8-bit volume the pipeline traces (volume.hip), behind
// pnr_set_volume_u16[_device]; and what is computed over the whole 8-bit stack: its byte sum and mean threshold.
#pragma once
#include "ctx.h"

// Maps channel `channel` of the u16 device buffer d_src (voxel i at element i * nchan + channel, c->N voxels: set_dims has run)
// into the context's owned u8 volume c->d_img_owned, on c->stream, with the window `win` (validated by the caller; lo = hi = -1:
// from the stack).  Returns the window used.  Allocation failures return PNR_E_NOMEM; c->d_img is not touched.
int pnr_volume_u16_run(pnr_ctx *c, const uint16_t *d_src, int nchan, int channel, const pnr_window &win, int32_t *lo_out, int32_t *hi_out);

// The exact u64 sum of the N bytes at V (device memory): *sum, through the device word d_sum (zeroed here), on c's stream
// (synchronised on return); the kernel is timed under `group`.  A HIP failure is reported as `who`'s.
int pnr_byte_sum_run(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, unsigned long long *d_sum, unsigned long long *sum);
// The threshold "thr = -1" of the radii, the coverage and the components: *t = the floor of the exact mean of V, at least 1.
int pnr_mean_threshold(pnr_ctx *c, const char *who, const char *group, const uint8_t *V, int64_t N, unsigned long long *d_word, int *t);

namespace pnr {
// A tool's finished result becomes the context's volume (pnr_filter_volume, pnr_despeckle_volume; api.cpp): what pnr_set_volume of the same
// bytes leaves -- owned, the same dimensions, no later pipeline state.
void replace_volume(pnr_ctx *c, DevBuf<uint8_t> &&v);
} // namespace pnr
