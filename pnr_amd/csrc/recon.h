// recon.h -- the device forms of the two neighbour stages of reconstruct() (recon.hip), behind pnr_reconstruct_ctx.
#pragma once
#include "ctx.h"
#include "../host/reconstruct.h"

// non-blurring mean-shift of src on the context's GPU: the bits of reconstruct.cpp mean_shift (res[0] = src[0])
int pnr_recon_shift(pnr_ctx *c, const std::vector<advantra::P4> &src, float sig2radius, int refine_iter, float epsilon2,
                    std::vector<advantra::P4> &res);
// the grouping's ball lists over pos (group_spheres' distance test), every list ascending
int pnr_recon_balls(pnr_ctx *c, const std::vector<advantra::P4> &pos, float group_radius, advantra::BallLists &out);
