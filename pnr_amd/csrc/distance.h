// distance.h -- the bidirectional tree distance (distance.hip), behind pnr_point_segment_distance / pnr_tree_sample / pnr_tree_distance.
#pragma once
#include "ctx.h"
#include <vector>

namespace pnr {
// The sample points of a tree by the rule of include/pnr_hip.h: z *= zscale (f32), then in node order the node itself and, for a
// node with a parent and step > 0, the q - 1 interior points of its segment (f64, rounded to f32).  *n_out = the number of points;
// the first min(cap, *n_out) of them are written to pts_out (x, y, z) and owner_out (the node), either may be NULL.  Pure host
// code.  PNR_E_ARG: a parent outside [-1, n) (any negative value = none), a coordinate that is not finite, a segment of more than
// 2^31 steps.
int tree_sample(const float *xyz, const int32_t *parent, int64_t n, float zscale, float step, float *pts_out, int32_t *owner_out, int64_t cap,
                int64_t *n_out);

// one side of pnr_tree_distance: the sample points with their nodes, and the segments (a = the node, b = its parent or itself)
struct TreeSide {
    std::vector<float> pts, a, b, d;
    std::vector<int32_t> owner;
    int64_t np = 0, n = 0;
};
// Fills s but for d (np entries, zero) from tree `which` ("A" / "B") of pnr_tree_distance.  PNR_E_ARG: the node count or the pointers, what
// tree_sample refuses, more than 2^22 sample points.
int tree_side(const char *which, const float *xyz, const int32_t *parent, int64_t n, const pnr_distance_opts &o, TreeSide &s);
// the metrics of one direction over its distances d (not empty): sequential f64 sums in point order
void direction_metrics(const std::vector<float> &d, float thr, pnr_distance_dir &r);
} // namespace pnr

// d_out[i] = the distance of point i (pts: host, n x 3) to the nearest of the m segments (seg_a, seg_b: host, m x 3), j_out[i]
// (nullable) = the smallest index of a segment at that distance; validated arguments, n >= 1.  DistRule under the pair minimum of
// pairmin.h.  Runs on c's stream; every device buffer is freed before the call returns.
int pnr_distance_run(pnr_ctx *c, const float *pts, int64_t n, const float *seg_a, const float *seg_b, int64_t m, float *d_out, int32_t *j_out);
