// geojoin.h -- the traced forest joined along the signal (geojoin.hip), behind pnr_geodesic_bridges / pnr_join_expand: the minimum spanning
// forest of the fragments under gray-weighted path cost, found on the settled keys of one geodesic pass (geodesic.h).
#pragma once
#include "geodesic.h"
#include <vector>

// The bridges of the forest (xyz, parent, n: checked by the caller) through the context's volume under the rule of include/pnr_hip.h, in
// ascending key order, and their voxel chains s_a .. p, q .. s_b one after the other in `chain` (pnr_geo_bridge::path_off / path_len).
// Runs on c's stream; every device buffer is freed before the call returns; c->geojoin_rounds holds the Boruvka rounds of the call.
int pnr_geojoin_run(pnr_ctx *c, const float *xyz, const int32_t *parent, int64_t n, const pnr_geojoin_opts &o, pnr_geojoin_info *info,
                    std::vector<pnr_geo_bridge> &bridges, std::vector<int64_t> &chain);
// the expansion of the rule; pure host
int pnr_geojoin_expand(const float *xyz, const int32_t *parent, int64_t n, const pnr_geo_bridge *bridges, int64_t nb, const int64_t *path_vox, int64_t n_path, int64_t w,
                       int64_t h, int64_t l, float *xyz_out, int32_t *parent_out, int32_t *bridge_of, int64_t cap_nodes, int64_t *n_nodes, pnr_bridge *join_out);
