// What the rigid (slac.cpp) and non-rigid (slac_nonrigid.cpp) optimizers
// share on the host: pose rounding, the edge checks and the correspondence
// sets of a pose graph.
#pragma once

#include <cstdint>
#include <vector>

#include "common.h"
#include "o3d_mi355x_host.h"
#include "slac.h"

namespace o3dmi {

constexpr int kSlacMaxNodes = 512;  // a 3072^2 float64 host matrix, 75 MB

inline void Pose12(const double* T, float* out) {
    for (int k = 0; k < 12; ++k) out[k] = (float)T[k];
}

inline int CheckEdges(const int32_t* edges, int n_edges, int n_nodes) {
    for (int e = 0; e < n_edges; ++e) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        O3DMI_REQUIRE(i >= 0 && j >= 0 && i < n_nodes && j < n_nodes,
                      "node id out of range");
        O3DMI_REQUIRE(i != j, "an edge joins two different nodes");
    }
    return O3DMI_OK;
}

// The argument checks both optimizers start with.
inline int CheckPoseGraph(const void* const* positions_dev,
                          const void* const* normals_dev,
                          const int64_t* sizes, int n_nodes,
                          const double* poses, const int32_t* edges,
                          const double* T_ij, int n_edges) {
    O3DMI_REQUIRE(n_nodes > 0 && n_edges >= 0, "empty pose graph");
    if (n_nodes > kSlacMaxNodes) {
        SetLastError("slac: more than 512 nodes are not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    O3DMI_REQUIRE(positions_dev && normals_dev && sizes && poses &&
                          (n_edges == 0 || (edges && T_ij)),
                  "null argument");
    const int st = CheckEdges(edges, n_edges, n_nodes);
    if (st) return st;
    for (int k = 0; k < n_nodes; ++k)
        O3DMI_REQUIRE(sizes[k] > 0 && positions_dev[k] && normals_dev[k],
                      "empty fragment");
    return O3DMI_OK;
}

// o3dmi_slac_correspondence_set for every edge, once, from the input graph:
// ed[e] = {set, count (0 when the edge is not kept), i, j}; the sets live in
// `sc`. kept / n_corres / n_inliers (each may be null) as the optimizers
// report them, n_inliers zeroed.
inline int SlacCorrespondenceSets(const void* const* positions_dev,
                                  const int64_t* sizes, const double* poses,
                                  const int32_t* edges, const double* T_ij,
                                  int n_edges, float distance_threshold,
                                  float fitness_threshold, PoolScratch& sc,
                                  std::vector<SlacEdge>& ed, int32_t* kept,
                                  int64_t* n_corres, int64_t* n_inliers,
                                  o3dmi_stream_t stream) {
    ed.assign((size_t)n_edges, SlacEdge{});
    for (int e = 0; e < n_edges; ++e) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        int64_t* corres = nullptr;
        int st = sc.Alloc(&corres, 16 * (size_t)sizes[i]);
        if (st) return st;
        int64_t C = 0, inl = 0;
        float ratio = 0;
        int keep = 0;
        if ((st = o3dmi_slac_correspondence_set(
                     positions_dev[i], sizes[i], positions_dev[j], sizes[j], i,
                     j, poses + 16 * i, poses + 16 * j, T_ij + 16 * e,
                     distance_threshold, fitness_threshold, corres, &C, &inl,
                     &ratio, &keep, stream)))
            return st;
        ed[e].corres = corres;
        ed[e].count = keep ? C : 0;
        ed[e].i = i;
        ed[e].j = j;
        if (kept) kept[e] = keep;
        if (n_corres) n_corres[e] = C;
        if (n_inliers) n_inliers[e] = 0;
    }
    return O3DMI_OK;
}

// UpdatePoses (SLACOptimizer.cpp:265-286) in float64:
// T_k <- PoseToTransformation(x[6k..6k+5]) T_k.
inline void SlacUpdatePoses(const double* x, int n_nodes, double* T) {
    for (int k = 0; k < n_nodes; ++k) {
        double D[16], R[16];
        o3dmi_pose_to_transformation(x + 6 * (size_t)k, D);
        double* Tk = T + 16 * (size_t)k;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                double v = 0;
                for (int m = 0; m < 4; ++m) v += D[4 * r + m] * Tk[4 * m + c];
                R[4 * r + c] = v;
            }
        for (int m = 0; m < 16; ++m) Tk[m] = R[m];
    }
}

}  // namespace o3dmi
