// RunSLACOptimizerForFragments (t/pipelines/slac/SLACOptimizer.cpp:253-367)
// and the two FillInSLAC*Term seams (slac/FillInLinearSystemImpl.h:102-236)
// over the kernels of slac_nonrigid.hip, for fragments in device memory.
//
// An iteration is: zero the float64 system, one launch for the alignment terms
// of every edge, the per-edge final pass, the pose blocks, the regularizer,
// the anchor pin, the Cholesky solve, and one download of E x 29 + 1 + n
// doubles. The system
// never leaves the device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "control_grid.h"
#include "host/slac_common.h"
#include "o3d_mi355x_host.h"
#include "slac.h"

using namespace o3dmi;

namespace {

// The float64 scratch system behind a float32 seam.
struct SeamSystem {
    SlacSystem sys{};
    double* tail = nullptr;  // [29 sums | regularizer residual]
    int Make(PoolScratch& sc, int64_t n_vars, int n_frags, hipStream_t s) {
        int st;
        if ((st = sc.Alloc(&sys.AtA, sizeof(double) * (size_t)n_vars *
                                             (size_t)n_vars)) ||
            (st = sc.Alloc(&sys.Atb, sizeof(double) * (size_t)n_vars)) ||
            (st = sc.Alloc(&tail, sizeof(double) * (kSlacSums + 1))) ||
            (st = sc.Alloc(&sys.counters, 2 * sizeof(int))))
            return st;
        sys.n = n_vars;
        sys.n_frags = n_frags;
        O3DMI_HIP_CHECK(hipMemsetAsync(
                sys.AtA, 0, sizeof(double) * (size_t)n_vars * (size_t)n_vars,
                s));
        O3DMI_HIP_CHECK(hipMemsetAsync(sys.Atb, 0,
                                       sizeof(double) * (size_t)n_vars, s));
        O3DMI_HIP_CHECK(hipMemsetAsync(tail, 0,
                                       sizeof(double) * (kSlacSums + 1), s));
        O3DMI_HIP_CHECK(hipMemsetAsync(sys.counters, 0, 2 * sizeof(int), s));
        return O3DMI_OK;
    }
    // Waits; the seam's error rule.
    int Finish(hipStream_t s) {
        int bad = 0;
        O3DMI_HIP_CHECK(hipMemcpyAsync(&bad, sys.counters, sizeof(int),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        O3DMI_REQUIRE(!bad, "slac: control node index out of range");
        return O3DMI_OK;
    }
};

int CheckSeamSystem(const float* AtA, const float* Atb, const float* residual,
                    int64_t n_vars, int n_frags) {
    O3DMI_REQUIRE(AtA && Atb && residual, "null argument");
    O3DMI_REQUIRE(n_frags > 0 && n_vars >= 6 * (int64_t)n_frags,
                  "n_vars must be at least 6 x the number of fragments");
    if (n_vars > kSlacMaxVars) {
        SetLastError("slac: more than 32768 unknowns are not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    return O3DMI_OK;
}

}  // namespace

extern "C" int o3dmi_fill_in_slac_alignment_term(
        float* AtA_dev, float* Atb_dev, float* residual_dev, int64_t n_vars,
        const float* Ti_Cps_dev, const float* Tj_Cqs_dev,
        const float* Cnormal_ps_dev, const float* Ri_Cnormal_ps_dev,
        const float* RjT_Ri_Cnormal_ps_dev, const int32_t* cgrid_idx_ps_dev,
        const int32_t* cgrid_idx_qs_dev, const float* cgrid_ratio_ps_dev,
        const float* cgrid_ratio_qs_dev, int64_t n, int i, int j, int n_frags,
        float threshold, o3dmi_stream_t stream) {
    int st = CheckSeamSystem(AtA_dev, Atb_dev, residual_dev, n_vars, n_frags);
    if (st) return st;
    O3DMI_REQUIRE(n >= 0, "negative count");
    O3DMI_REQUIRE(i >= 0 && j >= 0 && i < n_frags && j < n_frags,
                  "node id out of range");
    O3DMI_REQUIRE(i != j, "an edge joins two different nodes");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(Ti_Cps_dev && Tj_Cqs_dev && Cnormal_ps_dev &&
                          Ri_Cnormal_ps_dev && RjT_Ri_Cnormal_ps_dev &&
                          cgrid_idx_ps_dev && cgrid_idx_qs_dev &&
                          cgrid_ratio_ps_dev && cgrid_ratio_qs_dev,
                  "null argument");
    const int64_t tiles = SlacTiles(n);
    O3DMI_REQUIRE(tiles < (1ll << 31), "slac: too many correspondences");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    SeamSystem seam;
    double* partials = nullptr;
    SlacEdge* edge_dev = nullptr;
    if ((st = seam.Make(sc, n_vars, n_frags, s)) ||
        (st = sc.Alloc(&partials, sizeof(double) * kSlacSums * (size_t)tiles)) ||
        (st = sc.Alloc(&edge_dev, sizeof(SlacEdge))))
        return st;
    SlacEdge ed{};
    ed.count = n;
    ed.tile_first = 0;
    ed.i = i;
    ed.j = j;
    O3DMI_HIP_CHECK(hipMemcpyAsync(edge_dev, &ed, sizeof(ed),
                                   hipMemcpyHostToDevice, s));
    if ((st = SlacNonrigidSeamTermsAsync(
                 Ti_Cps_dev, Tj_Cqs_dev, Cnormal_ps_dev, Ri_Cnormal_ps_dev,
                 RjT_Ri_Cnormal_ps_dev, cgrid_idx_ps_dev, cgrid_idx_qs_dev,
                 cgrid_ratio_ps_dev, cgrid_ratio_qs_dev, n, threshold, i, j,
                 seam.sys, partials, s)) ||
        (st = SlacEdgeSumsAsync(partials, edge_dev, 1, tiles,
                                seam.sys.counters, seam.tail, s)) ||
        (st = SlacPoseBlocksAsync(seam.tail, edge_dev, 1, seam.sys, s)) ||
        (st = SlacSeamFinishAsync(seam.sys, seam.tail + 27, AtA_dev, Atb_dev,
                                  residual_dev, s)))
        return st;
    return seam.Finish(s);
}

extern "C" int o3dmi_fill_in_slac_regularizer_term(
        float* AtA_dev, float* Atb_dev, float* residual_dev, int64_t n_vars,
        const int32_t* grid_idx_dev, const int32_t* grid_nbs_idx_dev,
        const uint8_t* grid_nbs_mask_dev, int64_t n,
        const float* positions_init_dev, const float* positions_curr_dev,
        int64_t n_positions, float weight, int n_frags, int anchor_idx,
        o3dmi_stream_t stream) {
    int st = CheckSeamSystem(AtA_dev, Atb_dev, residual_dev, n_vars, n_frags);
    if (st) return st;
    O3DMI_REQUIRE(n >= 0 && n_positions >= 0, "negative count");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(grid_idx_dev && grid_nbs_idx_dev && grid_nbs_mask_dev &&
                          positions_init_dev && positions_curr_dev,
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    SeamSystem seam;
    double* node_residual = nullptr;
    if ((st = seam.Make(sc, n_vars, n_frags, s)) ||
        (st = sc.Alloc(&node_residual, sizeof(double) * (size_t)n)))
        return st;
    if ((st = SlacSeamIndexCheckAsync(grid_idx_dev, n, nullptr, seam.sys,
                                      s)) ||
        (st = SlacSeamIndexCheckAsync(grid_nbs_idx_dev, 6 * n,
                                      grid_nbs_mask_dev, seam.sys, s)) ||
        (st = SlacRegularizerAsync(grid_idx_dev, grid_nbs_idx_dev,
                                   grid_nbs_mask_dev, n, positions_init_dev,
                                   positions_curr_dev, nullptr, n_positions,
                                   weight, anchor_idx, seam.sys, node_residual,
                                   seam.tail + kSlacSums, s)) ||
        (st = SlacSeamFinishAsync(seam.sys, seam.tail + kSlacSums, AtA_dev,
                                  Atb_dev, residual_dev, s)))
        return st;
    return seam.Finish(s);
}

extern "C" int o3dmi_slac_solve_spd(double* A_dev, double* b_dev, int64_t n,
                                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n > 0, "empty system");
    if (n > kSlacMaxVars) {
        SetLastError("slac: more than 32768 unknowns are not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    O3DMI_REQUIRE(A_dev && b_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    int* flag = nullptr;
    int st = sc.Alloc(&flag, sizeof(int));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), s));
    if ((st = SlacSolveSpdAsync(A_dev, b_dev, n, flag, s))) return st;
    int h = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&h, flag, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (h) {
        SetLastError("slac: the system is not positive definite");
        return O3DMI_ERR_SINGULAR;
    }
    return O3DMI_OK;
}

extern "C" int o3dmi_slac_optimize(
        const void* const* positions_dev, const void* const* normals_dev,
        const int64_t* sizes, int n_nodes, double* poses, const int32_t* edges,
        const double* T_ij, int n_edges, o3dmi_control_grid_t* grid,
        int max_iterations, float distance_threshold, float fitness_threshold,
        float regularizer_weight, double* alignment_losses,
        double* regularizer_losses, int32_t* kept, int64_t* n_corres,
        int64_t* n_inliers, int64_t* skipped, o3dmi_stream_t stream) {
    int st = CheckPoseGraph(positions_dev, normals_dev, sizes, n_nodes, poses,
                            edges, T_ij, n_edges);
    if (st) return st;
    O3DMI_REQUIRE(grid != nullptr, "control grid is null");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    if (skipped) *skipped = 0;

    // ---- InitializeControlGrid + Compactify for an empty grid --------------
    int64_t G = 0;
    if ((st = o3dmi_control_grid_size(grid, stream, &G))) return st;
    if (G == 0) {
        for (int k = 0; k < n_nodes; ++k)
            if ((st = o3dmi_control_grid_touch(
                         grid, (const float*)positions_dev[k], sizes[k],
                         stream)))
                return st;
        if ((st = o3dmi_control_grid_compactify(grid, stream)) ||
            (st = o3dmi_control_grid_size(grid, stream, &G)))
            return st;
    }
    const int64_t n = 6 * (int64_t)n_nodes + 3 * G;
    if (n > kSlacMaxVars) {
        SetLastError("slac: more than 32768 unknowns are not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    o3dmi_hash_t* hash = o3dmi_control_grid_hashmap(grid);
    const int64_t cap = hash->capacity;
    const float grid_size = o3dmi_control_grid_grid_size(grid);
    const int anchor = o3dmi_control_grid_anchor_idx(grid);
    float* curr = o3dmi_control_grid_curr_positions(grid);

    int32_t *active = nullptr, *nb_idx = nullptr, *rank = nullptr;
    uint8_t* nb_mask = nullptr;
    float *init = nullptr, *backup = nullptr;
    const size_t ucap = (size_t)std::max<int64_t>(cap, 1);
    if ((st = sc.Alloc(&active, 4 * ucap)) ||
        (st = sc.Alloc(&nb_idx, 24 * ucap)) ||
        (st = sc.Alloc(&nb_mask, 6 * ucap)) ||
        (st = sc.Alloc(&rank, 4 * ucap)) || (st = sc.Alloc(&init, 12 * ucap)) ||
        (st = sc.Alloc(&backup, 12 * ucap)))
        return st;
    int64_t G_map = 0;
    if ((st = o3dmi_control_grid_neighbor_grid_map(grid, active, nb_idx,
                                                   nb_mask, &G_map, stream)) ||
        (st = o3dmi_control_grid_init_positions(grid, init, stream)) ||
        (st = SlacRankTableAsync(active, G_map, (int)cap, rank, s)))
        return st;
    if (G_map != G) {
        SetLastError("slac: the control grid changed during the call");
        return O3DMI_ERR_INTERNAL;
    }
    O3DMI_HIP_CHECK(hipMemcpyAsync(backup, curr, 12 * (size_t)cap,
                                   hipMemcpyDeviceToDevice, s));
    // the node that holds the gauge (see the header): Compactify's anchor
    int pinned_rank = -1;
    if (anchor >= 0 && anchor < cap) {
        O3DMI_HIP_CHECK(hipMemcpyAsync(&pinned_rank, rank + anchor,
                                       sizeof(int), hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    }
    O3DMI_REQUIRE(G == 0 || pinned_rank >= 0,
                  "slac: the control grid has no anchor node (compactify it)");

    // ---- correspondence sets, once, from the input graph -------------------
    std::vector<SlacEdge> ed;
    if ((st = SlacCorrespondenceSets(positions_dev, sizes, poses, edges, T_ij,
                                     n_edges, distance_threshold,
                                     fitness_threshold, sc, ed, kept, n_corres,
                                     n_inliers, stream)))
        return st;
    if (max_iterations <= 0) return O3DMI_OK;

    // ---- the embedding of every fragment, once: only the nodes move --------
    std::vector<SlacGridFragment> frags((size_t)n_nodes);
    for (int k = 0; k < n_nodes; ++k) {
        int32_t* corners = nullptr;
        if ((st = sc.Alloc(&corners, 32 * (size_t)sizes[k])) ||
            (st = SlacGridCornersAsync(hash->view,
                                       (const float*)positions_dev[k],
                                       sizes[k], grid_size, corners, s)))
            return st;
        frags[k] = {(const float*)positions_dev[k],
                    (const float*)normals_dev[k], corners, sizes[k]};
    }
    const int64_t n_tiles = SlacLayoutTiles(ed.data(), n_edges);
    SlacGridFragment* frags_dev = nullptr;
    SlacEdge* edges_dev = nullptr;
    double *partials = nullptr, *tail = nullptr, *node_residual = nullptr;
    SlacSystem sys{};
    sys.n = n;
    sys.n_frags = n_nodes;
    const size_t n_sums = (size_t)n_edges * kSlacSums;
    if ((st = sc.Alloc(&frags_dev, sizeof(SlacGridFragment) * frags.size())) ||
        (st = sc.Alloc(&edges_dev,
                       sizeof(SlacEdge) * std::max<size_t>(ed.size(), 1))) ||
        (st = sc.Alloc(&partials, sizeof(double) * kSlacSums *
                                          (size_t)std::max<int64_t>(n_tiles,
                                                                    1))) ||
        (st = sc.Alloc(&tail, sizeof(double) * (n_sums + 1))) ||
        (st = sc.Alloc(&node_residual,
                       sizeof(double) * (size_t)std::max<int64_t>(G, 1))) ||
        (st = sc.Alloc(&sys.AtA, sizeof(double) * (size_t)n * (size_t)n)) ||
        (st = sc.Alloc(&sys.Atb, sizeof(double) * (size_t)n)) ||
        (st = sc.Alloc(&sys.counters, 3 * sizeof(int))))  // bad, skipped, flag
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(frags_dev, frags.data(),
                                   sizeof(SlacGridFragment) * frags.size(),
                                   hipMemcpyHostToDevice, s));

    auto fail = [&](int code, const char* msg) {
        SetLastError(msg);
        return code;
    };
    std::vector<double> T(poses, poses + 16 * (size_t)n_nodes);
    std::vector<double> h(n_sums + 1), x((size_t)n);
    std::vector<double> align((size_t)max_iterations, 0.0),
            reg((size_t)max_iterations, 0.0);
    const float weight = (float)n_nodes * regularizer_weight;
    // every exit of an iteration goes through the restore below
    auto iterate = [&](int it) -> int {
        for (int e = 0; e < n_edges; ++e) {
            Pose12(&T[16 * (size_t)ed[e].i], ed[e].Ti);
            Pose12(&T[16 * (size_t)ed[e].j], ed[e].Tj);
        }
        if (n_edges > 0)
            O3DMI_HIP_CHECK(hipMemcpyAsync(edges_dev, ed.data(),
                                           sizeof(SlacEdge) * ed.size(),
                                           hipMemcpyHostToDevice, s));
        // SLACOptimizer.cpp:331-339: zeros, ones on the first six diagonals
        O3DMI_HIP_CHECK(hipMemsetAsync(
                sys.AtA, 0, sizeof(double) * (size_t)n * (size_t)n, s));
        O3DMI_HIP_CHECK(hipMemsetAsync(sys.Atb, 0, sizeof(double) * (size_t)n,
                                       s));
        O3DMI_HIP_CHECK(hipMemsetAsync(tail, 0, sizeof(double) * (n_sums + 1),
                                       s));
        O3DMI_HIP_CHECK(hipMemsetAsync(sys.counters, 0, 3 * sizeof(int), s));
        if ((st = SlacPrepareSystemAsync(sys, s)) ||
            (st = SlacNonrigidTermsAsync(frags_dev, edges_dev, n_edges,
                                         n_tiles, curr, rank, (int)cap,
                                         grid_size, distance_threshold, sys,
                                         partials, s)) ||
            (st = SlacEdgeSumsAsync(partials, edges_dev, n_edges, n_tiles,
                                    sys.counters, tail, s)) ||
            (st = SlacPoseBlocksAsync(tail, edges_dev, n_edges, sys, s)) ||
            (st = SlacRegularizerAsync(active, nb_idx, nb_mask, G, init, curr,
                                       rank, cap, weight, anchor, sys,
                                       node_residual, tail + n_sums, s)) ||
            (G > 0 && (st = SlacPinNodeAsync(
                               sys, 6 * (int64_t)n_nodes + 3 * pinned_rank,
                               s))) ||
            // delta = AtA.Solve(Atb.Neg())
            (st = SlacNegateAsync(sys.Atb, n, s)) ||
            (st = SlacSolveSpdAsync(sys.AtA, sys.Atb, n, sys.counters + 2, s)))
            return st;
        int counters[3] = {0, 0, 0};
        O3DMI_HIP_CHECK(hipMemcpyAsync(h.data(), tail,
                                       sizeof(double) * (n_sums + 1),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipMemcpyAsync(x.data(), sys.Atb,
                                       sizeof(double) * (size_t)n,
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipMemcpyAsync(counters, sys.counters,
                                       sizeof(counters),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        if (counters[0])
            return fail(O3DMI_ERR_INTERNAL,
                        "slac: correspondence or node index out of range");
        if (counters[2])
            return fail(O3DMI_ERR_SINGULAR, "slac: singular linear system");
        for (int e = 0; e < n_edges; ++e) {
            align[it] += h[(size_t)e * kSlacSums + 27];
            if (n_inliers) n_inliers[e] = (int64_t)h[(size_t)e * kSlacSums + 28];
        }
        reg[it] = h[n_sums];
        if (skipped) *skipped = counters[1];
        for (int64_t k = 0; k < n; ++k)
            if (!std::isfinite(x[(size_t)k]))
                return fail(O3DMI_ERR_SINGULAR,
                            "slac: singular linear system");
        SlacUpdatePoses(x.data(), n_nodes, T.data());
        // UpdateControlGrid, SLACOptimizer.cpp:288-295
        if ((st = SlacUpdateGridAsync(active, G, sys.Atb + 6 * n_nodes, curr,
                                      s)))
            return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    };
    for (int it = 0; it < max_iterations; ++it) {
        if ((st = iterate(it))) {
            // poses were never written; the nodes go back to what they were
            (void)hipMemcpyAsync(curr, backup, 12 * (size_t)cap,
                                 hipMemcpyDeviceToDevice, s);
            (void)hipStreamSynchronize(s);
            return st;
        }
    }
    std::copy(T.begin(), T.end(), poses);
    if (alignment_losses)
        std::copy(align.begin(), align.end(), alignment_losses);
    if (regularizer_losses)
        std::copy(reg.begin(), reg.end(), regularizer_losses);
    return O3DMI_OK;
}
