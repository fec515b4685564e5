// RunRigidOptimizerForFragments and GetCorrespondenceSetForPointCloudPair
// (t/pipelines/slac/SLACOptimizer.cpp:85-204,265-286,369-414) over the kernels
// of slac.hip, for fragments in device memory.
//
// An iteration is two launches (terms of every edge, per-edge final pass), one
// upload of the edge table (the poses moved) and one download of E x 29
// doubles; the 6N x 6N system is assembled and solved on the host in float64.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.h"
#include "host/host_util.h"
#include "o3d_mi355x_host.h"
#include "scan.h"
#include "slac.h"
#include "host/slac_common.h"

using namespace o3dmi;

namespace {

// x = solve(A, b) for the n x n row-major A (overwritten) by LU with partial
// pivoting; false on a zero or non-finite pivot.
bool SolveLU(std::vector<double>& A, std::vector<double>& b, int n) {
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double best = std::fabs(A[(size_t)k * n + k]);
        for (int r = k + 1; r < n; ++r) {
            const double v = std::fabs(A[(size_t)r * n + k]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (!(best > 0) || !std::isfinite(best)) return false;
        if (piv != k) {
            std::swap_ranges(A.begin() + (size_t)k * n,
                             A.begin() + (size_t)(k + 1) * n,
                             A.begin() + (size_t)piv * n);
            std::swap(b[k], b[piv]);
        }
        const double* rk = &A[(size_t)k * n];
        const double d = rk[k];
        for (int r = k + 1; r < n; ++r) {
            double* rr = &A[(size_t)r * n];
            const double l = rr[k] / d;
            if (l == 0) continue;
            rr[k] = l;
            for (int c = k + 1; c < n; ++c) rr[c] -= l * rk[c];
            b[r] -= l * b[k];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        const double* rk = &A[(size_t)k * n];
        double v = b[k];
        for (int c = k + 1; c < n; ++c) v -= rk[c] * b[c];
        b[k] = v / rk[k];
        if (!std::isfinite(b[k])) return false;
    }
    return true;
}

}  // namespace

extern "C" int o3dmi_slac_correspondence_set(
        const void* positions_i_dev, int64_t ni, const void* positions_j_dev,
        int64_t nj, int i, int j, const double* T_i, const double* T_j,
        const double* T_ij, float distance_threshold, float fitness_threshold,
        int64_t* corres_dev, int64_t* n_corres, int64_t* n_inliers,
        float* inlier_ratio, int* kept, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(T_i && T_j && T_ij && n_corres && n_inliers &&
                          inlier_ratio && kept,
                  "null argument");
    O3DMI_REQUIRE(ni > 0 && nj > 0 && positions_i_dev && positions_j_dev &&
                          corres_dev,
                  "empty fragment");
    O3DMI_REQUIRE(ni < (1ll << 31), "fragment too large");
    O3DMI_REQUIRE(distance_threshold > 0, "distance_threshold must be > 0");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    NnsGuard index;
    float* moved = nullptr;
    int32_t* idx = nullptr;
    float* dist2 = nullptr;
    int32_t* counts = nullptr;
    int64_t* position = nullptr;
    void* scan_tmp = nullptr;
    int64_t* head = nullptr;  // {C, inliers, bad}
    int st;
    if ((st = sc.Alloc(&moved, 12 * (size_t)ni)) ||
        (st = sc.Alloc(&idx, 4 * (size_t)ni)) ||
        (st = sc.Alloc(&dist2, 4 * (size_t)ni)) ||
        (st = sc.Alloc(&counts, 4 * (size_t)ni)) ||
        (st = sc.Alloc(&position, 8 * (size_t)ni)) ||
        (st = sc.Alloc(&scan_tmp, ScanScratchBytes(ni))) ||
        (st = sc.Alloc(&head, 3 * sizeof(int64_t))))
        return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(head, 0, 3 * sizeof(int64_t), s));
    // tpcd_i.Clone().Transform(T_ij), HybridIndex(d), HybridSearch(.., d, 1)
    O3DMI_HIP_CHECK(hipMemcpyAsync(moved, positions_i_dev, 12 * (size_t)ni,
                                   hipMemcpyDeviceToDevice, s));
    if ((st = o3dmi_transform_points(T_ij, moved, ni, O3DMI_F32, stream)) ||
        (st = o3dmi_nns_create(positions_j_dev, nj, O3DMI_F32,
                               (double)distance_threshold, stream,
                               &index.nns)) ||
        (st = o3dmi_nns_hybrid_search_k1(index.nns, moved, ni, idx, dist2,
                                         counts, stream)) ||
        // counts = 1 where a neighbour was found: the ordered compaction
        (st = PrefixSumAsync(counts, ni, false, position, head, scan_tmp, s)))
        return st;
    float ti[12], tj[12];
    Pose12(T_i, ti);
    Pose12(T_j, tj);
    if ((st = SlacCorrespondenceSetAsync(
                 idx, position, ni, nj, (const float*)positions_i_dev,
                 (const float*)positions_j_dev, ti, tj,
                 distance_threshold * distance_threshold, corres_dev,
                 (unsigned long long*)(head + 1), (int*)(head + 2), s)))
        return st;
    int64_t h[3] = {0, 0, 0};
    O3DMI_HIP_CHECK(hipMemcpyAsync(h, head, sizeof(h), hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (h[2] != 0) {
        SetLastError("slac: neighbour index out of range");
        return O3DMI_ERR_INTERNAL;
    }
    *n_corres = h[0];
    *n_inliers = h[1];
    // SLACOptimizer.cpp:188-194
    const float ratio = static_cast<float>(h[1]) / static_cast<float>(h[0]);
    *inlier_ratio = ratio;
    *kept = !((j != i + 1 && ratio < fitness_threshold) || h[0] == 0);
    return O3DMI_OK;
}

extern "C" int o3dmi_slac_rigid_optimize(
        const void* const* positions_dev, const void* const* normals_dev,
        const int64_t* sizes, int n_nodes, double* poses, const int32_t* edges,
        const double* T_ij, int n_edges, int max_iterations,
        float distance_threshold, float fitness_threshold, double* losses,
        int32_t* kept, int64_t* n_corres, int64_t* n_inliers,
        o3dmi_stream_t stream) {
    int st = CheckPoseGraph(positions_dev, normals_dev, sizes, n_nodes, poses,
                            edges, T_ij, n_edges);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);

    // ---- correspondence sets, once, from the input graph -------------------
    std::vector<SlacEdge> ed;
    if ((st = SlacCorrespondenceSets(positions_dev, sizes, poses, edges, T_ij,
                                     n_edges, distance_threshold,
                                     fitness_threshold, sc, ed, kept, n_corres,
                                     n_inliers, stream)))
        return st;
    if (max_iterations <= 0) return O3DMI_OK;

    const int64_t n_tiles = SlacLayoutTiles(ed.data(), n_edges);
    std::vector<SlacFragment> frags((size_t)n_nodes);
    for (int k = 0; k < n_nodes; ++k)
        frags[k] = {(const float*)positions_dev[k],
                    (const float*)normals_dev[k], sizes[k]};
    SlacFragment* frags_dev = nullptr;
    SlacEdge* edges_dev = nullptr;
    double* partials = nullptr;
    double* block = nullptr;  // [E x 29 sums | bad flag]
    const size_t n_sums = (size_t)n_edges * kSlacSums;
    if ((st = sc.Alloc(&frags_dev, sizeof(SlacFragment) * frags.size())) ||
        (st = sc.Alloc(&edges_dev,
                       sizeof(SlacEdge) * std::max<size_t>(ed.size(), 1))) ||
        (st = sc.Alloc(&partials, sizeof(double) * kSlacSums *
                                          (size_t)std::max<int64_t>(n_tiles,
                                                                    1))) ||
        (st = sc.Alloc(&block, sizeof(double) * (n_sums + 1))))
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(frags_dev, frags.data(),
                                   sizeof(SlacFragment) * frags.size(),
                                   hipMemcpyHostToDevice, s));

    const int n = 6 * n_nodes;
    std::vector<double> T((size_t)16 * n_nodes);
    std::copy(poses, poses + 16 * (size_t)n_nodes, T.begin());
    std::vector<double> h(n_sums + 1), AtA, rhs((size_t)n);
    std::vector<double> loss((size_t)max_iterations, 0.0);
    for (int it = 0; it < max_iterations; ++it) {
        for (int e = 0; e < n_edges; ++e) {
            Pose12(&T[16 * (size_t)ed[e].i], ed[e].Ti);
            Pose12(&T[16 * (size_t)ed[e].j], ed[e].Tj);
        }
        O3DMI_HIP_CHECK(hipMemsetAsync(block, 0,
                                       sizeof(double) * (n_sums + 1), s));
        if (n_edges > 0) {
            O3DMI_HIP_CHECK(hipMemcpyAsync(edges_dev, ed.data(),
                                           sizeof(SlacEdge) * ed.size(),
                                           hipMemcpyHostToDevice, s));
            if ((st = SlacRigidTermsAsync(frags_dev, edges_dev, n_edges,
                                          n_tiles, distance_threshold,
                                          partials, (int*)(block + n_sums),
                                          block, s)))
                return st;
        }
        O3DMI_HIP_CHECK(hipMemcpyAsync(h.data(), block,
                                       sizeof(double) * (n_sums + 1),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        int bad = 0;
        std::memcpy(&bad, &h[n_sums], sizeof(int));
        if (bad) {
            SetLastError("slac: correspondence index out of range");
            return O3DMI_ERR_INTERNAL;
        }
        // SLACOptimizer.cpp:394-409: zeros, 1e5 on node 0, the edges' blocks
        AtA.assign((size_t)n * n, 0.0);
        std::fill(rhs.begin(), rhs.end(), 0.0);
        for (int k = 0; k < 6; ++k) AtA[(size_t)k * n + k] = 1e5;
        double residual = 0;
        for (int e = 0; e < n_edges; ++e) {
            const double* S = &h[(size_t)e * kSlacSums];
            const int bi = 6 * ed[e].i, bj = 6 * ed[e].j;
            for (int u = 0; u < 6; ++u) {
                for (int v = 0; v < 6; ++v) {
                    const double a = u >= v ? S[u * (u + 1) / 2 + v]
                                            : S[v * (v + 1) / 2 + u];
                    AtA[(size_t)(bi + u) * n + bi + v] += a;
                    AtA[(size_t)(bj + u) * n + bj + v] += a;
                    AtA[(size_t)(bi + u) * n + bj + v] -= a;
                    AtA[(size_t)(bj + u) * n + bi + v] -= a;
                }
                // x = solve(AtA, -Atb)
                rhs[bi + u] -= S[21 + u];
                rhs[bj + u] += S[21 + u];
            }
            residual += S[27];
            if (n_inliers) n_inliers[e] = (int64_t)S[28];
        }
        loss[it] = residual;
        if (!SolveLU(AtA, rhs, n)) {
            SetLastError("slac: singular linear system");
            return O3DMI_ERR_SINGULAR;
        }
        SlacUpdatePoses(rhs.data(), n_nodes, T.data());
    }
    std::copy(T.begin(), T.end(), poses);
    if (losses) std::copy(loss.begin(), loss.end(), losses);
    return O3DMI_OK;
}
