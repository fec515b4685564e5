// Multiway alignment terms: the tables the kernels of slac.hip (rigid) and
// slac_nonrigid.hip (control grid, regularizer, SPD solve) read and the
// stream-ordered launchers host/slac.cpp and host/slac_nonrigid.cpp drive.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace o3dmi {

// 21 lower-triangle J J^T sums (sums[j (j + 1) / 2 + k] = A[j][k]), 6 J r
// sums, sum r r, count.
constexpr int kSlacSums = 29;
constexpr int kSlacBlock = 256;
constexpr int kSlacItems = 4;  // correspondences per lane
constexpr int kSlacTile = kSlacBlock * kSlacItems;

inline int64_t SlacTiles(int64_t n) {
    return n > 0 ? (n + kSlacTile - 1) / kSlacTile : 0;
}

struct SlacFragment {
    const float* positions;  // {n,3}
    const float* normals;    // {n,3}
    int64_t n;
};

// One pose-graph edge (i, j) of an iteration. Its tiles are
// [tile_first, tile_first + SlacTiles(count)) of the launch.
struct SlacEdge {
    const int64_t* corres;  // {count,2}: (index in i, index in j)
    int64_t count;
    int64_t tile_first;
    int32_t i, j;
    float Ti[12];  // rows 0..2 of the node poses, rounded to float32
    float Tj[12];
};

// Fills the per-iteration fields of edges_host (tile_first) and returns the
// number of tiles of the launch.
int64_t SlacLayoutTiles(SlacEdge* edges_host, int n_edges);

// Uploads nothing: frags_dev / edges_dev are device tables. Queues
// RigidTermsKernel over all tiles and the per-edge final pass. partials_dev:
// n_tiles x kSlacSums float64. *bad_dev (zeroed by the caller) is set when a
// correspondence index is out of range; sums_dev {E,29} is then not written.
int SlacRigidTermsAsync(const SlacFragment* frags_dev,
                        const SlacEdge* edges_dev, int n_edges,
                        int64_t n_tiles, float threshold, double* partials_dev,
                        int* bad_dev, double* sums_dev, hipStream_t s);

// The per-edge final pass alone: sums_dev[e] = the rows of edge e's tiles added
// in row order (one workgroup per edge); nothing is written when *bad_dev.
int SlacEdgeSumsAsync(const double* partials_dev, const SlacEdge* edges_dev,
                      int n_edges, int64_t n_tiles, const int* bad_dev,
                      double* sums_dev, hipStream_t s);

// {a, idx[a]} for every a with idx[a] != -1 at row position[a] of corres_dev,
// and the number of those pairs with |Ti p_a - Tj q_b|^2 <= d2 added to
// *inliers_dev (zeroed by the caller). Ti / Tj: 12 floats each.
int SlacCorrespondenceSetAsync(const int32_t* idx_dev,
                               const int64_t* position_dev, int64_t n_i,
                               int64_t n_j, const float* positions_i_dev,
                               const float* positions_j_dev, const float* Ti,
                               const float* Tj, float d2, int64_t* corres_dev,
                               unsigned long long* inliers_dev, int* bad_dev,
                               hipStream_t s);

// ---- the non-rigid optimizer (slac_nonrigid.hip) ---------------------------
// Unknowns: 6 per fragment, then 3 per active control node in the order of the
// node's rank in the ascending active buffer-index list. The system is a dense
// lower-triangular float64 {n,n} matrix (row-major, only c <= r is written or
// read) and a float64 {n} right-hand side.

constexpr int kSlacMaxVars = 32768;  // 8.6 GB of float64
// panel width of the blocked Cholesky; the panel kernel holds panel x 256
// doubles of LDS (64 KB at 32), see the static_assert in slac_nonrigid.hip
constexpr int kSlacCholPanel = 32;
constexpr int kSlacCholTile = 64;    // trailing-update tile (rows = columns)

// rank_dev[capacity]: rank of a buffer index in active_dev[0..G), or -1.
int SlacRankTableAsync(const int32_t* active_dev, int64_t G, int capacity,
                       int32_t* rank_dev, hipStream_t s);

// corners_dev {n,8} int32: the buffer indices of the eight corner nodes of
// every point's cell in ControlGrid's corner order; row[0] = -1 when the cell
// has an inactive corner (or the point cannot be a key).
int SlacGridCornersAsync(const HashView& hv, const float* points_dev,
                         int64_t n, float grid_size, int32_t* corners_dev,
                         hipStream_t s);

// The per-fragment inputs of the one-launch alignment kernel.
struct SlacGridFragment {
    const float* positions;  // {n,3}
    const float* normals;    // {n,3}
    const int32_t* corners;  // {n,8}, SlacGridCornersAsync
    int64_t n;
};

// The system of one call. counters_dev[0]: bad index flag, [1]: pairs skipped
// for an inactive corner.
struct SlacSystem {
    double* AtA;  // {n,n} lower
    double* Atb;  // {n}
    int64_t n;
    int n_frags;
    int* counters;
};

// Alignment terms of all edges in one launch: embeds, deforms (curr_dev: the
// grid's value buffer), transforms, and adds the grid-grid / pose-grid / grid
// rhs entries to `sys` with float64 atomics. The 29 pose sums of every
// (edge, tile) go to partials_dev {n_tiles,29} (reduce with SlacEdgeSumsAsync,
// scatter with SlacPoseBlocksAsync).
int SlacNonrigidTermsAsync(const SlacGridFragment* frags_dev,
                           const SlacEdge* edges_dev, int n_edges,
                           int64_t n_tiles, const float* curr_dev,
                           const int32_t* rank_dev, int capacity,
                           float grid_size, float threshold, SlacSystem sys,
                           double* partials_dev, hipStream_t s);

// The pose-pose blocks of all edges, [[A, -A], [-A, A]] and [b, -b] from
// sums_dev {E,29}, added to the lower triangle in edge order by one workgroup
// (run-to-run identical). Nothing is written when counters[0].
int SlacPoseBlocksAsync(const double* sums_dev, const SlacEdge* edges_dev,
                        int n_edges, SlacSystem sys, hipStream_t s);

// The reference's alignment seam into `sys` (raw cgrid indices: rank = idx).
// partials_dev: SlacTiles(count) x 29. A node index with
// 6 n_frags + 3 idx + 2 >= n sets counters[0].
int SlacNonrigidSeamTermsAsync(const float* Ti_Cps, const float* Tj_Cqs,
                               const float* Cnormal_ps,
                               const float* Ri_Cnormal_ps,
                               const float* RjT_Ri_Cnormal_ps,
                               const int32_t* idx_ps, const int32_t* idx_qs,
                               const float* ratio_ps, const float* ratio_qs,
                               int64_t count, float threshold, int i, int j,
                               SlacSystem sys, double* partials_dev,
                               hipStream_t s);

// counters[0] is set when a listed raw node index (mask_dev null: all of
// them) is negative or has 6 n_frags + 3 idx + 2 >= n.
int SlacSeamIndexCheckAsync(const int32_t* idx_dev, int64_t n_idx,
                            const uint8_t* mask_dev, SlacSystem sys,
                            hipStream_t s);

// Regularizer: one lane per listed node. rank_dev null: rank = buffer index
// (the seam). node_residual_dev {G} receives every node's weighted residual;
// residual_dev[0] their sum in a fixed order.
int SlacRegularizerAsync(const int32_t* active_dev, const int32_t* nb_idx_dev,
                         const uint8_t* nb_mask_dev, int64_t G,
                         const float* init_dev, const float* curr_dev,
                         const int32_t* rank_dev, int64_t n_rows, float weight,
                         int anchor_idx, SlacSystem sys,
                         double* node_residual_dev, double* residual_dev,
                         hipStream_t s);

// out[r][c] += (float)sys[max][min], out_b += (float)b, out_res += (float)res
// (pose sums row 27 / the regularizer's residual): the float32 seams' tail.
// Entries whose sum is 0 are left alone; nothing is written when counters[0].
int SlacSeamFinishAsync(SlacSystem sys, const double* residual_dev,
                        float* AtA_out, float* Atb_out, float* residual_out,
                        hipStream_t s);

// Blocked right-looking Cholesky of the lower triangle in place and the two
// triangular solves of b in place. *flag_dev (zeroed by the caller) is set on
// a pivot that is <= 0 or not finite; later launches then do nothing.
int SlacSolveSpdAsync(double* A_dev, double* b_dev, int64_t n, int* flag_dev,
                      hipStream_t s);

// x <- -x for n entries; first six diagonal entries of the system <- 1.
int SlacPrepareSystemAsync(SlacSystem sys, hipStream_t s);
int SlacNegateAsync(double* x_dev, int64_t n, hipStream_t s);

// The three unknowns row0 .. row0 + 2 are taken out of the system (identity
// rows and columns, rhs 0). The reference's system has a three-dimensional
// null space: moving every node by t and translating fragment k >= 1 by
// (R_0 - R_k) t changes no term, and the ones on the first six diagonals only
// hold fragment 0. Holding one node selects one of its solutions.
int SlacPinNodeAsync(SlacSystem sys, int64_t row0, hipStream_t s);

// curr[active[g]] += (float)x[3 g + a].
int SlacUpdateGridAsync(const int32_t* active_dev, int64_t G,
                        const double* x_dev, float* curr_dev, hipStream_t s);

}  // namespace o3dmi
