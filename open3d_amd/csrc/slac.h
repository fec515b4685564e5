// Rigid multiway alignment terms (slac.hip): the tables RigidTermsKernel reads
// and the stream-ordered launchers host/slac.cpp drives.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

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

}  // namespace o3dmi
