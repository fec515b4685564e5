// Private seam between the kernels of the oriented bounding boxes and the
// bounding ellipsoid (bounding_volume.hip) and their C ABI in
// host/bounding_volume.cpp (docs/bounding_volumes.md). Everything runs on the
// canonical convex hull (pointcloud_hull.h) with its V vertices widened to
// float64 and its T Int32 triangles. Every launcher is stream-ordered and waits
// for nothing; atomics are integer only; all arithmetic is float64, evaluated
// as written (-ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "common.h"

namespace o3dmi {

// ---- the fixed tree of every sum ------------------------------------------------
// Runs of kBvRun consecutive values are added in index order starting from
// 0.0, the run sums likewise, level by level until one value is left. A short
// last run adds what it has (adding 0.0 changes no bit, so padding with zeros
// is the same tree).
constexpr int kBvRun = 8;
// A workgroup of kBvBlock lanes, one run of vertices per lane, sums
// kBvBlock * kBvRun = kBvRun^4 consecutive vertices: four whole levels of the
// tree, whatever V is.
constexpr int kBvBlock = 512;
constexpr int kBvBlockVertices = kBvBlock * kBvRun;
static_assert(kBvBlockVertices == kBvRun * kBvRun * kBvRun * kBvRun,
              "a workgroup's slice is a node of the tree");
constexpr int kBvSums = 11;  // the widest row of sums (Khachiyan's)

// ---- (a) MINIMAL_APPROX ----------------------------------------------------------
constexpr int kObbBlock = kBlock;  // lane = one triangle
constexpr int kObbTile = 512;      // hull vertices per LDS tile
constexpr int kObbMaxSplit = 64;   // most vertex slices per triangle

// What the choice leaves on the device (all doubles): the winning candidate
// index (-1 = the axis-aligned box), its minima and maxima, volume, the box.
struct ObbResult {
    double winner;
    double lo[3], hi[3];
    double volume;
    double center[3];
    double rotation[9];  // row-major, columns u v w
    double extent[3];
};

// Scratch doubles of ObbApproxAsync for T triangles over `split` slices.
size_t ObbApproxScratchDoubles(int64_t n_tris, int split);

// The box of every hull triangle's frame over the V hull vertices X, the
// axis-aligned candidate, the smallest volume under a strict < in candidate
// order (NaN never wins) and the winner's box in *result_dev. split: vertex
// slices per triangle, 1 <= split <= kObbMaxSplit (min and max are exact, so
// every split gives the same bits). words_dev: 16 bytes, initialised here.
int ObbApproxAsync(const double* X_dev, int64_t n_verts, const int32_t* tri_dev,
                   int64_t n_tris, int split, double* scratch_dev,
                   unsigned long long* words_dev, ObbResult* result_dev,
                   hipStream_t s);

// ---- (b) PCA ---------------------------------------------------------------------
// Scratch doubles of the sums of V vertices (workgroup partials, two buffers).
size_t BvSumScratchDoubles(int64_t n_verts);

// sums_dev[0..9) = the sums of x, y, z, xx, xy, xz, yy, yz, zz over the hull
// vertices in the fixed tree. ticket_dev: one zeroed word, zero again after.
int BvMomentsAsync(const double* X_dev, int64_t n_verts, double* scratch_dev,
                   unsigned* ticket_dev, double* sums_dev, hipStream_t s);

// keys_dev[0..3) / [3..6) = the ordered bits (pointcloud_hull.hip's OrderedKey)
// of the minima / maxima of R^T (x - mean) over the hull vertices, each
// coordinate ((d.x r.x + d.y r.y) + d.z r.z) with r a column of the row-major
// R. keys_dev is initialised here.
int BvExtentsAsync(const double* X_dev, int64_t n_verts, const double mean[3],
                   const double rotation[9], unsigned long long* keys_dev,
                   hipStream_t s);

// The double whose ordered bits are k.
inline double FromOrderedKey(unsigned long long k) {
    const unsigned long long b =
            (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
}

// ---- (c) Khachiyan's loop --------------------------------------------------------
constexpr double kObeTolerance = 1e-6;  // upstream's eps (MinimumOBE.cpp:238)
constexpr int kObeMaxIterations = 1000; // upstream's maxiter (:239)
// Hull vertices the resident form holds: one workgroup, one run per lane.
constexpr int kObeResidentCapacity = kBvBlockVertices;

constexpr int kObeFormResident = 0;
constexpr int kObeFormStreamed = 1;

// The device word block of a loop (zeroed by the driver).
struct ObeWords {
    int done;        // the loop has ended: every later launch is a no-op
    int singular;    // a pivot <= 0 or a non-finite entry of Lambda
    int iterations;  // iterations completed
    int argmax;      // of the last M
    unsigned ticket[2];
    double step;     // of the last iteration
    double max_m;    // the last maximum of M
    double inv[16];  // Lambda^-1 of the iteration under way, row-major
    // x y z xx xy xz yy yz zz (weighted), the weights, the stop sum
    double sums[kBvSums];
};

// inv (row-major) = A^-1 for a symmetric positive definite A, of which the
// lower triangle is read: A = L D L^T in fixed order without pivoting, then
// column by column forward substitution, the division by D and backward
// substitution. False when a pivot is <= 0 or not finite.
template <int N>
__host__ __device__ inline bool LdltInverse(const double (&A)[N][N],
                                            double* inv) {
    double L[N][N], D[N];
    for (int j = 0; j < N; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= (L[j][k] * L[j][k]) * D[k];
        if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) return false;
        D[j] = d;
        for (int i = j + 1; i < N; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= (L[i][k] * L[j][k]) * D[k];
            L[i][j] = v / d;
        }
    }
    for (int c = 0; c < N; ++c) {
        double y[N], x[N];
        for (int i = 0; i < N; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
            y[i] = v;
        }
        for (int i = N - 1; i >= 0; --i) {
            double v = y[i] / D[i];
            for (int k = i + 1; k < N; ++k) v -= L[k][i] * x[k];
            x[i] = v;
        }
        for (int r = 0; r < N; ++r) inv[N * r + c] = x[r];
    }
    return true;
}

// Lambda^-1 from the ten sums {x, y, z, xx, xy, xz, yy, yz, zz, 1} weighted by
// p: Lambda = [[S, m], [m^T, w]] in the order (x, y, z, 1).
__host__ __device__ inline bool ObeInverse(const double* sums, double* inv) {
    const double A[4][4] = {{sums[3], sums[4], sums[5], sums[0]},
                            {sums[4], sums[6], sums[7], sums[1]},
                            {sums[5], sums[7], sums[8], sums[2]},
                            {sums[0], sums[1], sums[2], sums[9]}};
    return LdltInverse<4>(A, inv);
}

// Scratch doubles of the streamed form for V vertices: the weights, the
// workgroup partials of the sums (two buffers) and of the argmax.
size_t ObeStreamScratchDoubles(int64_t n_verts);

// The whole loop in one launch of one workgroup; n_verts <=
// kObeResidentCapacity. words_dev is zeroed by the caller.
int ObeResidentAsync(const double* X_dev, int64_t n_verts, ObeWords* words_dev,
                     hipStream_t s);

// weights = 1 / V, before the first streamed iteration.
int ObeStreamInitAsync(int64_t n_verts, double* scratch_dev, hipStream_t s);

// The two launches of streamed iteration `iteration` (0-based): the weight
// update of the iteration before with its stop value and the sums of Lambda
// (the last workgroup to arrive ends the loop or inverts Lambda), then M, its
// maximum and the step (the last arrival again). With words->done set both
// are no-ops. The driver queues one more sums launch after the last iteration.
int ObeStreamSumsAsync(const double* X_dev, int64_t n_verts, int iteration,
                       double* scratch_dev, ObeWords* words_dev, hipStream_t s);
int ObeStreamArgmaxAsync(const double* X_dev, int64_t n_verts,
                         double* scratch_dev, ObeWords* words_dev,
                         hipStream_t s);

}  // namespace o3dmi

// For tests and tools: the resident form's capacity, and what the last
// bounding-volume call of this thread did: stats = {hull vertices, hull
// triangles, iterations run, the form used (0 resident, 1 streamed, -1 none),
// the winner of MINIMAL_APPROX (-1 = the axis-aligned box; -2 none)},
// values = {the nine sums (PCA: of the vertices; ellipsoid: weighted),
// minima[3], maxima[3] of the box's frame, the last maximum of M}.
// o3dmi_pointcloud_oriented_bounding_box with MINIMAL_APPROX and the vertex
// slices of its mapping chosen, 1 <= split <= kObbMaxSplit (the public call
// takes 1): the same bits for every split.
extern "C" int o3dmi_internal_pointcloud_obb_minimal_approx(
        const void* points_dev, int64_t n, int dtype, int split,
        double center_out[3], double rotation_out[9], double extent_out[3],
        void* stream);
extern "C" int64_t o3dmi_internal_obe_resident_capacity();
extern "C" int o3dmi_internal_bounding_volume_stats(int64_t stats[5],
                                                    double values[16]);
