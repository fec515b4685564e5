// Private header of the RANSAC operators: the sample function (rule 1 of the
// contract in o3d_mi355x.h) and the steps ransac.hip offers the host driver
// (host/ransac.cpp) beyond the public kernel seam.
#pragma once

#include "common.h"

namespace o3dmi {

constexpr int kRansacTile = 256;  // source points per scoring tile

// Draw j of iteration i over n correspondences.
__host__ __device__ inline uint64_t RansacDraw(uint64_t seed, int64_t i, int j,
                                               uint64_t n) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull *
                                ((uint64_t)i * 8ull + (uint64_t)j + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(z, n);
#else
    return (uint64_t)(((unsigned __int128)z * n) >> 64);
#endif
}

// The finaliser RansacDraw applies to its counter.
__host__ __device__ inline uint64_t SplitMix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// Entry j of a permutation of [0, n) chosen by seed (0 <= j < n < 2^62): a
// stateless bijection. Four rounds of a balanced Feistel network over 2 h
// bits, 4^h the lowest even power of two >= n, with SplitMix64 of (seed, round,
// right half) as round function; a value >= n is fed through again (cycle
// walking). The network permutes [0, 4^h), so the walk follows the cycle of j,
// which returns to j < n: it ends, after fewer than 4 steps on average.
__host__ __device__ inline int64_t SampleIndex(uint64_t seed, int64_t n,
                                               int64_t j) {
    int h = 1;
    while ((1ull << (2 * h)) < (uint64_t)n) ++h;
    const uint64_t half = (1ull << h) - 1;
    uint64_t v = (uint64_t)j;
    do {
        uint64_t l = v >> h, r = v & half;
        for (uint64_t k = 0; k < 4; ++k) {
            const uint64_t f =
                    SplitMix64(seed + 0x9E3779B97F4A7C15ull * (r * 4 + k + 1));
            const uint64_t t = l ^ (f & half);
            l = r;
            r = t;
        }
        v = (l << h) | r;
    } while (v >= (uint64_t)n);
    return (int64_t)v;
}

inline int64_t RansacTiles(int64_t ns) {
    return (ns + kRansacTile - 1) / kRansacTile;
}

// The driver's batch schedule. A round holds one partial per (survivor,
// tile): at most 2^22 of them, and at most 16384 hypotheses. Every per-round
// buffer is sized by this cap, so no batch may exceed it.
constexpr int64_t kRansacMaxBatch = 16384;
constexpr int64_t kRansacFirstBatch = 1024;
constexpr int64_t kRansacMaxPartials = 1ll << 22;

inline int64_t RansacBatchCap(int64_t ns) {
    const int64_t c = kRansacMaxPartials / RansacTiles(ns);
    return c < 1 ? 1 : (c > kRansacMaxBatch ? kRansacMaxBatch : c);
}

// The batch after a round of `batch` hypotheses with n_surv survivors: enough
// queries per round to fill the chip (double below 2^21), not more work past
// the bound than that needs (halve above 2^24, not below 64); never above cap.
inline int64_t RansacNextBatch(int64_t batch, int64_t cap, int64_t n_surv,
                               int64_t ns) {
    const int64_t queries = (n_surv < 1 ? 1 : n_surv) * ns;
    if (queries < (1ll << 21)) batch *= 2;
    else if (queries > (1ll << 24)) batch = batch / 2 < 64 ? 64 : batch / 2;
    return batch > cap ? cap : batch;
}

}  // namespace o3dmi

extern "C" {
// *bad_dev (zeroed by the caller) becomes non-zero when a pair of corres_dev
// lies outside [0, ns) x [0, nt).
int o3dmi_internal_ransac_corres_range(const int64_t* corres_dev,
                                       int64_t n_corres, int64_t ns,
                                       int64_t nt, int* bad_dev,
                                       o3dmi_stream_t stream);
// Survivors of a batch in iteration order: position_dev = exclusive prefix sum
// of pass_dev. iterations_dev[k] / transformations_out_dev[k] = iteration
// number and matrix of the k-th survivor.
int o3dmi_internal_ransac_compact(const int32_t* pass_dev,
                                  const int64_t* position_dev, int64_t count,
                                  int64_t first_iteration,
                                  const double* transformations_dev,
                                  int64_t* iterations_dev,
                                  double* transformations_out_dev,
                                  o3dmi_stream_t stream);
// o3dmi_ransac_score with the number of transformations read on the device
// (*b_dev <= b_max; NULL: b_max) and the caller's partials:
// part_counts_dev int32 / part_sums_dev float64 {b_max, RansacTiles(ns)}.
int o3dmi_internal_ransac_score(const o3dmi_nns_t* nns, const void* source_dev,
                                int64_t ns, const void* target_dev, int64_t nt,
                                const double* transformations_dev,
                                const int64_t* b_dev, int64_t b_max,
                                const int64_t* corres_dev, int64_t n_corres,
                                int32_t* part_counts_dev,
                                double* part_sums_dev, int64_t* counts_dev,
                                double* d2_sums_dev,
                                int64_t* corres_inliers_dev,
                                o3dmi_stream_t stream);
// The driver's batch schedule (RansacBatchCap / RansacNextBatch), for tests.
int64_t o3dmi_internal_ransac_next_batch(int64_t batch, int64_t ns,
                                         int64_t n_surv, int64_t* cap_out);
}
