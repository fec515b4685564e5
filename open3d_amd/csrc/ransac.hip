// RANSAC on correspondences (o3d_mi355x.h, "RANSAC on correspondences"):
//   o3dmi_ransac_hypotheses  one lane per iteration: draws, gathers, Kabsch,
//                            checks (rules 1-3);
//   o3dmi_ransac_score       the hot path: (a few survivors) x (a tile of
//                            source points) per work item, the k = 1 search of
//                            nns.h over one target index, per-tile partials
//                            and a fixed-order second pass (rule 4); a sibling
//                            launch scores the correspondence list (rule 6).
// Float64 only where the contract asks for it (Kabsch, checks, sums); the
// per-point transform and distance are in the point dtype, like the search.
#include "ransac.h"

#include <algorithm>
#include <cmath>

#include "kabsch.h"
#include "nns.h"

namespace o3dmi {
namespace {

constexpr int kHypoBlock = 128;
constexpr int kScoreWaves = kRansacTile / 64;
constexpr int kScoreGroup = 8;  // survivors a work item scores at most

struct HypoArgs {
    uint64_t seed;
    int64_t first, count;
    const void* src;
    const void* tgt;
    const void* src_n;
    const void* tgt_n;
    int64_t ns, nt;
    const int64_t* corres;
    int64_t n_corres;
    int ransac_n;
    int n_check;
    int check_type[3];
    double check_thr[3];  // normal: cos(threshold)
    int64_t* samples;
    double* T;
    int32_t* pass;
};

template <typename P>
__device__ __forceinline__ void Load3(const void* base, int64_t row,
                                      double* out) {
    const P* p = (const P*)base + 3 * row;
    out[0] = (double)p[0];
    out[1] = (double)p[1];
    out[2] = (double)p[2];
}

__device__ __forceinline__ double Dist3(const double* a, const double* b) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt(x * x + y * y + z * z);
}

template <typename P>
__global__ void __launch_bounds__(kHypoBlock) HypothesisKernel(HypoArgs a) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < a.count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t it = a.first + i;
        const int n = a.ransac_n;
        int64_t* smp = a.samples + i * n;
        double* T = a.T + i * 16;
        // rule 1: the draws; the pairs must lie inside both clouds
        bool ok = true;
        for (int j = 0; j < n; ++j) {
            const int64_t c =
                    (int64_t)RansacDraw(a.seed, it, j, (uint64_t)a.n_corres);
            smp[j] = c;
            const int64_t si = a.corres[2 * c], ti = a.corres[2 * c + 1];
            if (si < 0 || si >= a.ns || ti < 0 || ti >= a.nt) ok = false;
        }
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
        if (ok) {
            // rule 2: means, centred sum in sample order, shared Jacobi routine
            double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
            for (int j = 0; j < n; ++j) {
                double s[3], q[3];
                Load3<P>(a.src, a.corres[2 * smp[j]], s);
                Load3<P>(a.tgt, a.corres[2 * smp[j] + 1], q);
                for (int k = 0; k < 3; ++k) {
                    ms[k] += s[k];
                    mt[k] += q[k];
                }
            }
            for (int k = 0; k < 3; ++k) {
                ms[k] /= (double)n;
                mt[k] /= (double)n;
            }
            double G[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int j = 0; j < n; ++j) {
                double s[3], q[3];
                Load3<P>(a.src, a.corres[2 * smp[j]], s);
                Load3<P>(a.tgt, a.corres[2 * smp[j] + 1], q);
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                        G[r][k] += (q[r] - mt[r]) * (s[k] - ms[k]);
            }
            double s0, s1;
            KabschJacobi(G, ms, mt, R, t, &s0, &s1);
            if (!(s0 > 0) || !(s1 > 1e-12 * s0)) ok = false;
        }
        // rule 3
        for (int c = 0; ok && c < a.n_check; ++c) {
            const double thr = a.check_thr[c];
            if (a.check_type[c] == O3DMI_RANSAC_CHECK_EDGE_LENGTH) {
                for (int x = 0; ok && x < n; ++x)
                    for (int y = x + 1; ok && y < n; ++y) {
                        double sx[3], sy[3], tx[3], ty[3];
                        Load3<P>(a.src, a.corres[2 * smp[x]], sx);
                        Load3<P>(a.src, a.corres[2 * smp[y]], sy);
                        Load3<P>(a.tgt, a.corres[2 * smp[x] + 1], tx);
                        Load3<P>(a.tgt, a.corres[2 * smp[y] + 1], ty);
                        const double ds = Dist3(sx, sy), dt = Dist3(tx, ty);
                        if (ds < dt * thr || dt < ds * thr) ok = false;
                    }
            } else if (a.check_type[c] == O3DMI_RANSAC_CHECK_DISTANCE) {
                for (int j = 0; ok && j < n; ++j) {
                    double s[3], q[3], m[3];
                    Load3<P>(a.src, a.corres[2 * smp[j]], s);
                    Load3<P>(a.tgt, a.corres[2 * smp[j] + 1], q);
                    for (int r = 0; r < 3; ++r)
                        m[r] = R[3 * r] * s[0] + R[3 * r + 1] * s[1] +
                               R[3 * r + 2] * s[2] + t[r];
                    if (Dist3(q, m) > thr) ok = false;
                }
            } else if (a.src_n && a.tgt_n) {
                for (int j = 0; ok && j < n; ++j) {
                    double s[3], q[3];
                    Load3<P>(a.src_n, a.corres[2 * smp[j]], s);
                    Load3<P>(a.tgt_n, a.corres[2 * smp[j] + 1], q);
                    double dot = 0;
                    for (int r = 0; r < 3; ++r)
                        dot += q[r] * (R[3 * r] * s[0] + R[3 * r + 1] * s[1] +
                                       R[3 * r + 2] * s[2]);
                    if (dot < thr) ok = false;
                }
            }
        }
        for (int r = 0; r < 3; ++r) {
            T[4 * r + 0] = R[3 * r + 0];
            T[4 * r + 1] = R[3 * r + 1];
            T[4 * r + 2] = R[3 * r + 2];
            T[4 * r + 3] = t[r];
        }
        T[12] = 0;
        T[13] = 0;
        T[14] = 0;
        T[15] = 1;
        a.pass[i] = ok ? 1 : 0;
    }
}

__global__ void CorresRangeKernel(const int64_t* __restrict__ corres,
                                  int64_t n, int64_t ns, int64_t nt,
                                  int* __restrict__ bad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = corres[2 * i], t = corres[2 * i + 1];
        if (s < 0 || s >= ns || t < 0 || t >= nt) atomicOr(bad, 1);
    }
}

__global__ void CompactKernel(const int32_t* __restrict__ pass,
                              const int64_t* __restrict__ position,
                              int64_t count, int64_t first,
                              const double* __restrict__ T,
                              int64_t* __restrict__ iterations,
                              double* __restrict__ T_out) {
    // 16 lanes per iteration: one matrix element each
    const int64_t total = count * 16;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total;
         x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = x >> 4;
        const int e = (int)(x & 15);
        if (!pass[i]) continue;
        const int64_t k = position[i];
        T_out[k * 16 + e] = T[i * 16 + e];
        if (e == 0) iterations[k] = first + i;
    }
}

// The matrix of survivor sv in the point dtype (o3dmi_transform_points casts
// the float64 matrix first). sv is wave-uniform: scalar loads.
template <typename P>
struct Mat {
    P m[16];
    __device__ __forceinline__ void Load(const double* __restrict__ T) {
#pragma unroll
        for (int e = 0; e < 16; ++e) m[e] = (P)T[e];
    }
    // TransformPointsKernel (icp.hip), statement by statement
    __device__ __forceinline__ void Apply(P p0, P p1, P p2, P* q) const {
        const P x0 = m[0] * p0 + m[1] * p1 + m[2] * p2 + m[3];
        const P x1 = m[4] * p0 + m[5] * p1 + m[6] * p2 + m[7];
        const P x2 = m[8] * p0 + m[9] * p1 + m[10] * p2 + m[11];
        const P x3 = m[12] * p0 + m[13] * p1 + m[14] * p2 + m[15];
        q[0] = x0 / x3;
        q[1] = x1 / x3;
        q[2] = x2 / x3;
    }
};

// Survivors per work item: kScoreGroup once that still leaves a few thousand
// work items, fewer for a small batch (the partials do not depend on it).
__device__ __forceinline__ int GroupSize(int64_t b, int64_t n_tiles) {
    const int64_t g = (b * n_tiles) / (kCUs * 8);
    return g >= kScoreGroup ? kScoreGroup : (g < 1 ? 1 : (int)g);
}

template <typename P>
__global__ void __launch_bounds__(kRansacTile)
ScoreKernel(NnsView<P> nv, const P* __restrict__ src, int64_t ns,
            const double* __restrict__ T, const int64_t* __restrict__ b_dev,
            int64_t b_max, int64_t n_tiles, int32_t* __restrict__ part_cnt,
            double* __restrict__ part_sum) {
    __shared__ int s_cnt[kScoreWaves][kScoreGroup];
    __shared__ double s_sum[kScoreWaves][kScoreGroup];
    int64_t b = b_dev ? *b_dev : b_max;
    if (b > b_max) b = b_max;
    const int gs = GroupSize(b, n_tiles);
    const int64_t groups = (b + gs - 1) / gs;
    const int64_t items = groups * n_tiles;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t g = item / n_tiles, tile = item - g * n_tiles;
        const int64_t p = tile * kRansacTile + threadIdx.x;
        const bool live = p < ns;
        P p0 = 0, p1 = 0, p2 = 0;
        if (live) {
            p0 = src[3 * p + 0];
            p1 = src[3 * p + 1];
            p2 = src[3 * p + 2];
        }
        const int64_t sv0 = g * gs;
        for (int k = 0; k < gs; ++k) {
            const int64_t sv = sv0 + k;
            if (sv >= b) break;  // uniform over the workgroup
            Mat<P> m;
            m.Load(T + sv * 16);
            int c = 0;
            double d = 0;
            if (live) {
                P q[3];
                m.Apply(p0, p1, p2, q);
                int idx;
                P d2;
                if (SearchNearest(nv, q, idx, d2) >= 0) {
                    c = 1;
                    d = (double)d2;
                }
            }
            // fixed tree over the wave
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c += __shfl_xor(c, o, 64);
                d += __shfl_xor(d, o, 64);
            }
            if (lane == 0) {
                s_cnt[wave][k] = c;
                s_sum[wave][k] = d;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < gs && sv0 + threadIdx.x < b) {
            int c = 0;
            double d = 0;
            for (int w = 0; w < kScoreWaves; ++w) {
                c += s_cnt[w][threadIdx.x];
                d += s_sum[w][threadIdx.x];
            }
            const int64_t o = (sv0 + threadIdx.x) * n_tiles + tile;
            part_cnt[o] = c;
            part_sum[o] = d;
        }
        __syncthreads();
    }
}

// One wave per survivor: lane l adds tiles l, l + 64, ... in order, then the
// fixed tree.
__global__ void __launch_bounds__(64)
ScoreFinalKernel(const int32_t* __restrict__ part_cnt,
                 const double* __restrict__ part_sum,
                 const int64_t* __restrict__ b_dev, int64_t b_max,
                 int64_t n_tiles, int64_t* __restrict__ counts,
                 double* __restrict__ sums) {
    int64_t b = b_dev ? *b_dev : b_max;
    if (b > b_max) b = b_max;
    for (int64_t sv = blockIdx.x; sv < b; sv += gridDim.x) {
        long long c = 0;
        double d = 0;
        for (int64_t t = threadIdx.x; t < n_tiles; t += 64) {
            c += part_cnt[sv * n_tiles + t];
            d += part_sum[sv * n_tiles + t];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o, 64);
            d += __shfl_xor(d, o, 64);
        }
        if (threadIdx.x == 0) {
            counts[sv] = c;
            sums[sv] = d;
        }
    }
}

// Rule 6: work item = (survivors, tile of correspondences); inliers[] zeroed
// by the caller (integer atomics: any order gives the same count).
template <typename P>
__global__ void __launch_bounds__(kRansacTile)
CorresScoreKernel(const P* __restrict__ src, const P* __restrict__ tgt,
                  int64_t ns, int64_t nt, const int64_t* __restrict__ corres,
                  int64_t n_corres, P r2, const double* __restrict__ T,
                  const int64_t* __restrict__ b_dev, int64_t b_max,
                  unsigned long long* __restrict__ inliers) {
    int64_t b = b_dev ? *b_dev : b_max;
    if (b > b_max) b = b_max;
    const int64_t n_tiles = (n_corres + kRansacTile - 1) / kRansacTile;
    const int gs = GroupSize(b, n_tiles);
    const int64_t groups = (b + gs - 1) / gs;
    const int64_t items = groups * n_tiles;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t g = item / n_tiles, tile = item - g * n_tiles;
        const int64_t c = tile * kRansacTile + threadIdx.x;
        bool live = c < n_corres;
        P s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0, t2 = 0;
        if (live) {
            const int64_t si = corres[2 * c], ti = corres[2 * c + 1];
            live = si >= 0 && si < ns && ti >= 0 && ti < nt;
            if (live) {
                s0 = src[3 * si + 0];
                s1 = src[3 * si + 1];
                s2 = src[3 * si + 2];
                t0 = tgt[3 * ti + 0];
                t1 = tgt[3 * ti + 1];
                t2 = tgt[3 * ti + 2];
            }
        }
        for (int k = 0; k < gs; ++k) {
            const int64_t sv = g * gs + k;
            if (sv >= b) break;
            Mat<P> m;
            m.Load(T + sv * 16);
            P q[3];
            m.Apply(s0, s1, s2, q);
            P result = P(0);
            const P d0 = q[0] - t0;
            result += d0 * d0;
            const P d1 = q[1] - t1;
            result += d1 * d1;
            const P d2 = q[2] - t2;
            result += d2 * d2;
            const unsigned long long hit = __ballot(live && result < r2);
            if (lane == 0 && hit)
                atomicAdd(&inliers[sv], (unsigned long long)__popcll(hit));
        }
    }
}

}  // namespace
}  // namespace o3dmi

using namespace o3dmi;

extern "C" {

int o3dmi_ransac_hypotheses(uint64_t seed, int64_t first_iteration,
                            int64_t count, const void* source_dev, int64_t ns,
                            const void* target_dev, int64_t nt,
                            const void* source_normals_dev,
                            const void* target_normals_dev, int dtype,
                            const int64_t* corres_dev, int64_t n_corres,
                            int ransac_n, int num_checkers,
                            const int* checker_types,
                            const double* checker_thresholds,
                            int64_t* samples_dev, double* transformations_dev,
                            int32_t* pass_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(first_iteration >= 0 && count >= 0, "negative iteration");
    if (ransac_n > O3DMI_RANSAC_MAX_N) {
        SetLastError("ransac_n > 8 is not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    O3DMI_REQUIRE(ransac_n >= 3, "ransac_n must be at least 3");
    O3DMI_REQUIRE(num_checkers >= 0 && num_checkers <= 3 &&
                          (num_checkers == 0 ||
                           (checker_types && checker_thresholds)),
                  "at most one checker of each kind");
    if (count == 0) return O3DMI_OK;
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(corres_dev && n_corres > 0, "no correspondences");
    O3DMI_REQUIRE(samples_dev && transformations_dev && pass_dev,
                  "null output");
    HypoArgs a;
    a.seed = seed;
    a.first = first_iteration;
    a.count = count;
    a.src = source_dev;
    a.tgt = target_dev;
    a.src_n = source_normals_dev;
    a.tgt_n = target_normals_dev;
    a.ns = ns;
    a.nt = nt;
    a.corres = corres_dev;
    a.n_corres = n_corres;
    a.ransac_n = ransac_n;
    a.n_check = num_checkers;
    unsigned seen = 0;
    for (int c = 0; c < 3; ++c) {
        a.check_type[c] = -1;
        a.check_thr[c] = 0;
    }
    for (int c = 0; c < num_checkers; ++c) {
        const int ty = checker_types[c];
        O3DMI_REQUIRE(ty >= 0 && ty <= 2 && !(seen & (1u << ty)),
                      "at most one checker of each kind");
        seen |= 1u << ty;
        a.check_type[c] = ty;
        a.check_thr[c] = ty == O3DMI_RANSAC_CHECK_NORMAL
                                 ? std::cos(checker_thresholds[c])
                                 : checker_thresholds[c];
    }
    a.samples = samples_dev;
    a.T = transformations_dev;
    a.pass = pass_dev;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(GridFor(count, kHypoBlock)), block(kHypoBlock);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(HypothesisKernel<double>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(HypothesisKernel<float>, grid, block, 0, s, a);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int o3dmi_internal_ransac_corres_range(const int64_t* corres_dev,
                                       int64_t n_corres, int64_t ns,
                                       int64_t nt, int* bad_dev,
                                       o3dmi_stream_t stream) {
    if (n_corres <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(CorresRangeKernel, dim3(GridFor(n_corres, kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, corres_dev,
                       n_corres, ns, nt, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int o3dmi_internal_ransac_compact(const int32_t* pass_dev,
                                  const int64_t* position_dev, int64_t count,
                                  int64_t first_iteration,
                                  const double* transformations_dev,
                                  int64_t* iterations_dev,
                                  double* transformations_out_dev,
                                  o3dmi_stream_t stream) {
    if (count <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(CompactKernel, dim3(GridFor(count * 16, kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, pass_dev,
                       position_dev, count, first_iteration,
                       transformations_dev, iterations_dev,
                       transformations_out_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int o3dmi_internal_ransac_score(const o3dmi_nns_t* nns, const void* source_dev,
                                int64_t ns, const void* target_dev, int64_t nt,
                                const double* transformations_dev,
                                const int64_t* b_dev, int64_t b_max,
                                const int64_t* corres_dev, int64_t n_corres,
                                int32_t* part_counts_dev,
                                double* part_sums_dev, int64_t* counts_dev,
                                double* d2_sums_dev,
                                int64_t* corres_inliers_dev,
                                o3dmi_stream_t stream) {
    O3DMI_REQUIRE(nns && source_dev && ns > 0 && transformations_dev &&
                          part_counts_dev && part_sums_dev && counts_dev &&
                          d2_sums_dev,
                  "null argument");
    if (b_max <= 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = RansacTiles(ns);
    const int64_t max_items = b_max * n_tiles;
    const int grid = (int)std::min<int64_t>(max_items, (int64_t)kCUs * 16);
    const bool f64 = nns->dtype == O3DMI_F64;
    if (f64)
        hipLaunchKernelGGL(ScoreKernel<double>, dim3(grid), dim3(kRansacTile),
                           0, s, MakeView<double>(nns),
                           (const double*)source_dev, ns, transformations_dev,
                           b_dev, b_max, n_tiles, part_counts_dev,
                           part_sums_dev);
    else
        hipLaunchKernelGGL(ScoreKernel<float>, dim3(grid), dim3(kRansacTile),
                           0, s, MakeView<float>(nns),
                           (const float*)source_dev, ns, transformations_dev,
                           b_dev, b_max, n_tiles, part_counts_dev,
                           part_sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ScoreFinalKernel,
                       dim3((int)std::min<int64_t>(b_max, kCUs * 16)),
                       dim3(64), 0, s, part_counts_dev, part_sums_dev, b_dev,
                       b_max, n_tiles, counts_dev, d2_sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    if (corres_inliers_dev && corres_dev && n_corres > 0) {
        O3DMI_REQUIRE(target_dev && nt > 0, "target is null");
        O3DMI_HIP_CHECK(hipMemsetAsync(corres_inliers_dev, 0,
                                       sizeof(int64_t) * (size_t)b_max, s));
        const int64_t c_items = b_max * RansacTiles(n_corres);
        const int c_grid =
                (int)std::min<int64_t>(c_items, (int64_t)kCUs * 16);
        if (f64) {
            const NnsView<double> v = MakeView<double>(nns);
            hipLaunchKernelGGL(
                    CorresScoreKernel<double>, dim3(c_grid),
                    dim3(kRansacTile), 0, s, (const double*)source_dev,
                    (const double*)target_dev, ns, nt, corres_dev, n_corres,
                    v.radius_squared, transformations_dev, b_dev, b_max,
                    (unsigned long long*)corres_inliers_dev);
        } else {
            const NnsView<float> v = MakeView<float>(nns);
            hipLaunchKernelGGL(
                    CorresScoreKernel<float>, dim3(c_grid), dim3(kRansacTile),
                    0, s, (const float*)source_dev, (const float*)target_dev,
                    ns, nt, corres_dev, n_corres, v.radius_squared,
                    transformations_dev, b_dev, b_max,
                    (unsigned long long*)corres_inliers_dev);
        }
        O3DMI_HIP_CHECK(hipGetLastError());
    }
    return O3DMI_OK;
}

// partials of at most 2^22 (transformation, tile) pairs at a time
static int64_t ScoreChunk(int64_t ns, int64_t b) {
    return std::max<int64_t>(
            1, std::min<int64_t>(b, kRansacMaxPartials / RansacTiles(ns)));
}

size_t o3dmi_ransac_score_scratch_bytes(int64_t ns, int64_t b) {
    if (ns <= 0 || b <= 0) return 0;
    // float64 sums first, then the int32 counts
    return 12 * (size_t)(ScoreChunk(ns, b) * RansacTiles(ns));
}

int o3dmi_ransac_score(const o3dmi_nns_t* nns, const void* source_dev,
                       int64_t ns, const void* target_dev, int64_t nt,
                       const double* transformations_dev, int64_t b,
                       const int64_t* corres_dev, int64_t n_corres,
                       int64_t* counts_dev, double* d2_sums_dev,
                       int64_t* corres_inliers_dev, void* scratch_dev,
                       o3dmi_stream_t stream) {
    O3DMI_REQUIRE(nns != nullptr && ns > 0 && b >= 0, "bad argument");
    if (b == 0) return O3DMI_OK;
    O3DMI_REQUIRE(scratch_dev != nullptr, "scratch is null");
    const int64_t n_tiles = RansacTiles(ns);
    const int64_t chunk = ScoreChunk(ns, b);
    double* ps = (double*)scratch_dev;
    int32_t* pc = (int32_t*)(ps + chunk * n_tiles);
    for (int64_t o = 0; o < b; o += chunk) {
        const int64_t m = std::min(chunk, b - o);
        const int st = o3dmi_internal_ransac_score(
                nns, source_dev, ns, target_dev, nt,
                transformations_dev + 16 * o, nullptr, m, corres_dev, n_corres,
                pc, ps, counts_dev + o, d2_sums_dev + o,
                corres_inliers_dev ? corres_inliers_dev + o : nullptr, stream);
        if (st) return st;
    }
    return O3DMI_OK;
}

int64_t o3dmi_internal_ransac_next_batch(int64_t batch, int64_t ns,
                                         int64_t n_surv, int64_t* cap_out) {
    const int64_t cap = RansacBatchCap(ns);
    if (cap_out) *cap_out = cap;
    return RansacNextBatch(batch, cap, n_surv, ns);
}

}  // extern "C"
