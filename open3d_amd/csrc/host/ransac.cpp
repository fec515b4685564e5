// RegistrationRANSACBasedOnCorrespondence / ...BasedOnFeatureMatching (legacy
// pipelines/registration/Registration.cpp:212-406) over the kernels of
// ransac.hip: the reference loop of ONE thread, run a batch of hypotheses per
// round (rules 1-7 in o3d_mi355x.h / o3d_mi355x_host.h).
//
// A round queues: hypotheses -> prefix sum of the pass flags -> survivors in
// iteration order -> scoring of all survivors -> one copy of the per-survivor
// arrays to pinned memory; the host waits once, then scans the survivors in
// ascending iteration exactly as the sequential loop would, moving the
// stopping bound as it goes. Work a batch did past the bound is dropped.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "common.h"
#include "host/host_util.h"
#include "nns.h"
#include "o3d_mi355x_host.h"
#include "ransac.h"
#include "scan.h"

using namespace o3dmi;

namespace {

void EmptyResult(o3dmi_registration_result_t* r, o3dmi_ransac_info_t* info,
                 int64_t bound) {
    for (int i = 0; i < 16; ++i) r->transformation[i] = (i % 5 == 0) ? 1 : 0;
    r->fitness = 0;
    r->inlier_rmse = 0;
    r->converged = 0;
    r->num_iterations = 0;
    r->num_correspondences = 0;
    if (info) {
        info->best_iteration = -1;
        info->num_validations = 0;
        info->final_iteration_bound = bound;
        info->iterations_run = 0;
        info->num_batches = 0;
    }
}

// The pinned block the per-round arrays are copied to: one per host thread,
// kept for the life of the process like the drivers' mailboxes, grown on demand.
void* ThreadPinned(size_t bytes) {
    thread_local void* p = nullptr;
    thread_local size_t have = 0;
    if (bytes > have) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        have = 0;
        if (hipHostMalloc(&p, bytes) != hipSuccess) return nullptr;
        have = bytes;
    }
    return p;
}

int CheckEstimator(int estimation, int with_scaling, int ransac_n) {
    if (estimation != O3DMI_ICP_POINT_TO_POINT)
        return Unsupported(
                "RANSAC supports TransformationEstimationPointToPoint only");
    if (with_scaling) return Unsupported("with_scaling is not supported");
    if (ransac_n > O3DMI_RANSAC_MAX_N)
        return Unsupported("ransac_n > 8 is not supported");
    return O3DMI_OK;
}

}  // namespace

extern "C" int o3dmi_registration_ransac_correspondence(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        const void* source_normals_dev, const void* target_normals_dev,
        int dtype, const int64_t* corres_dev, int64_t n_corres,
        double max_dist, int estimation, int with_scaling, int ransac_n,
        const o3dmi_ransac_options_t* opt, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_ransac_info_t* info,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(result != nullptr && opt != nullptr, "null argument");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    int st = CheckEstimator(estimation, with_scaling, ransac_n);
    if (st) return st;
    O3DMI_REQUIRE(opt->num_checkers >= 0 && opt->num_checkers <= 3,
                  "at most one checker of each kind");
    {
        unsigned seen = 0;
        for (int c = 0; c < opt->num_checkers; ++c) {
            const int ty = opt->checker_types[c];
            O3DMI_REQUIRE(ty >= 0 && ty <= 2 && !(seen & (1u << ty)),
                          "at most one checker of each kind");
            seen |= 1u << ty;
        }
    }
    O3DMI_REQUIRE(opt->batch_size >= 0, "batch_size is negative");
    hipStream_t s = (hipStream_t)stream;
    const int64_t max_it = opt->max_iteration;
    EmptyResult(result, info, std::max<int64_t>(max_it, 0));
    if (correspondences_dev && ns > 0)
        O3DMI_HIP_CHECK(hipMemsetAsync(correspondences_dev, 0xFF,
                                       sizeof(int64_t) * (size_t)ns, s));
    // Registration.cpp:356-359
    if (ransac_n < 3 || n_corres < ransac_n || max_dist <= 0.0 ||
        max_it <= 0) {
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(corres_dev != nullptr, "correspondences are null");

    const int64_t n_tiles = RansacTiles(ns);
    const int64_t cap = RansacBatchCap(ns);
    const bool adaptive = opt->batch_size == 0;
    int64_t batch = adaptive ? std::min(kRansacFirstBatch, cap)
                             : std::min<int64_t>(opt->batch_size, cap);
    // every per-round buffer holds bmax hypotheses
    const int64_t bmax = adaptive ? cap : batch;

    PoolScratch sc(s);
    NnsGuard index;
    int* bad = nullptr;
    int64_t* samples = nullptr;
    double* T_all = nullptr;
    int32_t* pass = nullptr;
    int64_t* position = nullptr;
    void* scan_tmp = nullptr;
    double* T_surv = nullptr;
    int32_t* part_cnt = nullptr;
    double* part_sum = nullptr;
    int64_t* block = nullptr;  // [n_surv | iterations | counts | corres | sums]
    const size_t block_words = 1 + 4 * (size_t)bmax;
    if ((st = sc.Alloc(&bad, sizeof(int))) ||
        (st = sc.Alloc(&samples, 8 * (size_t)(bmax * ransac_n))) ||
        (st = sc.Alloc(&T_all, 8 * 16 * (size_t)bmax)) ||
        (st = sc.Alloc(&pass, 4 * (size_t)bmax)) ||
        (st = sc.Alloc(&position, 8 * (size_t)bmax)) ||
        (st = sc.Alloc(&scan_tmp, ScanScratchBytes(bmax))) ||
        (st = sc.Alloc(&T_surv, 8 * 16 * (size_t)bmax)) ||
        (st = sc.Alloc(&part_cnt, 4 * (size_t)(bmax * n_tiles))) ||
        (st = sc.Alloc(&part_sum, 8 * (size_t)(bmax * n_tiles))) ||
        (st = sc.Alloc(&block, 8 * block_words)))
        return st;
    int64_t* h = (int64_t*)ThreadPinned(8 * block_words);
    O3DMI_REQUIRE(h != nullptr, "pinned host allocation failed");

    O3DMI_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    if ((st = o3dmi_internal_ransac_corres_range(corres_dev, n_corres, ns, nt,
                                                 bad, stream)))
        return st;
    int hbad = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    // the target index, built once per call (radius = max_distance)
    if ((st = o3dmi_nns_create(target_dev, nt, dtype, max_dist, stream,
                               &index.nns)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!hbad, "correspondence index out of range");

    const double log_confidence = std::log(1.0 - opt->confidence);
    int64_t est_k = max_it;
    int64_t best_it = -1, validations = 0, run = 0, batches = 0;
    double best_fitness = 0, best_rmse = 0;
    for (int64_t first = 0; first < est_k;) {
        const int64_t count = std::min(batch, max_it - first);
        if (count < 1 || count > bmax) {
            SetLastError("ransac: batch beyond the round buffers");
            return O3DMI_ERR_INTERNAL;
        }
        // this round's arrays, packed behind the survivor count
        int64_t* d_n = block;
        int64_t* d_it = block + 1;
        int64_t* d_cnt = d_it + count;
        int64_t* d_cor = d_cnt + count;
        double* d_sum = (double*)(d_cor + count);
        if ((st = o3dmi_ransac_hypotheses(
                     opt->seed, first, count, source_dev, ns, target_dev, nt,
                     source_normals_dev, target_normals_dev, dtype, corres_dev,
                     n_corres, ransac_n, opt->num_checkers, opt->checker_types,
                     opt->checker_thresholds, samples, T_all, pass, stream)) ||
            (st = PrefixSumAsync(pass, count, false, position, d_n, scan_tmp,
                                 s)) ||
            (st = o3dmi_internal_ransac_compact(pass, position, count, first,
                                                T_all, d_it, T_surv,
                                                stream)) ||
            (st = o3dmi_internal_ransac_score(
                     index.nns, source_dev, ns, target_dev, nt, T_surv, d_n,
                     count, corres_dev, n_corres, part_cnt, part_sum, d_cnt,
                     d_sum, d_cor, stream)))
            return st;
        const size_t words = 1 + 4 * (size_t)count;
        O3DMI_HIP_CHECK(hipMemcpyAsync(h, block, 8 * words,
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        ++batches;
        run += count;
        const int64_t n_surv = h[0];
        if (n_surv < 0 || n_surv > count) {
            SetLastError("ransac: survivor count out of range");
            return O3DMI_ERR_INTERNAL;
        }
        const int64_t* h_it = h + 1;
        const int64_t* h_cnt = h_it + count;
        const int64_t* h_cor = h_cnt + count;
        const double* h_sum = (const double*)(h_cor + count);
        for (int64_t k = 0; k < n_surv; ++k) {
            const int64_t i = h_it[k];
            if (i >= est_k) break;  // est_k only shrinks: the rest is dropped
            ++validations;
            // ComputeRegistrationResult, Registration.cpp:24-62
            const double num = (double)h_cnt[k];
            const double fitness = h_cnt[k] ? num / (double)ns : 0.0;
            const double rmse = h_cnt[k] ? std::sqrt(h_sum[k] / num) : 0.0;
            // IsBetterRANSACThan
            if (fitness > best_fitness ||
                (fitness == best_fitness && rmse < best_rmse)) {
                best_fitness = fitness;
                best_rmse = rmse;
                best_it = i;
                const double ratio = (double)h_cor[k] / (double)n_corres;
                // Registration.cpp:315-324
                const double est = log_confidence /
                                   std::log(1.0 - std::pow(ratio, ransac_n));
                if (!(est < 0) && est < (double)est_k)
                    est_k = (int64_t)std::ceil(est);
            }
        }
        first += count;
        if (adaptive) batch = RansacNextBatch(batch, cap, n_surv, ns);
    }
    if (info) {
        info->best_iteration = best_fitness > 0 ? best_it : -1;
        info->num_validations = validations;
        info->final_iteration_bound = est_k;
        info->iterations_run = run;
        info->num_batches = batches;
    }
    if (best_it < 0 || !(best_fitness > 0)) return O3DMI_OK;
    // T_best: the hypothesis of iteration best_it formed once more (a pure
    // function of the seed and the iteration: the same bits), so that a round
    // has one host wait whether or not its best changed
    double best_T[16];
    if ((st = o3dmi_ransac_hypotheses(
                 opt->seed, best_it, 1, source_dev, ns, target_dev, nt,
                 source_normals_dev, target_normals_dev, dtype, corres_dev,
                 n_corres, ransac_n, opt->num_checkers, opt->checker_types,
                 opt->checker_thresholds, samples, T_all, pass, stream)))
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(best_T, T_all, sizeof(best_T),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    // rule 7: the result is the evaluate path's, bit for bit
    return o3dmi_registration_evaluate(source_dev, ns, target_dev, nt, dtype,
                                       max_dist, best_T, correspondences_dev,
                                       result, stream);
}

extern "C" int o3dmi_registration_ransac_feature_matching(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        const void* source_normals_dev, const void* target_normals_dev,
        int dtype, const void* source_features_dev,
        const void* target_features_dev, int dim, int feature_dtype,
        int mutual_filter, double max_dist, int estimation, int with_scaling,
        int ransac_n, const o3dmi_ransac_options_t* opt,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_ransac_info_t* info, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(result != nullptr && opt != nullptr, "null argument");
    int st = CheckEstimator(estimation, with_scaling, ransac_n);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    // Registration.cpp:396-398
    if (ransac_n < 3 || max_dist <= 0.0) {
        EmptyResult(result, info, std::max(opt->max_iteration, 0));
        if (correspondences_dev && ns > 0)
            O3DMI_HIP_CHECK(hipMemsetAsync(correspondences_dev, 0xFF,
                                           sizeof(int64_t) * (size_t)ns, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }
    O3DMI_REQUIRE(source_features_dev && target_features_dev && ns > 0 &&
                          nt > 0 && dim > 0,
                  "empty feature set");
    PoolScratch sc(s);
    int64_t* corres = nullptr;
    if ((st = sc.Alloc(&corres, 16 * (size_t)ns))) return st;
    int64_t n_corres = 0;
    // Feature.cpp:279-333 with its default mutual_consistency_ratio
    if ((st = o3dmi_registration_correspondences_from_features(
                 source_features_dev, ns, target_features_dev, nt, dim,
                 feature_dtype, mutual_filter, 0.1f, corres, &n_corres,
                 nullptr, stream)))
        return st;
    return o3dmi_registration_ransac_correspondence(
            source_dev, ns, target_dev, nt, source_normals_dev,
            target_normals_dev, dtype, corres, n_corres, max_dist, estimation,
            with_scaling, ransac_n, opt, correspondences_dev, result, info,
            stream);
}
