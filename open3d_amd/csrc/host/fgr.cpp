// FastGlobalRegistrationBasedOnCorrespondence / ...BasedOnFeatureMatching
// (legacy pipelines/registration/FastGlobalRegistration.cpp) over the kernels
// of fgr.hip (rules 1-6 in o3d_mi355x.h / o3d_mi355x_host.h).
//
// A call queues: the gate and rule 1 (finiteness of both clouds, the range of
// the pairs, sums, scales, the normalised clouds; ONE download), the matching
// (feature entry point), the tuple test (one wait per batch), the whole
// optimisation (no wait: one launch, or 2 x iteration_number launches), one
// download of trans; rule 5 runs on the host and ends in the evaluate path.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "feature.h"
#include "fgr.h"
#include "host/pointcloud_call.h"
#include "o3d_mi355x_host.h"
#include "ransac.h"

using namespace o3dmi;

namespace {

int CheckOptions(const o3dmi_fgr_options_t* o) {
    O3DMI_REQUIRE(o->maximum_tuple_count > 0,
                  "maximum_tuple_count must be > 0");
    O3DMI_REQUIRE(std::isfinite(o->division_factor) && o->division_factor > 0,
                  "division_factor must be finite and > 0");
    O3DMI_REQUIRE(std::isfinite(o->tuple_scale) && o->tuple_scale > 0,
                  "tuple_scale must be finite and > 0");
    O3DMI_REQUIRE(std::isfinite(o->maximum_correspondence_distance) &&
                          o->maximum_correspondence_distance > 0,
                  "maximum_correspondence_distance must be finite and > 0");
    O3DMI_REQUIRE(o->iteration_number >= 0, "iteration_number is negative");
    return O3DMI_OK;
}

// What rule 1 leaves behind: the normalised clouds and the words on the host.
struct Prepared {
    double* source = nullptr;  // {ns, 3}
    double* target = nullptr;  // {nt, 3}
    FgrNormWords words;
};

// The gate and rule 1; corres_dev may be NULL (feature entry point: the
// matching forms its pairs from row numbers).
int Prepare(PoolScratch& sc, const void* source_dev, int64_t ns,
            const void* target_dev, int64_t nt, int dtype,
            const int64_t* corres_dev, int64_t n_corres,
            const o3dmi_fgr_options_t* opt, Prepared* out) {
    hipStream_t s = sc.s;
    FgrNormWords* w = nullptr;
    double* tree = nullptr;
    int* range_bad = nullptr;
    int st;
    if ((st = sc.Alloc(&w, sizeof(FgrNormWords))) ||
        (st = sc.Alloc(&range_bad, sizeof(int))) ||
        (st = sc.Alloc(&tree, 8 * FgrNormScratchDoubles(ns, nt))) ||
        (st = sc.Alloc(&out->source, 24 * (size_t)ns)) ||
        (st = sc.Alloc(&out->target, 24 * (size_t)nt)))
        return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(w, 0, sizeof(FgrNormWords), s));
    O3DMI_HIP_CHECK(hipMemsetAsync(range_bad, 0, sizeof(int), s));
    if ((st = CheckFiniteAsync(source_dev, ns, dtype, &w->bad, s)) ||
        (st = CheckFiniteAsync(target_dev, nt, dtype, &w->bad, s)))
        return st;
    if (corres_dev &&
        (st = o3dmi_internal_ransac_corres_range(corres_dev, n_corres, ns, nt,
                                                 range_bad,
                                                 (o3dmi_stream_t)s)))
        return st;
    if ((st = FgrNormalizeAsync(source_dev, ns, target_dev, nt, dtype,
                                opt->use_absolute_scale, tree, w, out->source,
                                out->target, s)))
        return st;
    int hbad = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&out->words, w, sizeof(FgrNormWords),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipMemcpyAsync(&hbad, range_bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!out->words.bad,
                  "non-finite coordinate: run RemoveNonFinitePoints first");
    O3DMI_REQUIRE(!hbad, "correspondence index out of range");
    // FastGlobalRegistration.cpp:187-190
    O3DMI_REQUIRE(out->words.scale_global > 0 &&
                          std::isfinite(out->words.scale_global),
                  "Invalid scale_global, it must be > 0.");
    return O3DMI_OK;
}

// Rule 3 on (first, second) with pairs {n, 2}: *used / *n_used = the tuples.
int TupleTest(PoolScratch& sc, const void* first_dev, int64_t n_first,
              const void* second_dev, int64_t n_second, int dtype,
              const int64_t* pairs, int64_t n, const o3dmi_fgr_options_t* opt,
              int64_t** used, int64_t* n_used, o3dmi_fgr_info_t* info) {
    *used = nullptr;
    *n_used = 0;
    const int64_t rows =
            3 * std::min<int64_t>(opt->maximum_tuple_count, 100 * n);
    int st;
    if ((st = sc.Alloc(used, 16 * (size_t)std::max<int64_t>(rows, 1))))
        return st;
    int64_t n_tuples = 0, n_trials = 0;
    if ((st = o3dmi_fgr_tuple_test(opt->seed, first_dev, n_first, second_dev,
                                   n_second, dtype, pairs, n, opt->tuple_scale,
                                   opt->maximum_tuple_count, *used, &n_tuples,
                                   &n_trials, (o3dmi_stream_t)sc.s)))
        return st;
    *n_used = 3 * n_tuples;
    info->n_tuples = n_tuples;
    info->n_trials = n_trials;
    return O3DMI_OK;
}

// Rules 4 and 5 on the correspondences the optimisation sees.
int Finish(PoolScratch& sc, const Prepared& prep, const void* source_dev,
           int64_t ns, const void* target_dev, int64_t nt, int dtype,
           const int64_t* used, int64_t n_used, const o3dmi_fgr_options_t* opt,
           int64_t* correspondences_dev, o3dmi_registration_result_t* result,
           o3dmi_fgr_info_t* info, o3dmi_fgr_info_t* info_out) {
    hipStream_t s = sc.s;
    double* out = nullptr;
    void* scratch = nullptr;
    int st;
    if ((st = sc.Alloc(&out, 8 * 18))) return st;
    const size_t bytes = o3dmi_fgr_optimize_scratch_bytes(n_used);
    if (bytes && (st = sc.Alloc(&scratch, bytes))) return st;
    int form = 0;
    if ((st = o3dmi_internal_fgr_optimize(
                 prep.source, ns, prep.target, nt, used, n_used,
                 prep.words.par_start, opt->division_factor, opt->decrease_mu,
                 opt->maximum_correspondence_distance, opt->iteration_number,
                 kFgrFormAuto, scratch, out, &form, (o3dmi_stream_t)s)))
        return st;
    double h[18];
    O3DMI_HIP_CHECK(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    // rule 5: GetTransformationOriginalScale, then the rigid inverse
    const double* ms = prep.words.mean;
    const double* mt = prep.words.mean + 3;
    const double sg = prep.words.scale_global;
    double G[16], T[16];
    for (int i = 0; i < 3; ++i) {
        const double* R = h + 4 * i;
        const double rm = (R[0] * mt[0] + R[1] * mt[1]) + R[2] * mt[2];
        G[4 * i + 0] = R[0];
        G[4 * i + 1] = R[1];
        G[4 * i + 2] = R[2];
        G[4 * i + 3] = ((-rm) + R[3] * sg) + ms[i];
    }
    G[12] = 0;
    G[13] = 0;
    G[14] = 0;
    G[15] = 1;
    InverseTransformation(G, T);
    info->n_used = n_used;
    info->scale_global = sg;
    info->final_par = h[16];
    info->failed_solves = (int)h[17];
    info->form = form;
    if ((st = o3dmi_registration_evaluate(
                 source_dev, ns, target_dev, nt, dtype,
                 opt->maximum_correspondence_distance, T, correspondences_dev,
                 result, (o3dmi_stream_t)s)))
        return st;
    // EvaluateRegistration reports the identity when nothing matches
    // (Registration.cpp:56-58); the transformation FGR found stays the result
    for (int e = 0; e < 16; ++e) result->transformation[e] = T[e];
    if (info_out) *info_out = *info;
    return O3DMI_OK;
}

o3dmi_fgr_info_t EmptyInfo() {
    o3dmi_fgr_info_t i;
    i.n_initial = 0;
    i.n_trials = 0;
    i.n_tuples = 0;
    i.n_used = 0;
    i.scale_global = 0;
    i.final_par = 0;
    i.swapped = 0;
    i.failed_solves = 0;
    i.form = 0;
    return i;
}

}  // namespace

extern "C" int o3dmi_registration_fgr_correspondence(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, const int64_t* corres_dev, int64_t n_corres,
        const o3dmi_fgr_options_t* opt, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_fgr_info_t* info_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(result != nullptr && opt != nullptr, "null argument");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    int st = CheckOptions(opt);
    if (st) return st;
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(n_corres >= 0 && (n_corres == 0 || corres_dev),
                  "correspondences are null");
    PoolScratch sc((hipStream_t)stream);
    Prepared prep;
    if ((st = Prepare(sc, source_dev, ns, target_dev, nt, dtype, corres_dev,
                      n_corres, opt, &prep)))
        return st;
    o3dmi_fgr_info_t info = EmptyInfo();
    info.n_initial = n_corres;
    const int64_t* used = corres_dev;
    int64_t n_used = n_corres;
    if (opt->tuple_test) {
        int64_t* tuples = nullptr;
        if ((st = TupleTest(sc, source_dev, ns, target_dev, nt, dtype,
                            corres_dev, n_corres, opt, &tuples, &n_used,
                            &info)))
            return st;
        used = tuples;
    }
    return Finish(sc, prep, source_dev, ns, target_dev, nt, dtype, used,
                  n_used, opt, correspondences_dev, result, &info, info_out);
}

extern "C" int o3dmi_registration_fgr_feature_matching(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, const void* source_features_dev,
        const void* target_features_dev, int dim, int feature_dtype,
        const o3dmi_fgr_options_t* opt, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_fgr_info_t* info_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(result != nullptr && opt != nullptr, "null argument");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    int st = CheckOptions(opt);
    if (st) return st;
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(source_features_dev && target_features_dev && dim > 0,
                  "empty feature set");
    PoolScratch sc((hipStream_t)stream);
    hipStream_t s = sc.s;
    Prepared prep;
    if ((st = Prepare(sc, source_dev, ns, target_dev, nt, dtype, nullptr, 0,
                      opt, &prep)))
        return st;
    o3dmi_fgr_info_t info = EmptyInfo();
    // rule 6: with the tuple test, the larger cloud is the query side
    const bool swapped = opt->tuple_test && ns < nt;
    info.swapped = swapped ? 1 : 0;
    const void* fa = swapped ? target_features_dev : source_features_dev;
    const void* fb = swapped ? source_features_dev : target_features_dev;
    const int64_t na = swapped ? nt : ns, nb = swapped ? ns : nt;
    int32_t* ij = nullptr;
    int32_t* ji = nullptr;
    int64_t* pairs = nullptr;
    int64_t* minfo = nullptr;
    if ((st = sc.Alloc(&ij, 4 * (size_t)na)) ||
        (st = sc.Alloc(&ji, 4 * (size_t)nb)) ||
        (st = sc.Alloc(&pairs, 16 * (size_t)na)) ||
        (st = sc.Alloc(&minfo, 16)))
        return st;
    // rule 2; a negative ratio keeps the cross check for any count: FGR has
    // no fall-back to all pairs
    if ((st = o3dmi_internal_feature_nn1(fa, na, fb, nb, dim, feature_dtype,
                                         ij, stream)) ||
        (st = o3dmi_internal_feature_nn1(fb, nb, fa, na, dim, feature_dtype,
                                         ji, stream)) ||
        (st = o3dmi_internal_feature_mutual(ij, ji, na, 1, -1.0f, pairs, minfo,
                                            stream)))
        return st;
    int64_t hm[2] = {0, 0};
    O3DMI_HIP_CHECK(hipMemcpyAsync(hm, minfo, sizeof(hm),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (hm[0] < 0 || hm[0] > na || hm[1] != 0) {
        SetLastError("fgr: cross check out of range");
        return O3DMI_ERR_INTERNAL;
    }
    info.n_initial = hm[0];
    const int64_t* used = pairs;
    int64_t n_used = hm[0];
    if (opt->tuple_test) {
        int64_t* tuples = nullptr;
        if ((st = TupleTest(sc, swapped ? target_dev : source_dev, na,
                            swapped ? source_dev : target_dev, nb, dtype,
                            pairs, hm[0], opt, &tuples, &n_used, &info)))
            return st;
        if (swapped && (st = FgrSwapPairsAsync(tuples, n_used, s))) return st;
        used = tuples;
    }
    return Finish(sc, prep, source_dev, ns, target_dev, nt, dtype, used,
                  n_used, opt, correspondences_dev, result, &info, info_out);
}
