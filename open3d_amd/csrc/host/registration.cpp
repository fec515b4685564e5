// Host-side ICP driver for the MI355X backend: the control flow of
// t::pipelines::registration::MultiScaleICP (cpp/open3d/t/pipelines/
// registration/Registration.cpp:24-62 ComputeRegistrationResult, :221-273
// pyramid, :275-360 DoSingleScaleICPIterations, :362-444 MultiScaleICP) with
// TransformationEstimationPointToPlane (TransformationEstimation.cpp:196-227),
// re-cut for the GPU:
//
//   reference, per iteration          here, per iteration
//   ------------------------------    -----------------------------------------
//   HybridSearch kernel               one fused kernel: search + sum d2 + count
//   counts.Sum  -> D2H sync             + Jacobian/29-sum accumulation
//   dist.Sum    -> D2H sync           sums posted to a host mailbox by the final
//                                     reduction kernel (no copy / sync call)
//   29-sum kernel -> D2H sync         [optional cross-GPU all-reduce hook]
//   6x6 solve on host (F64)           6x6 solve on host (F64), same arithmetic
//   4x4 upload + transform kernel     the transform rides in the NEXT search
//                                     launch (matrix by value, points moved
//                                     in place before they are searched)
//
// The source cloud is transformed incrementally in its own dtype every
// iteration exactly like the reference (Registration.cpp:322), not re-derived
// from the cumulative transform, so float rounding accumulates the same way.
//
// Other estimators (o3dmi_registration_multiscale_icp_ex): the same fused
// search launch in its point-to-point form (correspondences + raw moments),
// then per estimator: point-to-point -> R, t from the moments on the host;
// symmetric / coloured / Doppler / generalized -> a second launch that gathers
// by correspondence and accumulates their 29 sums (two mailbox waits per
// iteration).
//
// This file: the entry point, which resolves its arguments (the options
// struct among them) and the thread's communicator into an IcpCall
// (icp_driver.h), and below it the index scheduler, the sums fetcher, the
// per-iteration update and the scale loop. Which host call is issued in the
// shadow of which launch is the design: the comments at each say why. The
// pyramids are icp_pyramid.cpp; EvaluateRegistration, GetInformationMatrix and
// ComputeRMSE are registration_eval.cpp.

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../common.h"
#include "../icp.h"
#include "../mailbox.h"
#include "../nns.h"
#include "../collectives.h"
#include "host_util.h"
#include "icp_driver.h"
#include "o3d_mi355x_host.h"

using namespace o3dmi;

namespace {

// The last of a call's description, which needs HIP (the caller holds the
// exit guard). Without a down-sampled finest level the sizes size the
// searches: sizes that live on the device have to come to the host (one small
// copy and wait). Two streams unless there is nothing to overlap (a single
// level without down-sampling is two copies).
int ResolveSizesAndStreams(IcpCall& c) {
    hipStream_t s = c.s;
    const int32_t *ns_dev = c.ns_dev, *nt_dev = c.nt_dev;
    if (c.finest_is_input && (ns_dev || nt_dev)) {
        int32_t host_n[2] = {(int32_t)c.ns, (int32_t)c.nt};
        if (ns_dev)
            O3DMI_HIP_CHECK(hipMemcpyAsync(&host_n[0], ns_dev, sizeof(int32_t),
                                           hipMemcpyDeviceToHost, s));
        if (nt_dev)
            O3DMI_HIP_CHECK(hipMemcpyAsync(&host_n[1], nt_dev, sizeof(int32_t),
                                           hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        O3DMI_REQUIRE(host_n[0] > 0 && host_n[0] <= c.ns && host_n[1] > 0 &&
                              host_n[1] <= c.nt,
                      "Source and/or Target pointcloud is empty.");
        c.ns = host_n[0];
        c.nt = host_n[1];
        c.ns_dev = c.nt_dev = nullptr;
    }
    c.side = s;
    if (c.num_scales > 1 || c.voxel_sizes[c.num_scales - 1] > 0) {
        c.side = SideStream();
        c.ev = SideEvent();
        O3DMI_REQUIRE(c.side != nullptr && c.ev != nullptr,
                      "side stream creation failed");
    }
    return O3DMI_OK;
}

// O3DMI_ICP_TIMING (read per call). Any value: wall time of the whole call
// including the exit path (declare it first: destroyed last) with the marks of
// its phases, one stderr line. Any value but 2: also a line per phase, each
// behind a wait for the stream.
class IcpTimer {
public:
    explicit IcpTimer(hipStream_t s) : s_(s) {
        if (const char* e = std::getenv("O3DMI_ICP_TIMING")) {
            on_ = true;
            phases_ = std::atoi(e) != 2;
            t0_ = t_mark_ = Now();
        }
    }
    ~IcpTimer() {
        if (on_)
            std::fprintf(stderr, "[o3dmi] icp: whole call %.0f us;%s\n",
                         Now() - t0_, marks_.c_str());
    }
    void PyramidBuilt() {
        Mark("pyramid");
        if (!phases_) return;
        std::fprintf(stderr, "[o3dmi] icp: pyramid built in %.0f us\n",
                     Phase());
        t_start_ = t_mark_;
    }
    void ScaleEntered(int scale, int64_t ns, int64_t nt) {
        if (!phases_) return;
        std::fprintf(stderr,
                     "[o3dmi] icp: scale %d (ns %lld nt %lld) index + "
                     "transform %.0f us\n",
                     scale, (long long)ns, (long long)nt, Phase());
    }
    void ScaleDone(int scale, int iterations) {
        Mark("scale");
        if (!phases_) return;
        std::fprintf(stderr, "[o3dmi] icp: scale %d %d iterations %.0f us\n",
                     scale, iterations, Phase());
    }
    void Finished() {
        if (phases_)
            std::fprintf(stderr,
                         "[o3dmi] icp: after pyramid %.0f us in total\n",
                         Now() - t_start_);
        Mark("final");
    }

private:
    static double Now() {
        return std::chrono::duration<double, std::micro>(
                       std::chrono::steady_clock::now().time_since_epoch())
                .count();
    }
    void Mark(const char* what) {
        if (!on_) return;
        char buf[64];
        std::snprintf(buf, sizeof(buf), " %s@%.0f", what, Now() - t0_);
        marks_ += buf;
    }
    // waits for the stream; the time since the previous phase ended
    double Phase() {
        (void)hipStreamSynchronize(s_);
        const double t = Now(), d = t - t_mark_;
        t_mark_ = t;
        return d;
    }
    hipStream_t s_;
    bool on_ = false, phases_ = false;
    double t0_ = 0, t_mark_ = 0, t_start_ = 0;
    std::string marks_;
};

// One index per scale (target_nns.HybridIndex(max_correspondence_distance),
// Registration.cpp:406-412). The first scale's comes with the pyramids
// (BuildPyramids); this issues ALL the later scales' on the side stream in the
// same four launches (round 6, nns.hip BuildIndexMany; up to four per call),
// in the shadow of the first search launch: the sums fetcher calls BuildNext
// between a search launch and the wait for its sums. One build per search
// launch (rounds 2-5) was a fill + three launches + four pool allocations
// each: ~20 us of host time behind an 11 us search -- two late hops per
// tracked frame.
struct IndexScheduler {
    const IcpCall& c;
    const std::vector<Level>& pyr;
    std::vector<NnsGuard>& guards;
    int next = 1;  // first scale whose index is not issued yet
    int status = O3DMI_OK;
    // the event the second scale waits for was recorded behind the last index
    bool on_side = false;

    void BuildNext() {
        while (next < c.num_scales && status == O3DMI_OK) {
            const void* pts[4];
            const void* nrm[4];
            int64_t nn[4];
            double rad[4];
            o3dmi_nns_t* made[4] = {};
            int cnt = 0;
            const int first = next;
            for (; cnt < 4 && next < c.num_scales; ++cnt, ++next) {
                const CloudLevel& Tk = pyr[(size_t)next].target;
                pts[cnt] = Tk.pos;
                nrm[cnt] = c.SearchesPointToPlane() ? Tk.attr[kNormals]
                                                    : nullptr;
                nn[cnt] = Tk.n;
                rad[cnt] = c.max_dists[next];
            }
            status = o3dmi_internal_nns_create_many(
                    cnt, pts, nrm, nn, c.dtype, rad, (o3dmi_stream_t)c.side,
                    made);
            for (int q = 0; q < cnt; ++q)
                guards[(size_t)(first + q)].nns = made[q];
        }
        if (status == O3DMI_OK && c.side != c.s && !on_side && c.num_scales > 1) {
            if (hipEventRecord(c.ev, c.side) != hipSuccess)
                status = O3DMI_ERR_HIP;
            else
                on_side = true;
        }
    }
    // Every index is issued; the caller's stream waits for them (scale 1).
    int Ensure() {
        BuildNext();
        if (status) return status;
        if (on_side) O3DMI_HIP_CHECK(hipStreamWaitEvent(c.s, c.ev, 0));
        return O3DMI_OK;
    }
};

// The iteration's 32 sums, summed over the ranks when the cloud is sharded.
// Per-iteration sums arrive through the thread's host mailbox: the final
// reduction kernel writes them into host-mapped memory and bumps a sequence
// word the host spins on (no copy / stream synchronise call).
// `launch(sums_dev, mail_data, mail_flag, seq)` issues the accumulate +
// final-sum chain. t29..t31: values for out[29..31] (NaN = keep what the
// kernels computed); they are set BEFORE the rank sum.
//   no hook      final sum posts to the host mailbox
//   device hook  final sum -> device buffer -> tail -> caller's collective
//                on the launch stream (RCCL) -> post kernel -> mailbox:
//                one host wait per iteration, nothing staged by the host
//   host hook    as "no hook", then allreduce(host buffer)
//   communicator (o3dmi_set_comm / o3dmi_set_rccl_comm): the device-hook
//                route with the library's own collective (ncclAllReduce
//                on the launch stream) in the hook's place
struct SumsFetcher {
    const IcpCall& c;
    IndexScheduler& indices;
    Mailbox* mb = nullptr;
    bool dev_reduce = false;
    DeviceBuffer dev_sums;

    int Init() {
        mb = ThreadMailbox();
        O3DMI_REQUIRE(mb != nullptr, "host mailbox allocation failed");
        dev_reduce = c.comm != nullptr || c.dev_allreduce != nullptr;
        return dev_reduce ? dev_sums.Alloc(32 * sizeof(double)) : O3DMI_OK;
    }
    // `sealed`: the launch posts through the search launch's final-sum tail
    // (mailbox.h MailboxWaitSealed), else through a final-sum kernel's fenced
    // post.
    template <typename Launch>
    int Fetch(Launch&& launch, double* out32, double t29, double t30,
              double t31, bool sealed = false) {
        const int seq = ++mb->seq;
        if (dev_reduce) {
            double* d = (double*)dev_sums.p;
            int e = launch(d, (double*)nullptr, (int*)nullptr, 0);
            if (e) return e;
            if ((e = o3dmi_internal_sums_tail(d, t29, t30, t31, c.stream())))
                return e;
            if (c.comm) {
                if ((e = c.comm->AllreduceSumF64(d, 32, c.s))) return e;
            } else if (c.dev_allreduce(d, 32, c.stream(), c.dev_allreduce_user) !=
                       0) {
                SetLastError("device all-reduce hook failed");
                return O3DMI_ERR_INVALID_ARG;
            }
            if ((e = o3dmi_internal_sums_post(d, mb->data, mb->flag, seq,
                                              c.stream())))
                return e;
            indices.BuildNext();
            O3DMI_HIP_CHECK(MailboxWait(mb, seq, c.s));
            std::memcpy(out32, mb->data, sizeof(double) * 32);
            return O3DMI_OK;
        }
        int e = launch((double*)nullptr, mb->data, mb->flag, seq);
        if (e) return e;
        indices.BuildNext();  // in the shadow of the launch just issued
        if (sealed) {
            O3DMI_HIP_CHECK(MailboxWaitSealed(mb, seq, c.s, out32));
        } else {
            O3DMI_HIP_CHECK(MailboxWait(mb, seq, c.s));
            std::memcpy(out32, mb->data, sizeof(double) * 32);
        }
        if (t29 == t29) out32[29] = t29;
        if (t30 == t30) out32[30] = t30;
        if (t31 == t31) out32[31] = t31;
        if (c.allreduce && c.allreduce(out32, 32, c.allreduce_user) != 0) {
            SetLastError("all-reduce hook failed");
            return O3DMI_ERR_INVALID_ARG;
        }
        return O3DMI_OK;
    }
};
const double kKeep = std::nan("");

// What this rank works on at a scale: the level's target cloud, and the
// level's source cloud or (level sharding) its slice [first, first + ns) of
// it; the scale's scratch of the estimators with a second launch.
struct ScaleView {
    void *src = nullptr, *srcn = nullptr, *srcc = nullptr;
    // Doppler: directions {ns,3}, the padded dopplers' slice and their
    // {ns,1} form (the scale's scratch); the range check's device word
    void *srcdir = nullptr, *srcdop3 = nullptr, *srcdop = nullptr;
    int* bad = nullptr;
    // generalized: the rows of the level's covariances (the source's: of this
    // rank's slice) and their {n,3,3} form (the scale's scratch)
    void* srccov_rows[3] = {};
    const void* tgtcov_rows[3] = {};
    void *srccov = nullptr, *tgtcov = nullptr;
    int64_t ns = 0, first = 0, nt = 0;
    const void *tgt = nullptr, *nrm = nullptr, *tgtc = nullptr,
               *tgtg = nullptr;
    int64_t* corr = nullptr;
    double* partials = nullptr;
};

void ViewOf(const IcpCall& c, const Level& L, ScaleView& v) {
    const CloudLevel& S = L.source;
    int64_t b = 0, e = S.n;
    if (c.level_sharding) {
        const int64_t base = S.n / c.comm->world, rem = S.n % c.comm->world;
        b = c.comm->rank * base + (c.comm->rank < rem ? c.comm->rank : rem);
        e = b + base + (c.comm->rank < rem ? 1 : 0);
    }
    const size_t off = (size_t)b * 3 * c.esz;
    // (a source level is the driver's own buffer: a clone or a down-sample)
    auto at = [off](void* p) { return p ? (char*)p + off : nullptr; };
    v.src = at(S.pos_buf.p);
    v.srcn = at(S.attr_buf[kNormals].p);
    v.srcc = at(S.attr_buf[kColors].p);
    v.srcdir = at(S.attr_buf[kDirections].p);
    v.srcdop3 = at(S.attr_buf[kDopplers].p);
    for (int r = 0; r < 3; ++r) {
        v.srccov_rows[r] = at(S.attr_buf[kCovRow0 + r].p);
        v.tgtcov_rows[r] = L.target.attr[kCovRow0 + r];
    }
    v.ns = e - b;
    v.first = b;
    v.tgt = L.target.pos;
    v.nrm = L.target.attr[kNormals];
    v.tgtc = L.target.attr[kColors];
    v.tgtg = L.target.attr[kGradients];
    v.nt = L.target.n;
}

// The scale's scratch of the estimators that gather by correspondence, issued
// on the call's stream in this order: Doppler -- the level's dopplers as
// {ns,1}; generalized -- the level's covariances as {n,3,3}, the source's
// slice and the target's; behind either the range check's zeroed word; then
// the correspondence set and the rows of partial sums.
struct ScaleScratch {
    DeviceBuffer corr, partials, tables;

    int Prepare(const IcpCall& c, ScaleView& L) {
        if (!c.GathersByCorrespondence()) return O3DMI_OK;
        int e;
        auto round8 = [](size_t bytes) { return (bytes + 7) / 8 * 8; };
        // `bytes` of tables and, behind them, L.bad, zeroed
        auto alloc_tables = [&](size_t bytes) -> int {
            int st = tables.Alloc(bytes + sizeof(int));
            if (st) return st;
            L.bad = (int*)((char*)tables.p + bytes);
            O3DMI_HIP_CHECK(hipMemsetAsync(L.bad, 0, sizeof(int), c.s));
            return O3DMI_OK;
        };
        if (c.Is(O3DMI_ICP_DOPPLER)) {
            if ((e = alloc_tables(round8((size_t)L.ns * c.esz)))) return e;
            L.srcdop = tables.p;
            if ((e = o3dmi_internal_take_column(L.srcdop3, L.ns, c.dtype,
                                                L.srcdop, c.stream())))
                return e;
        } else if (c.Is(O3DMI_ICP_GENERALIZED)) {
            const size_t so = round8((size_t)L.ns * 9 * c.esz);
            const size_t to = round8((size_t)L.nt * 9 * c.esz);
            if ((e = alloc_tables(so + to))) return e;
            L.srccov = tables.p;
            L.tgtcov = (char*)tables.p + so;
            if ((e = o3dmi_internal_join_rows3(
                         L.srccov_rows[0], L.srccov_rows[1], L.srccov_rows[2],
                         L.ns, c.dtype, L.srccov, c.stream())))
                return e;
            if ((e = o3dmi_internal_join_rows3(
                         L.tgtcov_rows[0], L.tgtcov_rows[1], L.tgtcov_rows[2],
                         L.nt, c.dtype, L.tgtcov, c.stream())))
                return e;
        }
        if ((e = corr.Alloc(sizeof(int64_t) * (size_t)L.ns))) return e;
        if ((e = partials.Alloc(sizeof(double) * 32 * kIcpPartialRows)))
            return e;
        L.corr = (int64_t*)corr.p;
        L.partials = (double*)partials.p;
        return O3DMI_OK;
    }
};

// The transformation the source still has to be moved by
// (`source.Transform(...)`, Registration.cpp:322,404) -- applied by the NEXT
// search launch itself, in place, before it searches.
struct PendingTransform {
    double m[16];
    bool set = false;
    void Set(const double* T) {
        std::memcpy(m, T, sizeof(m));
        set = true;
    }
    const double* Take() {
        const double* xf = set ? m : nullptr;
        set = false;
        return xf;
    }
};

struct SearchResult {
    double fitness = 0, inlier_rmse = 0;
    double sums[32];
};

// ComputeRegistrationResult (+ the Jacobian sums of the same pass).
int Search(const IcpCall& c, SumsFetcher& sums, o3dmi_nns_t* nns,
           const ScaleView& L, PendingTransform& pending, int64_t* corr_out,
           SearchResult& r) {
    const double* xf = pending.Take();
    // the fused search kernel accumulates the point-to-plane terms itself;
    // the other estimators take the point-to-point moments from it
    const int search_mode = c.SearchesPointToPlane() ? 0 : 1;
    int e = sums.Fetch(
            [&](double* sums_dev, double* mail_data, int* mail_flag, int seq) {
                return o3dmi_internal_icp_transform_search_accumulate(
                        nns, L.src, xf, nullptr, L.ns, search_mode,
                        c.robust_kernel, c.scaling_parameter,
                        c.shape_parameter, corr_out, sums_dev, mail_data,
                        mail_flag, seq, c.stream());
            },
            r.sums, kKeep, kKeep, (double)L.ns, /*sealed=*/true);
    if (e) return e;
    const double num_correspondences = r.sums[30];
    // (else "0 correspondence present between the pointclouds.": r's zeros)
    if (num_correspondences != 0) {
        const double squared_error = r.sums[29];
        r.fitness = num_correspondences / r.sums[31];
        r.inlier_rmse = std::sqrt(squared_error / num_correspondences);
    }
    return O3DMI_OK;
}

// What ComputePoseDopplerICP (kernel/Registration.cpp:222-265) prepares on the
// host for iteration `iteration` of a scale with the cumulative transformation
// `current`: the kernels and the rejection in force, and the vehicle's angular
// and linear velocity from TransformationToPose(current) -- the pose in
// float64, cast to the point dtype, negated and divided by the period there
// (Tensor::Div(Scalar) casts the scalar to the tensor's dtype first).
int DopplerSums(const IcpCall& c, SumsFetcher& sums, const ScaleView& L,
                const double* current, int iteration, double* out32) {
    const o3dmi_icp_doppler_t& d = c.dop;
    const bool robust_g = iteration >= d.geometric_robust_loss_min_iteration;
    const bool robust_d = iteration >= d.doppler_robust_loss_min_iteration;
    const int reject = d.reject_dynamic_outliers &&
                       iteration >= d.outlier_rejection_min_iteration;
    double state[6], w_v_in_V[3], v_v_in_V[3];
    o3dmi_transformation_to_pose(current, state);
    for (int k = 0; k < 3; ++k) {
        if (c.dtype == O3DMI_F32) {
            const float period = (float)d.period;
            w_v_in_V[k] = (double)(-(float)state[k] / period);
            v_v_in_V[k] = (double)(-(float)state[3 + k] / period);
        } else {
            w_v_in_V[k] = -state[k] / d.period;
            v_v_in_V[k] = -state[3 + k] / d.period;
        }
    }
    int e = sums.Fetch(
            [&](double* sums_dev, double* mail_data, int* mail_flag, int seq) {
                return o3dmi_icp_doppler_accumulate_post(
                        L.src, L.srcdop, L.srcdir, L.tgt, L.nrm, L.corr, L.ns,
                        L.nt, c.dtype, c.R_S_to_V, c.r_v_to_s_in_V, w_v_in_V,
                        v_v_in_V, d.period, reject, d.doppler_outlier_threshold,
                        robust_g ? d.geometric_kernel : O3DMI_L2_LOSS,
                        robust_g ? d.geometric_scaling_parameter : 1.0,
                        robust_g ? d.geometric_shape_parameter : 1.0,
                        robust_d ? d.doppler_kernel : O3DMI_L2_LOSS,
                        robust_d ? d.doppler_scaling_parameter : 1.0,
                        robust_d ? d.doppler_shape_parameter : 1.0,
                        d.lambda_doppler, sums_dev, L.partials, L.bad,
                        mail_data, mail_flag, seq, c.stream());
            },
            out32, 0.0, 0.0, 0.0);
    if (e) return e;
    // (the checked final pass posts NaN for an index outside the target)
    O3DMI_REQUIRE(out32[28] == out32[28],
                  "correspondence index out of range");
    return O3DMI_OK;
}

// TransformationEstimationForGeneralizedICP::ComputeTransformation up to the
// solve (GeneralizedICP.cpp:104-147). The level's source positions stand at
// `current`, its covariance tables as they were built: the rotation of
// `current` goes to the kernel (the reference rotates the covariances with
// every Transform, PointCloud.cpp). out32[29]: the pairs that could not be
// whitened.
int GeneralizedSums(const IcpCall& c, SumsFetcher& sums, const ScaleView& L,
                    const double* current, double* out32) {
    double R[9];
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) R[j * 3 + k] = current[j * 4 + k];
    int e = sums.Fetch(
            [&](double* sums_dev, double* mail_data, int* mail_flag, int seq) {
                return o3dmi_icp_generalized_accumulate_post(
                        L.src, L.srccov, L.tgt, L.tgtcov, L.corr, L.ns, L.nt,
                        c.dtype, R, c.gen.robust_kernel,
                        c.gen.scaling_parameter, c.gen.shape_parameter, 0,
                        sums_dev, L.partials, L.bad, mail_data, mail_flag, seq,
                        c.stream());
            },
            out32, kKeep, 0.0, 0.0);
    if (e) return e;
    O3DMI_REQUIRE(out32[28] == out32[28],
                  "correspondence index out of range");
    return O3DMI_OK;
}

// ComputeTransformationSymmetric up to the solve, kernel/Registration.cpp:
// 80-135: the means of the matched points (from the search pass' moments, in
// the clouds' dtype) and the 29 sums about them.
int SymmetricSums(const IcpCall& c, SumsFetcher& sums, const ScaleView& L,
                  const SearchResult& r, double* ms, double* mt,
                  double* out32) {
    const double cnt = r.sums[15];
    for (int k = 0; k < 3; ++k) {
        ms[k] = r.sums[k] / cnt;
        mt[k] = r.sums[3 + k] / cnt;
        if (c.dtype == O3DMI_F32) {
            ms[k] = (double)(float)ms[k];
            mt[k] = (double)(float)mt[k];
        }
    }
    return sums.Fetch(
            [&](double* sums_dev, double* mail_data, int* mail_flag, int seq) {
                return o3dmi_icp_symmetric_accumulate_post(
                        L.src, L.srcn, L.tgt, L.nrm, L.corr, L.ns, c.dtype, ms,
                        mt, c.robust_kernel, c.scaling_parameter,
                        c.shape_parameter, sums_dev, L.partials, mail_data,
                        mail_flag, seq, c.stream());
            },
            out32, 0.0, 0.0, 0.0);
}

// ComputePoseColoredICP (TransformationEstimation.cpp:420-432).
int ColoredSums(const IcpCall& c, SumsFetcher& sums, const ScaleView& L,
                double* out32) {
    return sums.Fetch(
            [&](double* sums_dev, double* mail_data, int* mail_flag, int seq) {
                return o3dmi_icp_colored_accumulate_post(
                        L.src, L.srcc, L.tgt, L.nrm, L.tgtc, L.tgtg, L.corr,
                        L.ns, c.dtype, c.lambda_geometric, c.robust_kernel,
                        c.scaling_parameter, c.shape_parameter, sums_dev,
                        L.partials, mail_data, mail_flag, seq, c.stream());
            },
            out32, 0.0, 0.0, 0.0);
}

// One iteration's update from its search: estimation.ComputeTransformation,
// Registration.cpp:314, in three steps. Point-to-point: R, t from the search
// pass' moments, and done. The others: their 29 sums -- point-to-plane: of the
// search pass; symmetric / coloured / Doppler / generalized: of a second
// launch that gathers by correspondence -- then the 6x6 solve and pose ->
// transformation (symmetric: the half-angle form about the means).
// *solve_status: a failed solve (the reference throws; the driver reports it
// after the loop); a returned error ends the call at once.
// `current`, `iteration`: the cumulative transformation before this update and
// the iteration's index within its scale (read by the Doppler and the
// generalized estimator only). *singular_pairs: the generalized estimator's
// count of pairs that could not be whitened.
int ComputeUpdate(const IcpCall& c, SumsFetcher& sums, const ScaleView& L,
                  const SearchResult& r, const double* current, int iteration,
                  double* update, int* solve_status, int64_t* singular_pairs) {
    if (c.Is(O3DMI_ICP_POINT_TO_POINT)) {
        // ComputeRtPointToPoint + RtToTransformation
        // (TransformationEstimation.cpp:150-159)
        double R[9], t[3];
        int e = o3dmi_compute_rt_p2point(r.sums, R, t);
        if (e) return e;
        Eye4(update);
        for (int j = 0; j < 3; ++j) {
            for (int k = 0; k < 3; ++k) update[j * 4 + k] = R[j * 3 + k];
            update[j * 4 + 3] = t[j];
        }
        return O3DMI_OK;
    }
    double gathered[32], ms[3], mt[3];
    int e = O3DMI_OK;
    switch (c.estimation) {
        case O3DMI_ICP_SYMMETRIC:
            e = SymmetricSums(c, sums, L, r, ms, mt, gathered);
            break;
        case O3DMI_ICP_COLORED:
            e = ColoredSums(c, sums, L, gathered);
            break;
        case O3DMI_ICP_DOPPLER:
            // ComputePoseDopplerICP (TransformationEstimation.cpp:469-519)
            e = DopplerSums(c, sums, L, current, iteration, gathered);
            break;
        case O3DMI_ICP_GENERALIZED:
            e = GeneralizedSums(c, sums, L, current, gathered);
            if (!e) *singular_pairs = (int64_t)gathered[29];
            break;
    }
    if (e) return e;
    // (point-to-plane: the search pass' own sums)
    const double* sums29 = c.GathersByCorrespondence() ? gathered : r.sums;
    double pose[6];
    float residual;
    int inlier_count;
    e = o3dmi_decode_and_solve6x6(sums29, pose, &residual, &inlier_count);
    if (e) *solve_status = e;
    if (c.Is(O3DMI_ICP_SYMMETRIC))
        o3dmi_symmetric_pose_to_transformation(pose, ms, mt, update);
    else
        o3dmi_pose_to_transformation(pose, update);
    return O3DMI_OK;
}

// What the scales hand on to each other, and the result in the making.
struct IcpState {
    double T[16];
    double fitness = 0, inlier_rmse = 0;
    bool converged = false;
    int iteration_count = 0;
    int status = O3DMI_OK;  // of a failed 6x6 solve: reported after the loop
    int64_t singular_pairs = 0;  // generalized: of the last accumulate
    PendingTransform pending;
};

// DoSingleScaleICPIterations, Registration.cpp:275-360. *iterations: the
// scale's `it` when the loop ended.
// (Rounds 3-4 carried two more forms of the point-to-plane loop, both
// bit-compatible and both measured slower -- the 6x6 solve in the search
// launch's last workgroup with the host one launch ahead, and a next
// launch queued ahead and gated on a host inbox: docs/rounds.md. What
// stayed of them is the final sum in the search launch's last workgroup,
// icp.hip SumTail.)
int RunScaleIterations(const IcpCall& c, SumsFetcher& sums, NnsGuard& guard,
                       const ScaleView& L, int scale_idx, IcpState& st,
                       int* iterations) {
    int e;
    double prev_fitness = st.fitness, prev_inlier_rmse = st.inlier_rmse;
    st.converged = false;
    const o3dmi_icp_criteria_t& crit = c.criterias[scale_idx];
    int& it = *iterations;
    for (it = 0; it < crit.max_iteration; ++it) {
        SearchResult r;
        // (an error path still pays the index's device-wide wait)
        guard.completed = false;
        if ((e = Search(c, sums, guard.nns, L, st.pending, L.corr, r)))
            return e;
        guard.completed = true;  // its sums were read: the search is done
        st.fitness = r.fitness;
        st.inlier_rmse = r.inlier_rmse;
        if (r.sums[30] == 0) Eye4(st.T);  // Registration.cpp:56-58
        if (st.fitness <= std::numeric_limits<double>::min()) break;
        double update[16];
        if ((e = ComputeUpdate(c, sums, L, r, st.T, it, update, &st.status,
                               &st.singular_pairs)))
            return e;
        Matmul4(update, st.T, st.T);
        // source.Transform(update): rides in the next search launch of
        // this scale (a scale that ends here has no further use for its
        // source cloud)
        st.pending.Set(update);
        if (c.Is(O3DMI_ICP_SYMMETRIC) &&
            (e = o3dmi_transform_normals(update, L.srcn, L.ns, c.dtype,
                                         c.stream())))
            return e;
        if (c.callback)
            c.callback(st.iteration_count + it, scale_idx, it, st.inlier_rmse,
                       st.fitness, st.T, c.callback_user);
        if (it != 0 &&
            std::abs(prev_fitness - st.fitness) < crit.relative_fitness &&
            std::abs(prev_inlier_rmse - st.inlier_rmse) < crit.relative_rmse) {
            st.converged = true;
            break;
        }
        prev_fitness = st.fitness;
        prev_inlier_rmse = st.inlier_rmse;
    }
    st.iteration_count += it;
    return O3DMI_OK;
}

// MultiScaleICP, Registration.cpp:362-444, for a resolved call. The caller
// owns what has to outlive this frame, in the order of their destruction.
int RunIcp(const IcpCall& c, IcpTimer& timer, std::vector<Level>& pyr,
           SyncOnExit& sync_on_exit, std::vector<NnsGuard>& guards,
           const double* init, int64_t* correspondences_dev,
           o3dmi_registration_result_t* result) {
    int e;
    if ((e = BuildPyramids(c, pyr, guards[0]))) return e;
    timer.PyramidBuilt();
    IndexScheduler indices{c, pyr, guards};
    SumsFetcher sums{c, indices};
    if ((e = sums.Init())) return e;

    IcpState st;
    if (init) std::memcpy(st.T, init, sizeof(st.T));
    else Eye4(st.T);
    int64_t last_ns = 0;
    for (int scale_idx = 0; scale_idx < c.num_scales; ++scale_idx) {
        const Level& full_level = pyr[(size_t)scale_idx];
        ScaleView L;
        ViewOf(c, full_level, L);
        last_ns = L.ns;
        // source_down_pyramid[scale].Transform(result.transformation_) :404
        // (positions and, when the estimator reads them, normals)
        st.pending.Set(st.T);
        if (c.Is(O3DMI_ICP_SYMMETRIC) &&
            (e = o3dmi_transform_normals(st.T, L.srcn, L.ns, c.dtype,
                                         c.stream())))
            return e;
        ScaleScratch scratch;
        if ((e = scratch.Prepare(c, L))) return e;
        // target_nns.HybridIndex(max_correspondence_distance) :406-412:
        // built behind the target pyramid, the later scales' in the shadow of
        // the first scale's searches
        NnsGuard& guard = guards[(size_t)scale_idx];
        if (scale_idx == 1 && (e = indices.Ensure())) return e;
        timer.ScaleEntered(scale_idx, L.ns, L.nt);

        int it = 0;
        if ((e = RunScaleIterations(c, sums, guard, L, scale_idx, st, &it)))
            return e;
        timer.ScaleDone(scale_idx, it);

        if (scale_idx == c.num_scales - 1) {
            // Final fitness / rmse for the stored transformation :424-431
            SearchResult r;
            // level sharding: this rank fills its rows of the level's
            // correspondence set, the others read -1 here
            if (c.level_sharding && correspondences_dev)
                O3DMI_HIP_CHECK(hipMemsetAsync(
                        correspondences_dev, 0xFF,
                        sizeof(int64_t) * (size_t)full_level.source.n, c.s));
            if (c.level_sharding) last_ns = full_level.source.n;
            if ((e = Search(c, sums, guard.nns, L, st.pending,
                            correspondences_dev ? correspondences_dev + L.first
                                                : nullptr,
                            r)))
                return e;
            st.fitness = r.fitness;
            st.inlier_rmse = r.inlier_rmse;
            if (r.sums[30] == 0) Eye4(st.T);
            // the search above waited for its sums: nothing of this call is
            // in flight any more (every scale's index was waited for by the
            // scale's first search)
            sync_on_exit.drained = true;
        }
        if (st.fitness <= std::numeric_limits<double>::min()) {
            st.converged = false;
            break;
        }
    }

    timer.Finished();
    std::memcpy(result->transformation, st.T, sizeof(st.T));
    result->fitness = st.fitness;
    result->inlier_rmse = st.inlier_rmse;
    result->converged = st.converged ? 1 : 0;
    result->num_iterations = st.iteration_count;
    result->num_correspondences = correspondences_dev ? last_ns : 0;
    if (c.Is(O3DMI_ICP_GENERALIZED) && c.gen.singular_pairs_out)
        *c.gen.singular_pairs_out = st.singular_pairs;
    return st.status;
}

}  // namespace

extern "C" int o3dmi_registration_multiscale_icp(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_dists, const double* init, int robust_kernel,
        double scaling_parameter, double shape_parameter,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream) {
    return o3dmi_registration_multiscale_icp_ex(
            source_dev, ns, target_dev, target_normals_dev, nt, dtype,
            num_scales, voxel_sizes, criterias, max_dists, init,
            O3DMI_ICP_POINT_TO_PLANE, nullptr, nullptr, robust_kernel,
            scaling_parameter, shape_parameter, callback, callback_user,
            allreduce, allreduce_user, correspondences_dev, result, stream);
}

namespace {

// TransformationEstimationForDopplerICP's constructor and argument checks
// (TransformationEstimation.h:356-500, TransformationEstimation.cpp:469-499)
// and what ComputePoseDopplerICP takes from transform_vehicle_to_sensor.
int ResolveDoppler(IcpCall& c, const o3dmi_icp_doppler_t* doppler) {
    O3DMI_REQUIRE(doppler != nullptr, "doppler is null");
    c.dop = *doppler;
    o3dmi_icp_doppler_t& d = c.dop;
    O3DMI_REQUIRE(d.source_dopplers != nullptr,
                  "DopplerICP requires source pointcloud to have Doppler "
                  "velocities.");
    O3DMI_REQUIRE(d.source_directions != nullptr,
                  "DopplerICP requires source pointcloud to have pre-computed "
                  "direction vectors.");
    O3DMI_REQUIRE(d.period > 0, "period must be positive");
    if (!(d.lambda_doppler >= 0 && d.lambda_doppler <= 1.0))
        d.lambda_doppler = 0.01;
    O3DMI_REQUIRE(d.geometric_kernel >= 0 && d.geometric_kernel <= 6 &&
                          d.doppler_kernel >= 0 && d.doppler_kernel <= 6,
                  "Unsupported method.");
    if (d.reject_dynamic_outliers && (d.geometric_kernel == O3DMI_L1_LOSS ||
                                      d.doppler_kernel == O3DMI_L1_LOSS)) {
        SetLastError(
                "Doppler ICP: dynamic outlier rejection with an L1Loss kernel "
                "is not supported");
        return O3DMI_ERR_UNSUPPORTED;
    }
    double* V = d.transform_vehicle_to_sensor;
    bool all_zero = true;
    for (int k = 0; k < 16; ++k) {
        O3DMI_REQUIRE(std::isfinite(V[k]),
                      "transform_vehicle_to_sensor is not finite");
        all_zero = all_zero && V[k] == 0;
    }
    if (all_zero) Eye4(V);
    // R_S_to_V = inverse of the rotation block, float64 (cofactors over the
    // determinant; the reference calls LAPACK getrf + getri)
    const double a = V[0], b = V[1], cc = V[2], dd = V[4], ee = V[5], f = V[6],
                 g = V[8], h = V[9], i = V[10];
    const double det = a * (ee * i - f * h) - b * (dd * i - f * g) +
                       cc * (dd * h - ee * g);
    O3DMI_REQUIRE(det != 0 && std::isfinite(1.0 / det),
                  "transform_vehicle_to_sensor has a singular rotation");
    double* R = c.R_S_to_V;
    R[0] = (ee * i - f * h) / det;
    R[1] = (cc * h - b * i) / det;
    R[2] = (b * f - cc * ee) / det;
    R[3] = (f * g - dd * i) / det;
    R[4] = (a * i - cc * g) / det;
    R[5] = (cc * dd - a * f) / det;
    R[6] = (dd * h - ee * g) / det;
    R[7] = (b * g - a * h) / det;
    R[8] = (a * ee - b * dd) / det;
    c.r_v_to_s_in_V[0] = V[3];
    c.r_v_to_s_in_V[1] = V[7];
    c.r_v_to_s_in_V[2] = V[11];
    c.source_directions = d.source_directions;
    return O3DMI_OK;
}

// TransformationEstimationForGeneralizedICP's constructor and argument checks.
int ResolveGeneralized(IcpCall& c, const o3dmi_icp_generalized_t* generalized,
                       const void* target_normals_dev) {
    O3DMI_REQUIRE(generalized != nullptr, "generalized is null");
    c.gen = *generalized;
    O3DMI_REQUIRE(c.gen.epsilon > 0 && std::isfinite(c.gen.epsilon),
                  "epsilon must be positive and finite");
    O3DMI_REQUIRE(c.gen.robust_kernel >= 0 && c.gen.robust_kernel <= 6,
                  "Unsupported method.");
    const bool estimate_source =
            !c.gen.source_covariances && !c.gen.source_normals;
    const bool estimate_target =
            !c.gen.target_covariances && !target_normals_dev;
    if ((estimate_source && c.ns_dev) || (estimate_target && c.nt_dev))
        return Unsupported(
                "Generalized ICP: normals cannot be estimated for a cloud "
                "whose size lives on the device");
    return O3DMI_OK;
}

// InitializePointCloudForGeneralizedICP (GeneralizedICP.cpp:52-80) for one
// cloud, on the call's stream: covariances given -> as they are; else from the
// given normals; else from EstimateNormals(KNN 20). `rows`: the three {n,3}
// row tables the pyramid carries.
int GeneralizedCovarianceRows(const IcpCall& c, const void* points, int64_t n,
                              const void* covariances, const void* normals,
                              DeviceBuffer& rows, const void** rows_out) {
    int e;
    DeviceBuffer own_normals, own_cov;
    if (!covariances) {
        if (!normals) {
            if ((e = own_normals.Alloc((size_t)n * 3 * c.esz))) return e;
            if ((e = o3dmi_pointcloud_estimate_normals(
                         points, n, c.dtype, 20, -1.0, own_normals.p, 0,
                         c.stream())))
                return e;
            normals = own_normals.p;
        }
        if ((e = own_cov.Alloc((size_t)n * 9 * c.esz))) return e;
        if ((e = o3dmi_pointcloud_covariances_from_normals(
                     normals, n, c.dtype, c.gen.epsilon, own_cov.p,
                     c.stream())))
            return e;
        covariances = own_cov.p;
    }
    const size_t row = (size_t)n * 3 * c.esz;
    if ((e = rows.Alloc(3 * row))) return e;
    for (int r = 0; r < 3; ++r) rows_out[r] = (char*)rows.p + r * row;
    e = o3dmi_internal_split_rows3(covariances, n, c.dtype,
                                   (void*)rows_out[0], (void*)rows_out[1],
                                   (void*)rows_out[2], c.stream());
    // (the temporaries above go back to the pool here)
    if (hipStreamSynchronize(c.s) != hipSuccess && !e) e = O3DMI_ERR_HIP;
    return e;
}

// The entry points: `doppler` != NULL is O3DMI_ICP_DOPPLER, `generalized`
// != NULL O3DMI_ICP_GENERALIZED.
int MultiScaleIcpEntry(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_dists, const double* init, int estimation,
        const o3dmi_icp_attributes_t* attrs, const o3dmi_icp_doppler_t* doppler,
        const o3dmi_icp_generalized_t* generalized,
        const o3dmi_icp_options_t* options, int robust_kernel,
        double scaling_parameter, double shape_parameter,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream) {
    IcpCall c;
    // the thread's communicator; a world of one rank counts as none
    c.comm = ThreadComm();
    if (c.comm && c.comm->world <= 1) c.comm = nullptr;
    if (options) {
        c.ns_dev = options->ns_dev;
        c.nt_dev = options->nt_dev;
        c.dev_allreduce = options->device_allreduce;
        c.dev_allreduce_user = options->device_allreduce_user;
        c.level_sharding = c.comm != nullptr && options->level_sharding != 0;
    }
    // AssertInputMultiScaleICP, Registration.cpp:119-219.
    O3DMI_REQUIRE(result != nullptr, "result is null");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    c.estimation = estimation;
    const bool symmetric = c.Is(O3DMI_ICP_SYMMETRIC),
               colored = c.Is(O3DMI_ICP_COLORED);
    c.source = source_dev;
    c.target = target_dev;
    c.target_normals = c.NeedsTargetNormals() ? target_normals_dev : nullptr;
    if (symmetric && attrs) c.source_normals = attrs->source_normals;
    if (colored && attrs) {
        c.source_colors = attrs->source_colors;
        c.target_colors = attrs->target_colors;
        c.target_gradients = attrs->target_color_gradients;
        c.lambda_geometric = attrs->lambda_geometric;
    }
    // TransformationEstimationForColoredICP ctor, TransformationEstimation.h:
    // 293-299
    if (!(c.lambda_geometric >= 0 && c.lambda_geometric <= 1.0))
        c.lambda_geometric = 0.968;
    O3DMI_REQUIRE(!(c.SearchesPointToPlane() || colored) ||
                          c.target_normals != nullptr,
                  "Target pointcloud missing normals attribute.");
    O3DMI_REQUIRE(!c.Is(O3DMI_ICP_DOPPLER) || c.target_normals != nullptr,
                  "DopplerICP requires target pointcloud to have normals.");
    if (c.Is(O3DMI_ICP_DOPPLER)) {
        int e = ResolveDoppler(c, doppler);
        if (e) return e;
    }
    if (c.Is(O3DMI_ICP_GENERALIZED)) {
        int e = ResolveGeneralized(c, generalized, target_normals_dev);
        if (e) return e;
    }
    O3DMI_REQUIRE(!symmetric || (c.source_normals && c.target_normals),
                  "SymmetricICP requires both source and target to have "
                  "normals.");
    O3DMI_REQUIRE(!colored || (c.source_colors && c.target_colors),
                  "Source and/or Target pointcloud missing colors attribute.");
    O3DMI_REQUIRE(num_scales > 0 && voxel_sizes && criterias && max_dists,
                  "Size of criterias, voxel_size, max_correspondence_distances "
                  "vectors must be same.");
    for (int i = 0; i < num_scales; ++i) {
        O3DMI_REQUIRE(max_dists[i] > 0,
                      "max_correspondence_distance must be positive");
        if (i + 1 < num_scales)
            O3DMI_REQUIRE(voxel_sizes[i + 1] <= 0 ||
                                  voxel_sizes[i] > voxel_sizes[i + 1],
                          "Decreasing order of voxel_sizes is required.");
    }
    c.dtype = dtype;
    c.esz = dtype == O3DMI_F64 ? 8 : 4;
    c.s = (hipStream_t)stream;
    c.ns = ns;
    c.nt = nt;
    c.num_scales = num_scales;
    c.voxel_sizes = voxel_sizes;
    c.criterias = criterias;
    c.max_dists = max_dists;
    c.finest_is_input = voxel_sizes[num_scales - 1] <= 0;
    c.robust_kernel = robust_kernel;
    c.scaling_parameter = scaling_parameter;
    c.shape_parameter = shape_parameter;
    c.callback = callback;
    c.callback_user = callback_user;
    c.allreduce = allreduce;
    c.allreduce_user = allreduce_user;
    IcpTimer timer(c.s);  // (declared first: destroyed last)
    std::vector<Level> pyr((size_t)num_scales);
    DeviceBuffer dopplers3;  // the caller's {ns,1} dopplers as column 0 of {ns,3}
    DeviceBuffer source_cov_rows, target_cov_rows;  // generalized
    // Declared after the pyramid so that it runs first on every exit path.
    SyncOnExit sync_on_exit{c.s};
    std::vector<NnsGuard> guards((size_t)num_scales);
    int st = ResolveSizesAndStreams(c);
    sync_on_exit.side = c.side;
    if (st) return st;
    if (c.Is(O3DMI_ICP_DOPPLER)) {
        if ((st = dopplers3.Alloc((size_t)c.ns * 3 * c.esz))) return st;
        if ((st = o3dmi_internal_pad_column(c.dop.source_dopplers, c.ns,
                                            c.dtype, dopplers3.p, c.stream())))
            return st;
        c.source_dopplers3 = dopplers3.p;
    }
    if (c.Is(O3DMI_ICP_GENERALIZED)) {
        if ((st = GeneralizedCovarianceRows(
                     c, c.source, c.ns, c.gen.source_covariances,
                     c.gen.source_normals, source_cov_rows,
                     c.source_cov_rows)))
            return st;
        if ((st = GeneralizedCovarianceRows(
                     c, c.target, c.nt, c.gen.target_covariances,
                     target_normals_dev, target_cov_rows, c.target_cov_rows)))
            return st;
    }
    return RunIcp(c, timer, pyr, sync_on_exit, guards, init,
                  correspondences_dev, result);
}

}  // namespace

extern "C" int o3dmi_registration_multiscale_icp_ex(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_dists, const double* init, int estimation,
        const o3dmi_icp_attributes_t* attrs, const o3dmi_icp_options_t* options,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream) {
    // (Doppler ICP's parameters travel in o3dmi_icp_doppler_t:
    // o3dmi_registration_multiscale_icp_doppler; generalized ICP's in
    // o3dmi_icp_generalized_t: o3dmi_registration_multiscale_icp_generalized)
    O3DMI_REQUIRE(estimation >= O3DMI_ICP_POINT_TO_PLANE &&
                          estimation <= O3DMI_ICP_COLORED,
                  "estimation must be point-to-plane, point-to-point, "
                  "symmetric or colored");
    return MultiScaleIcpEntry(
            source_dev, ns, target_dev, target_normals_dev, nt, dtype,
            num_scales, voxel_sizes, criterias, max_dists, init, estimation,
            attrs, nullptr, nullptr, options, robust_kernel, scaling_parameter,
            shape_parameter, callback, callback_user, allreduce,
            allreduce_user, correspondences_dev, result, stream);
}

extern "C" int o3dmi_registration_multiscale_icp_doppler(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_dists, const double* init,
        const o3dmi_icp_doppler_t* doppler, const o3dmi_icp_options_t* options,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(doppler != nullptr, "doppler is null");
    return MultiScaleIcpEntry(
            source_dev, ns, target_dev, target_normals_dev, nt, dtype,
            num_scales, voxel_sizes, criterias, max_dists, init,
            O3DMI_ICP_DOPPLER, nullptr, doppler, nullptr, options,
            O3DMI_L2_LOSS, 1.0, 1.0, callback, callback_user, allreduce,
            allreduce_user, correspondences_dev, result, stream);
}

extern "C" int o3dmi_registration_multiscale_icp_generalized(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_dists, const double* init,
        const o3dmi_icp_generalized_t* generalized,
        const o3dmi_icp_options_t* options, o3dmi_icp_callback_t callback,
        void* callback_user, o3dmi_allreduce_sum_t allreduce,
        void* allreduce_user, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(generalized != nullptr, "generalized is null");
    return MultiScaleIcpEntry(
            source_dev, ns, target_dev, target_normals_dev, nt, dtype,
            num_scales, voxel_sizes, criterias, max_dists, init,
            O3DMI_ICP_GENERALIZED, nullptr, nullptr, generalized, options,
            O3DMI_L2_LOSS, 1.0, 1.0, callback, callback_user, allreduce,
            allreduce_user, correspondences_dev, result, stream);
}
