// EvaluateRegistration and GetInformationMatrix (Registration.cpp:64-91,
// 446-486) and the estimators' ComputeRMSE for the MI355X backend: one fused
// search + sums pass each (icp.hip), no iteration.

#include <cmath>
#include <cstring>

#include "../common.h"
#include "../icp.h"
#include "../mailbox.h"
#include "../nns.h"
#include "host_util.h"
#include "o3d_mi355x_host.h"

using namespace o3dmi;

namespace {

// Shared front end of EvaluateRegistration / GetInformationMatrix: clone +
// transform the source, index the target, one fused search + sums pass.
int TransformSearch(const void* source_dev, int64_t ns, const void* target_dev,
                    int64_t nt, int dtype, double max_dist, const double* T,
                    int estimation, int64_t* corr_dev, double* sums32,
                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(max_dist > 0, "max_correspondence_distance must be positive");
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = dtype == O3DMI_F64 ? 8 : 4;
    DeviceBuffer src;
    SyncOnExit sync_on_exit{s};
    int st;
    if ((st = src.Alloc((size_t)ns * 3 * esz))) return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(src.p, source_dev, (size_t)ns * 3 * esz,
                                   hipMemcpyDeviceToDevice, s));
    if (T && (st = o3dmi_transform_points(T, src.p, ns, dtype, stream)))
        return st;
    NnsGuard guard;
    if ((st = o3dmi_nns_create(target_dev, nt, dtype, max_dist, stream,
                               &guard.nns)))
        return st;
    Mailbox* mb = ThreadMailbox();
    O3DMI_REQUIRE(mb != nullptr, "host mailbox allocation failed");
    const int seq = ++mb->seq;
    if ((st = o3dmi_icp_search_accumulate_post(
                 guard.nns, src.p, nullptr, ns, estimation, 0, 1.0, 1.0,
                 corr_dev, nullptr, mb->data, mb->flag, seq, stream)))
        return st;
    // (the search launch's tail posts a sealed block, mailbox.h)
    O3DMI_HIP_CHECK(MailboxWaitSealed(mb, seq, s, sums32));
    return O3DMI_OK;
}

}  // namespace

extern "C" int o3dmi_registration_evaluate(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, double max_dist, const double* transformation,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(result != nullptr, "result is null");
    double sums[32];
    int st = TransformSearch(source_dev, ns, target_dev, nt, dtype, max_dist,
                             transformation, O3DMI_ICP_POINT_TO_POINT,
                             correspondences_dev, sums, stream);
    if (st) return st;
    // ComputeRegistrationResult, Registration.cpp:24-62.
    const double num = sums[30];
    if (transformation)
        std::memcpy(result->transformation, transformation, sizeof(double) * 16);
    else
        Eye4(result->transformation);
    if (num != 0) {
        result->fitness = num / (double)ns;
        result->inlier_rmse = std::sqrt(sums[29] / num);
    } else {
        result->fitness = 0;
        result->inlier_rmse = 0;
        Eye4(result->transformation);
    }
    result->converged = 0;
    result->num_iterations = 0;
    result->num_correspondences = correspondences_dev ? ns : 0;
    return O3DMI_OK;
}

extern "C" int o3dmi_registration_information_matrix(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, double max_dist, const double* transformation,
        double* information36, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(information36 != nullptr, "information36 is null");
    double sums[32];
    int st = TransformSearch(source_dev, ns, target_dev, nt, dtype, max_dist,
                             transformation, 2, nullptr, sums, stream);
    if (st) return st;
    if (sums[30] == 0) {
        SetLastError(
                "0 correspondence present between the pointclouds. Try "
                "increasing the max_correspondence_distance parameter.");
        return O3DMI_ERR_NO_INLIERS;
    }
    // RegistrationCPU.cpp:727-733
    int i = 0;
    for (int j = 0; j < 6; j++)
        for (int k = 0; k <= j; k++) {
            information36[j * 6 + k] = information36[k * 6 + j] = sums[i];
            ++i;
        }
    return O3DMI_OK;
}

extern "C" int o3dmi_registration_compute_rmse(
        int estimation, const void* source_dev, int64_t ns,
        const void* target_dev, const void* target_normals_dev, int dtype,
        const o3dmi_icp_attributes_t* attrs, const int64_t* correspondences_dev,
        double* rmse_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(rmse_out != nullptr, "rmse_out is null");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && correspondences_dev,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(estimation >= O3DMI_ICP_POINT_TO_PLANE &&
                          estimation <= O3DMI_ICP_DOPPLER,
                  "unknown estimation");
    hipStream_t s = (hipStream_t)stream;
    DeviceBuffer sums;
    SyncOnExit sync_on_exit{s};
    int st = sums.Alloc(sizeof(double) * 32);
    if (st) return st;
    double h[32] = {0};
    const double zero3[3] = {0, 0, 0};
    switch (estimation) {
        case O3DMI_ICP_POINT_TO_PLANE:
        // TransformationEstimationForDopplerICP::ComputeRMSE
        // (TransformationEstimation.cpp:434-467) is the point-to-plane one
        case O3DMI_ICP_DOPPLER:
            O3DMI_REQUIRE(target_normals_dev,
                          "Target pointcloud missing normals attribute.");
            st = o3dmi_icp_residual_squares(source_dev, target_dev,
                                            target_normals_dev,
                                            correspondences_dev, ns, dtype,
                                            (double*)sums.p, stream);
            break;
        case O3DMI_ICP_POINT_TO_POINT:
            st = o3dmi_icp_residual_squares(source_dev, target_dev, nullptr,
                                            correspondences_dev, ns, dtype,
                                            (double*)sums.p, stream);
            break;
        case O3DMI_ICP_SYMMETRIC:
            O3DMI_REQUIRE(attrs && attrs->source_normals && target_normals_dev,
                          "SymmetricICP requires both source and target to "
                          "have normals.");
            // the un-centred residual does not depend on the means
            st = o3dmi_icp_symmetric_accumulate(
                    source_dev, attrs->source_normals, target_dev,
                    target_normals_dev, correspondences_dev, ns, dtype, zero3,
                    zero3, 0, 1.0, 1.0, (double*)sums.p, stream);
            break;
        default: {
            O3DMI_REQUIRE(target_normals_dev,
                          "Target pointcloud missing normals attribute.");
            O3DMI_REQUIRE(attrs && attrs->source_colors && attrs->target_colors,
                          "Source and/or Target pointcloud missing colors "
                          "attribute.");
            O3DMI_REQUIRE(attrs->target_color_gradients,
                          "Target pointcloud missing color_gradients "
                          "attribute.");
            double lambda = attrs->lambda_geometric;
            if (!(lambda >= 0 && lambda <= 1.0)) lambda = 0.968;
            st = o3dmi_icp_colored_accumulate(
                    source_dev, attrs->source_colors, target_dev,
                    target_normals_dev, attrs->target_colors,
                    attrs->target_color_gradients, correspondences_dev, ns,
                    dtype, lambda, 0, 1.0, 1.0, (double*)sums.p, stream);
        }
    }
    if (st) return st;
    const int n_read = (estimation == O3DMI_ICP_POINT_TO_PLANE ||
                        estimation == O3DMI_ICP_POINT_TO_POINT ||
                        estimation == O3DMI_ICP_DOPPLER)
                               ? 2
                               : 29;
    O3DMI_HIP_CHECK(hipMemcpyAsync(h, sums.p, sizeof(double) * n_read,
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (n_read == 2) {
        if (h[1] == 0) {
            SetLastError("No valid correspondence present.");
            return O3DMI_ERR_NO_INLIERS;
        }
        *rmse_out = std::sqrt(h[0] / h[1]);
    } else if (estimation == O3DMI_ICP_SYMMETRIC) {
        *rmse_out = h[28] == 0 ? 0.0 : std::sqrt(h[27] / h[28]);
    } else {
        *rmse_out = h[27];
    }
    return O3DMI_OK;
}

// TransformationEstimationForGeneralizedICP::ComputeRMSE (legacy
// GeneralizedICP.cpp:83-102): the accumulate kernel's rmse form -- sums[0] =
// sum d^T W d, sums[28] = the pairs.
extern "C" int o3dmi_registration_compute_rmse_generalized(
        const void* source_dev, const void* source_covariances_dev, int64_t ns,
        const void* target_dev, const void* target_covariances_dev, int64_t nt,
        int dtype, const int64_t* correspondences_dev, double* rmse_out,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(rmse_out != nullptr, "rmse_out is null");
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0 &&
                          correspondences_dev,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(source_covariances_dev && target_covariances_dev,
                  "GeneralizedICP requires both clouds to have covariances.");
    hipStream_t s = (hipStream_t)stream;
    DeviceBuffer sums;  // 32 sums and the range check's word
    SyncOnExit sync_on_exit{s};
    int st = sums.Alloc(sizeof(double) * 32 + sizeof(int));
    if (st) return st;
    int* bad = (int*)((double*)sums.p + 32);
    O3DMI_HIP_CHECK(hipMemsetAsync(sums.p, 0, sizeof(double) * 32 + sizeof(int),
                                   s));
    st = o3dmi_icp_generalized_accumulate_post(
            source_dev, source_covariances_dev, target_dev,
            target_covariances_dev, correspondences_dev, ns, nt, dtype, nullptr,
            O3DMI_L2_LOSS, 1.0, 1.0, /*rmse_form=*/1, (double*)sums.p, nullptr,
            bad, nullptr, nullptr, 0, stream);
    if (st) return st;
    struct { double v[32]; int bad; } h;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&h, sums.p, sizeof(double) * 32 + sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!h.bad, "correspondence index out of range");
    *rmse_out = h.v[28] == 0 ? 0.0 : std::sqrt(h.v[0] / h.v[28]);
    return O3DMI_OK;
}
