// Private seam between the ICP driver (host/registration.cpp: the scale loop;
// host/registration_eval.cpp: EvaluateRegistration, information matrix, RMSE)
// and icp.hip: the entry points that are not in the public header.
#pragma once

#include "common.h"

namespace o3dmi {
// Rows of kNumSums partial sums in a caller's `partials_dev`: at least the
// largest grid of the gather kernels (icp.hip ReduceGrid checks it).
constexpr int kIcpPartialRows = 1024;
}  // namespace o3dmi

extern "C" {

// o3dmi_icp_search_accumulate[_p2point] (`estimation` 0 / 1) that also posts
// the 32 sums to a host mailbox (mailbox.h) when mail_data != NULL;
// sums32_dev may then be NULL.
int o3dmi_icp_search_accumulate_post(
        const o3dmi_nns_t* nns, const void* src_dev,
        const void* tgt_normals_dev, int64_t n, int estimation,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        int64_t* corr_out_dev, double* sums32_dev, double* mail_data,
        int* mail_flag, int mail_seq, o3dmi_stream_t stream);

// The same with the source moved by `transformation` (4x4, NULL: as it is) in
// place before it is searched.
int o3dmi_internal_icp_transform_search_accumulate(
        const o3dmi_nns_t* nns, void* src_dev, const double* transformation,
        const void* tgt_normals_dev, int64_t n, int estimation,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        int64_t* corr_out_dev, double* sums32_dev, double* mail_data,
        int* mail_flag, int mail_seq, o3dmi_stream_t stream);

// o3dmi_icp_colored_accumulate / o3dmi_icp_symmetric_accumulate that also post
// the 29 sums to a host mailbox when mail_data != NULL.
int o3dmi_icp_colored_accumulate_post(
        const void* src_dev, const void* src_colors_dev, const void* tgt_dev,
        const void* tgt_normals_dev, const void* tgt_colors_dev,
        const void* tgt_color_gradients_dev, const int64_t* corr_dev, int64_t n,
        int dtype, double lambda_geometric, int robust_kernel,
        double scaling_parameter, double shape_parameter, double* sums29_dev,
        double* partials_dev, double* mail_data, int* mail_flag, int mail_seq,
        o3dmi_stream_t stream);

int o3dmi_icp_symmetric_accumulate_post(
        const void* src_dev, const void* src_normals_dev, const void* tgt_dev,
        const void* tgt_normals_dev, const int64_t* corr_dev, int64_t n,
        int dtype, const double* source_mean3, const double* target_mean3,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        double* sums29_dev, double* partials_dev, double* mail_data,
        int* mail_flag, int mail_seq, o3dmi_stream_t stream);

// o3dmi_icp_doppler_accumulate without its wait: bad_dev is the caller's
// zeroed device word, raised by a correspondence index outside [0, nt); the
// sums are then not written (sums29_dev) or posted as NaN (mailbox).
int o3dmi_icp_doppler_accumulate_post(
        const void* src_dev, const void* src_dopplers_dev,
        const void* src_directions_dev, const void* tgt_dev,
        const void* tgt_normals_dev, const int64_t* corr_dev, int64_t n,
        int64_t nt, int dtype, const double* R_S_to_V9,
        const double* r_v_to_s_in_V3, const double* w_v_in_V3,
        const double* v_v_in_V3, double period, int reject_dynamic_outliers,
        double doppler_outlier_threshold, int geometric_kernel,
        double geometric_scaling, double geometric_shape, int doppler_kernel,
        double doppler_scaling, double doppler_shape, double lambda_doppler,
        double* sums29_dev, double* partials_dev, int* bad_dev,
        double* mail_data, int* mail_flag, int mail_seq, o3dmi_stream_t stream);

// o3dmi_icp_generalized_accumulate without its wait (bad_dev as above); the
// 32 sums, [29] = the pairs that could not be whitened. rmse_form: sums[0] =
// sum d^T W d and [28] = the pair count only (ComputeRMSE, GeneralizedICP.cpp:
// 83-102; R_source9 and the robust kernel are then not read).
int o3dmi_icp_generalized_accumulate_post(
        const void* src_dev, const void* src_covariances_dev,
        const void* tgt_dev, const void* tgt_covariances_dev,
        const int64_t* corr_dev, int64_t n, int64_t nt, int dtype,
        const double* R_source9, int robust_kernel, double scaling_parameter,
        double shape_parameter, int rmse_form, double* sums32_dev,
        double* partials_dev, int* bad_dev, double* mail_data, int* mail_flag,
        int mail_seq, o3dmi_stream_t stream);

// {n,3,3} -> its three {n,3} row tables and back: a covariance attribute
// through the {n,3} VoxelDownSample levels of the pyramid.
int o3dmi_internal_split_rows3(const void* in9_dev, int64_t n, int dtype,
                               void* row0_dev, void* row1_dev, void* row2_dev,
                               o3dmi_stream_t stream);
int o3dmi_internal_join_rows3(const void* row0_dev, const void* row1_dev,
                              const void* row2_dev, int64_t n, int dtype,
                              void* out9_dev, o3dmi_stream_t stream);

// {n,1} -> column 0 of {n,3} (columns 1, 2 zero), and column 0 back: a
// 1-column attribute through the {n,3} VoxelDownSample levels of the pyramid.
int o3dmi_internal_pad_column(const void* in_dev, int64_t n, int dtype,
                              void* out3_dev, o3dmi_stream_t stream);
int o3dmi_internal_take_column(const void* in3_dev, int64_t n, int dtype,
                               void* out_dev, o3dmi_stream_t stream);

// sums32_dev[29..31] = {t29, t30, t31}; the 32 sums to a host mailbox.
int o3dmi_internal_sums_tail(double* sums32_dev, double t29, double t30,
                             double t31, o3dmi_stream_t stream);
int o3dmi_internal_sums_post(const double* sums32_dev, double* mail_data,
                             int* mail_flag, int seq, o3dmi_stream_t stream);

// o3dmi_registration_compute_rmse: sums2_dev[0] = sum of squared residual
// components, [1] = number of correspondences.
int o3dmi_icp_residual_squares(const void* src_dev, const void* tgt_dev,
                               const void* tgt_normals_dev,
                               const int64_t* corr_dev, int64_t n, int dtype,
                               double* sums2_dev, o3dmi_stream_t stream);

}  // extern "C"
