// Private seam between the RGB-D odometry driver (host/odometry.cpp) and
// odometry.hip.
#pragma once

#include "common.h"

// o3dmi_odometry_sums with the result also posted to a host mailbox
// (mailbox.h) when mail_data != NULL.
extern "C" int o3dmi_odometry_sums_post(
        int method, int rows, int cols, const float* const* maps11,
        const double* intrinsics, const double* init_source_to_target,
        float depth_outlier_trunc, float depth_huber_delta,
        float intensity_huber_delta, double* scratch_dev, double* sums29_dev,
        double* mail_data, int* mail_flag, int mail_seq, o3dmi_stream_t stream);
