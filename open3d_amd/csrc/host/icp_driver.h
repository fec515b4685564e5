// Private seam between the pieces of the MultiScaleICP host driver:
// registration.cpp (entry point, index scheduler, sums fetcher, scale loop)
// and icp_pyramid.cpp (the two clouds' VoxelDownSample pyramids and the first
// scale's index).
#pragma once

#include <vector>

#include "../collectives.h"
#include "../common.h"
#include "host_util.h"
#include "o3d_mi355x_host.h"

namespace o3dmi {

// Everything one driver call was asked to do, resolved once by the entry point
// (o3dmi_registration_multiscale_icp_ex) and const below it: nothing there
// reads the thread's communicator or an argument of the C ABI again.
struct IcpCall {
    int dtype = O3DMI_F32;
    size_t esz = 4;
    // the caller's stream, and the side stream + event of the overlapped
    // pyramid build (`side` == `s`: no overlap)
    hipStream_t s = nullptr, side = nullptr;
    o3dmi_stream_t stream() const { return (o3dmi_stream_t)s; }
    hipEvent_t ev = nullptr;

    int estimation = O3DMI_ICP_POINT_TO_POINT;  // O3DMI_ICP_*
    bool Is(int e) const { return estimation == e; }
    // the fused search launch accumulates the point-to-plane terms itself (its
    // index carries the target's normals); the others take its moments
    bool SearchesPointToPlane() const { return Is(O3DMI_ICP_POINT_TO_PLANE); }
    // a second launch per iteration gathers by correspondence
    bool GathersByCorrespondence() const {
        return !Is(O3DMI_ICP_POINT_TO_PLANE) && !Is(O3DMI_ICP_POINT_TO_POINT);
    }
    bool NeedsTargetNormals() const {
        return !Is(O3DMI_ICP_POINT_TO_POINT) && !Is(O3DMI_ICP_GENERALIZED);
    }

    // clouds and attributes (NULL: the estimator does not read it)
    const void *source = nullptr, *source_normals = nullptr,
               *source_colors = nullptr;
    const void *target = nullptr, *target_normals = nullptr,
               *target_colors = nullptr, *target_gradients = nullptr;
    // Doppler ICP: directions {n,3}; dopplers as column 0 of an {n,3} buffer
    // of the driver (the pyramid's levels take {n,3} attributes)
    const void *source_directions = nullptr, *source_dopplers3 = nullptr;
    // Generalized ICP: each cloud's covariances {n,3,3} as the three {n,3} row
    // tables of the driver
    const void *source_cov_rows[3] = {}, *target_cov_rows[3] = {};
    int64_t ns = 0, nt = 0;
    // sizes that live on the device (o3dmi_icp_options_t)
    const int32_t *ns_dev = nullptr, *nt_dev = nullptr;

    int num_scales = 0;
    const double *voxel_sizes = nullptr, *max_dists = nullptr;
    const o3dmi_icp_criteria_t* criterias = nullptr;
    bool finest_is_input = false;  // voxel_sizes[last] <= 0

    double lambda_geometric = 0.968;  // (clamped)
    // TransformationEstimationForDopplerICP's parameters (lambda_doppler
    // clamped), and from its transform_vehicle_to_sensor, in float64: the
    // inverse of the rotation and the translation
    o3dmi_icp_doppler_t dop = {};
    double R_S_to_V[9] = {}, r_v_to_s_in_V[3] = {};
    // TransformationEstimationForGeneralizedICP's parameters
    o3dmi_icp_generalized_t gen = {};
    int robust_kernel = 0;
    double scaling_parameter = 1.0, shape_parameter = 1.0;

    o3dmi_icp_callback_t callback = nullptr;
    o3dmi_allreduce_sum_t allreduce = nullptr;  // host all-reduce hook
    void *callback_user = nullptr, *allreduce_user = nullptr;
    // the thread's communicator, read once at entry; NULL also for a world of
    // one rank
    o3dmi_comm* comm = nullptr;
    // o3dmi_icp_options_t: device hook; level sharding (false without `comm`)
    o3dmi_allreduce_device_t dev_allreduce = nullptr;
    void* dev_allreduce_user = nullptr;
    bool level_sharding = false;
};

// One cloud at one pyramid level: positions and its {n,3} attributes.
// Source: normals (symmetric), colours (coloured), directions and dopplers
// (Doppler; the dopplers in column 0); target: normals, colours, colour
// gradients; both: the three rows of the covariances (generalized).
enum {
    kNormals = 0, kColors = 1, kGradients = 2, kDirections = 3, kDopplers = 4,
    kCovRow0 = 5, kCovRow1 = 6, kCovRow2 = 7, kCloudAttrs = 8
};
struct CloudLevel {
    DeviceBuffer pos_buf, attr_buf[kCloudAttrs];
    const void* pos = nullptr;  // may alias the caller's buffers (target)
    const void* attr[kCloudAttrs] = {};
    int64_t n = 0;
};
struct Level { CloudLevel source, target; };

// InitializePointCloudPyramidForMultiScaleICP, Registration.cpp:221-273, for
// both clouds, with every level's size on the host when it returns, and the
// coarsest scale's index (`first_index`) issued on the caller's stream.
int BuildPyramids(const IcpCall& call, std::vector<Level>& pyr,
                  NnsGuard& first_index);

// One side stream and event per host thread AND device for the overlapped
// pyramid build (a thread may switch devices between calls: per-device pool,
// VoxelBlockGrid::To(device)).
hipStream_t SideStream();
hipEvent_t SideEvent();

}  // namespace o3dmi
