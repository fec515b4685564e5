/* o3d_mi355x_host.h -- host-side mirror (C++ implementation, C linkage) of the
 * Open3D classes that drive the hot path, built on top of the kernel C ABI in
 * o3d_mi355x.h. These are what a language binding (pybind / ctypes / cgo)
 * calls when it wants the whole operator rather than one kernel:
 *
 *   o3dmi_registration_multiscale_icp  <- t::pipelines::registration::MultiScaleICP / ICP
 *   (_ex: estimator choice)               (t/pipelines/registration/Registration.cpp:93-106,362-444)
 *   o3dmi_registration_evaluate,       <- EvaluateRegistration, GetInformationMatrix
 *   o3dmi_registration_information_matrix (Registration.cpp:64-91,446-486)
 *   o3dmi_registration_compute_fpfh_feature, <- ComputeFPFHFeature, CorrespondencesFromFeatures
 *   o3dmi_registration_correspondences_from_features (Feature.cpp:23-333)
 *   o3dmi_registration_ransac_correspondence, <- legacy RegistrationRANSACBasedOnCorrespondence /
 *   o3dmi_registration_ransac_feature_matching   ...FeatureMatching (pipelines/registration/Registration.cpp:212-406)
 *   o3dmi_registration_fgr_correspondence, <- legacy FastGlobalRegistrationBasedOnCorrespondence /
 *   o3dmi_registration_fgr_feature_matching   ...FeatureMatching (pipelines/registration/FastGlobalRegistration.cpp)
 *   o3dmi_slac_correspondence_set,     <- t::pipelines::slac::RunRigidOptimizerForFragments
 *   o3dmi_slac_rigid_optimize             (t/pipelines/slac/SLACOptimizer.cpp:85-204,265-286,369-414)
 *   o3dmi_slac_optimize,               <- t::pipelines::slac::RunSLACOptimizerForFragments, kernel::FillInSLAC*Term
 *   o3dmi_fill_in_slac_*_term,            (t/pipelines/slac/SLACOptimizer.cpp:253-367, kernel/FillInLinearSystemImpl.h:156-524)
 *   o3dmi_slac_solve_spd
 *   o3dmi_control_grid_*,              <- t::pipelines::slac::ControlGrid (t/pipelines/slac/ControlGrid.cpp:24-322),
 *   o3dmi_project_to_{depth,rgbd}_image   PointCloud::ProjectTo{Depth,RGBD}Image (t/geometry/PointCloud.cpp:1471-1530)
 *   o3dmi_voxel_down_sample,           <- t::geometry::PointCloud::{VoxelDownSample, EstimateNormals,
 *   o3dmi_pointcloud_estimate_*           EstimateColorGradients} (t/geometry/PointCloud.cpp:496-567,856-1060)
 *   o3dmi_vbg_*                        <- t::geometry::VoxelBlockGrid (+ Save / Load)
 *                                         (t/geometry/VoxelBlockGrid.cpp:65-117,212-602)
 *   o3dmi_rgbd_odometry_multiscale     <- t::pipelines::odometry::RGBDOdometryMultiScale
 *                                         (t/pipelines/odometry/RGBDOdometry.cpp:56-513)
 *   o3dmi_slam_model_*                 <- t::pipelines::slam::Model (t/pipelines/slam/Model.cpp:23-118)
 *   o3dmi_npz_*                        <- t::io::WriteNpz / ReadNpz (t/io/NumpyIO.cpp:157-789)
 *
 * Same argument meaning, defaults and error behaviour as the reference
 * (errors are status codes + o3dmi_last_error() instead of exceptions).
 */
#ifndef O3D_MI355X_HOST_H_
#define O3D_MI355X_HOST_H_

#include "o3d_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ICPConvergenceCriteria (t/pipelines/registration/Registration.h:31-58):
 * defaults relative_fitness 1e-6, relative_rmse 1e-6, max_iteration 30. */
typedef struct {
    double relative_fitness;
    double relative_rmse;
    int max_iteration;
} o3dmi_icp_criteria_t;

/* RegistrationResult (Registration.h:61-98). */
typedef struct {
    double transformation[16]; /* 4x4 float64, row-major, host            */
    double inlier_rmse;
    double fitness;
    int converged;
    int num_iterations;
    int64_t num_correspondences; /* rows written to correspondences_dev   */
} o3dmi_registration_result_t;

/* callback_after_iteration (Registration.cpp:330-345): iteration_index,
 * scale_index, scale_iteration_index, inlier_rmse, fitness, transformation. */
typedef void (*o3dmi_icp_callback_t)(int64_t iteration_index,
                                     int64_t scale_index,
                                     int64_t scale_iteration_index,
                                     double inlier_rmse, double fitness,
                                     const double* transformation, void* user);

/* Cross-GPU hook: in-place SUM over all ranks of `n` host doubles (the 29
 * Gauss-Newton sums, sum d2, match count and the local source-point count).
 * NULL = single GPU. Each rank holds a shard of the source cloud and the whole
 * target; every rank then solves the same 6x6 system. */
typedef int (*o3dmi_allreduce_sum_t)(double* host_buf, int n, void* user);

/* The same exchange on the DEVICE: the hook enqueues an in-place sum
 * all-reduce of dev_buf[0..n) (float64) over all ranks on `stream`
 * (asynchronously -- e.g. RCCL's ncclAllReduce, or torch.distributed's
 * all_reduce under that stream) and returns 0. Passed to a driver call in
 * o3dmi_icp_options_t. */
typedef int (*o3dmi_allreduce_device_t)(double* dev_buf, int n,
                                        o3dmi_stream_t stream, void* user);

/* ---- Collectives owned by the library (multi-GPU) -------
 * One process (or host thread) per GPU. An o3dmi_comm_t carries the three
 * exchanges the sharded hot path needs -- sum all-reduce of float64 (the ICP
 * sums), all-gather of fixed-size records and all-to-all of byte ranges (block
 * IDs and voxel rows to their owners) -- all enqueued on the caller's stream.
 * Transports:
 *   RCCL    librccl.so resolved with dlopen at first use (the instance the
 *           process already holds, e.g. PyTorch's, else the system one;
 *           O3DMI_RCCL_LIB overrides): ncclAllReduce / ncclAllGather / grouped
 *           ncclSend + ncclRecv over xGMI. o3dmi_rccl_unique_id +
 *           o3dmi_comm_create_rccl wrap ncclGetUniqueId / ncclCommInitRank on
 *           the current device (the 128-byte id travels by the caller's own
 *           means: MPI, a file, torch.distributed); o3dmi_comm_adopt_rccl
 *           wraps an existing ncclComm_t (not destroyed with the wrapper).
 *   custom  a table of functions (tests over gloo; other runtimes). Each
 *           entry enqueues (or completes) the exchange for the given stream
 *           and returns 0.
 * o3dmi_set_comm(c) makes c the communicator of the calling host thread: the
 * registration drivers (every estimator) then sum their per-iteration values
 * through it ON THE DEVICE, between the final reduction kernel and the kernel that
 * posts them to the host mailbox (takes precedence over both hooks of the
 * call; NULL restores them). o3dmi_set_rccl_comm(ncclComm) = adopt + set in one
 * call (NULL clears). The reference has no counterpart. */
typedef struct o3dmi_comm o3dmi_comm_t;
typedef struct {
    int (*allreduce_sum_f64)(void* user, double* dev_buf, int64_t n,
                             o3dmi_stream_t stream);
    int (*allgather)(void* user, const void* send_dev, void* recv_dev,
                     int64_t bytes_per_rank, o3dmi_stream_t stream);
    int (*alltoallv)(void* user, const void* send_dev,
                     const int64_t* send_bytes, const int64_t* send_offsets,
                     void* recv_dev, const int64_t* recv_bytes,
                     const int64_t* recv_offsets, o3dmi_stream_t stream);
} o3dmi_transport_t;
int o3dmi_rccl_available(void);
int o3dmi_rccl_unique_id(void* id128 /* 128 bytes */);
int o3dmi_comm_create_rccl(const void* id128, int rank, int world,
                           o3dmi_comm_t** out);
int o3dmi_comm_adopt_rccl(void* nccl_comm, o3dmi_comm_t** out);
int o3dmi_comm_create_custom(const o3dmi_transport_t* table, void* user,
                             int rank, int world, o3dmi_comm_t** out);
int o3dmi_comm_destroy(o3dmi_comm_t* c);
int o3dmi_comm_rank(const o3dmi_comm_t* c);
int o3dmi_comm_world(const o3dmi_comm_t* c);
/* ncclCommCount of the RCCL communicator behind `c`, asked of RCCL at the
 * time of the call; 0 for a custom transport (or a NULL handle): lets a
 * caller record which transport carried its collectives and over how many
 * ranks (bench.py config.transport / config.rccl_ranks). */
int o3dmi_comm_rccl_ranks(const o3dmi_comm_t* c);
int o3dmi_set_comm(o3dmi_comm_t* c);
int o3dmi_set_rccl_comm(void* nccl_comm);
/* The exchanges themselves (what the drivers call). Counts / offsets of the
 * all-to-all are host arrays of `world` entries, in bytes. */
int o3dmi_comm_allreduce_sum_f64(o3dmi_comm_t* c, double* dev_buf, int64_t n,
                                 o3dmi_stream_t stream);
int o3dmi_comm_allgather(o3dmi_comm_t* c, const void* send_dev, void* recv_dev,
                         int64_t bytes_per_rank, o3dmi_stream_t stream);
int o3dmi_comm_alltoallv(o3dmi_comm_t* c, const void* send_dev,
                         const int64_t* send_bytes,
                         const int64_t* send_offsets, void* recv_dev,
                         const int64_t* recv_bytes,
                         const int64_t* recv_offsets, o3dmi_stream_t stream);

/* MultiScaleICP with TransformationEstimationPointToPlane(kernel).
 * source/target/normals: device, {N,3}, dtype O3DMI_F32 or O3DMI_F64.
 * voxel_sizes[i] <= 0 means "no down-sampling" for the finest level, as in
 * the reference (Registration.cpp:233-236).
 * correspondences_dev: optional device int64 buffer of ns entries receiving
 * the final correspondence set of the finest scale (-1 = none).
 * Status O3DMI_ERR_SINGULAR mirrors the reference's "Singular 6x6 linear
 * system detected, tracking failed." exception. */
int o3dmi_registration_multiscale_icp(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_correspondence_distances,
        const double* init_source_to_target /* 4x4, may be NULL = identity */,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream);

/* TransformationEstimation choice for o3dmi_registration_multiscale_icp_ex
 * (t/pipelines/registration/TransformationEstimation.h:28-34). */
typedef enum {
    O3DMI_ICP_POINT_TO_PLANE = 0,
    O3DMI_ICP_POINT_TO_POINT = 1,
    O3DMI_ICP_SYMMETRIC = 2,
    O3DMI_ICP_COLORED = 3,
    O3DMI_ICP_DOPPLER = 4, /* o3dmi_registration_multiscale_icp_doppler only */
    O3DMI_ICP_GENERALIZED = 5 /* o3dmi_registration_multiscale_icp_generalized
                                 only */
} o3dmi_icp_estimation_t;

/* Point attributes beyond positions / target normals that some estimators
 * read (device, {N,3}, point dtype). Unused members may be NULL. */
typedef struct {
    const void* source_normals;         /* SYMMETRIC                          */
    const void* source_colors;          /* COLORED                            */
    const void* target_colors;          /* COLORED                            */
    const void* target_color_gradients; /* COLORED, optional: estimated on the
                                           finest level when NULL, as
                                           Registration.cpp:243-262 does     */
    double lambda_geometric;            /* COLORED; outside [0,1] -> 0.968    */
} o3dmi_icp_attributes_t;

/* What one o3dmi_registration_multiscale_icp_ex call is given beyond the
 * reference's arguments; zeroed (or a NULL pointer) = none of it. The
 * communicator is not here: o3dmi_set_comm is ambient per-thread state that
 * integrate, ray cast and ICP all read, not an argument of one call. */
typedef struct {
    /* Sizes that are still on the device. A tracking loop produces its clouds
     * with o3dmi_unproject, which leaves the point counts in device words;
     * reading them back costs the loop a stream drain per frame. With a
     * pointer given, the call takes the live source / target size from it
     * (int32, written by work queued earlier on the call's stream; NULL = the
     * host argument as usual) and reads its ns / nt argument as the capacity
     * of the buffer. With a down-sampled finest level (voxel_sizes[last] > 0,
     * the tracking configuration) nothing waits for them: the pyramid launches
     * bound themselves by the device words. Without one the driver fetches
     * them first. A live size of zero is then reported through the usual "0
     * correspondence" result. The reference has no counterpart (its Tensor
     * shapes live on the host). */
    const int32_t* ns_dev;
    const int32_t* nt_dev;
    /* Device-side all-reduce hook (NULL = the host hook, or none). It takes
     * precedence over the host hook `allreduce` and yields to a communicator
     * installed with o3dmi_set_comm: the per-iteration sums then stay on the
     * device from the final reduction kernel through the collective to the
     * kernel that posts them to the host mailbox (one host wait per
     * iteration, no staging copies). */
    o3dmi_allreduce_device_t device_allreduce;
    void* device_allreduce_user;
    /* Who shards the source cloud when the calling thread has a communicator
     * of more than one rank installed (ignored without one):
     *   0  the caller: each rank passes ITS shard of the source (the semantics
     *      of the two hooks). A voxel pyramid is then built per shard, i.e.
     *      the coarse levels differ from the unsharded run's.
     *   1  the driver: every rank passes the WHOLE source; the pyramid is
     *      built from it on every rank (it IS the unsharded pyramid), and each
     *      rank searches and accumulates a contiguous slice of every level.
     *      The poses equal the unsharded run's to the rounding of the float64
     *      sums for any number of scales. correspondences_dev: a rank fills
     *      its slice of the finest level's rows, the other rows read -1. */
    int level_sharding;
} o3dmi_icp_options_t;

/* MultiScaleICP with a selectable estimator. POINT_TO_PLANE is exactly
 * o3dmi_registration_multiscale_icp; POINT_TO_POINT
 * (TransformationEstimationPointToPoint, TransformationEstimation.cpp:101-160)
 * ignores the normals (may be NULL) and the robust kernel; SYMMETRIC
 * (TransformationEstimationSymmetric, :229-292) needs attrs->source_normals
 * and target_normals_dev -- the source normals are carried through the pyramid
 * and rotated with the source, as PointCloud::Transform does; COLORED
 * (TransformationEstimationForColoredICP, :296-440) needs target normals and
 * both colour sets, every attribute is averaged through the VoxelDownSample
 * pyramid, and missing colour gradients are estimated on the finest level
 * with EstimateColorGradients(30, 4 voxel_size or 2 max_distance).
 * attrs may be NULL for the first two estimators, options always. */
int o3dmi_registration_multiscale_icp_ex(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_correspondence_distances,
        const double* init_source_to_target, int estimation,
        const o3dmi_icp_attributes_t* attrs, const o3dmi_icp_options_t* options,
        int robust_kernel, double scaling_parameter, double shape_parameter,
        o3dmi_icp_callback_t callback, void* callback_user,
        o3dmi_allreduce_sum_t allreduce, void* allreduce_user,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_stream_t stream);

/* TransformationEstimationForDopplerICP (TransformationEstimation.h:356-500;
 * Hexsel et al., "DICP: Doppler Iterative Closest Point Algorithm", RSS 2022):
 * the estimator's parameters and the two source attributes it reads. */
typedef struct {
    const void* source_dopplers;   /* device {N,1}, point dtype               */
    const void* source_directions; /* device {N,3}, point dtype, unit vectors
                                      of the vehicle frame; carried through
                                      the pyramid, never rotated             */
    double transform_vehicle_to_sensor[16]; /* row-major 4x4; all zero =
                                               identity                      */
    double period;                 /* default 0.1; <= 0: INVALID_ARG          */
    double lambda_doppler;         /* default 0.01; outside [0,1] -> 0.01     */
    int reject_dynamic_outliers;   /* default 0                               */
    double doppler_outlier_threshold;        /* default 2.0                   */
    int outlier_rejection_min_iteration;     /* default 2                     */
    int geometric_robust_loss_min_iteration; /* default 0                     */
    int doppler_robust_loss_min_iteration;   /* default 2                     */
    int geometric_kernel;          /* o3dmi robust kernel method, default L2  */
    double geometric_scaling_parameter, geometric_shape_parameter;
    int doppler_kernel;
    double doppler_scaling_parameter, doppler_shape_parameter;
} o3dmi_icp_doppler_t;

/* MultiScaleICP with TransformationEstimationForDopplerICP: the argument list
 * of o3dmi_registration_multiscale_icp_ex with `estimation`, `attrs` and the
 * single robust kernel replaced by `doppler` (o3dmi_registration_multiscale_
 * icp_ex itself answers O3DMI_ICP_DOPPLER with O3DMI_ERR_INVALID_ARG: it has
 * nowhere to take these from). Per iteration: search, then one launch that
 * gathers by correspondence and accumulates the 29 sums
 * (o3dmi_icp_doppler_accumulate); the host prepares what ComputePoseDopplerICP
 * (kernel/Registration.cpp:222-265) prepares -- the kernels and the rejection
 * in force at the iteration index, which restarts at 0 at every scale, and the
 * vehicle's velocities from TransformationToPose(current transformation) / period
 * -- in float64, narrowed to the point dtype where the reference narrows.
 * dopplers and directions are averaged through the VoxelDownSample pyramid like
 * any attribute (directions are not re-normalised). O3DMI_ERR_INVALID_ARG:
 * missing target normals, dopplers or directions, period <= 0, a non-finite
 * transform_vehicle_to_sensor. O3DMI_ERR_UNSUPPORTED: reject_dynamic_outliers
 * with L1Loss on either term (the reference sums NaN there). Sharding: the two
 * all-reduce hooks with a caller-sharded source see the 29 sums as for the other
 * estimators; with level_sharding the driver slices dopplers and directions
 * with the positions. */
int o3dmi_registration_multiscale_icp_doppler(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_correspondence_distances,
        const double* init_source_to_target, const o3dmi_icp_doppler_t* doppler,
        const o3dmi_icp_options_t* options, o3dmi_icp_callback_t callback,
        void* callback_user, o3dmi_allreduce_sum_t allreduce,
        void* allreduce_user, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_stream_t stream);

/* TransformationEstimationForGeneralizedICP (legacy pipelines/registration/
 * GeneralizedICP.{h,cpp}; Segal et al., "Generalized-ICP", RSS 2009): the
 * estimator's parameters and the per-point covariances it reads. The reference
 * has it in the legacy API only (CPU, float64, single scale). */
typedef struct {
    const void* source_covariances; /* device {N,3,3}, point dtype, or NULL   */
    const void* target_covariances; /* device {N,3,3}, point dtype, or NULL   */
    const void* source_normals;     /* device {N,3}; read when
                                       source_covariances is NULL (the target's
                                       normals are the call's
                                       target_normals_dev)                    */
    double epsilon;                 /* default 1e-3; <= 0 or non-finite:
                                       INVALID_ARG                            */
    int robust_kernel;              /* o3dmi robust kernel method, default L2 */
    double scaling_parameter, shape_parameter;
    int64_t* singular_pairs_out;    /* optional, host: sums[29] of the call's
                                       last accumulate (pairs that could not
                                       be whitened)                           */
} o3dmi_icp_generalized_t;

/* MultiScaleICP with TransformationEstimationForGeneralizedICP: the argument
 * list of o3dmi_registration_multiscale_icp_doppler with `doppler` replaced by
 * `generalized` (o3dmi_registration_multiscale_icp_ex answers
 * O3DMI_ICP_GENERALIZED with O3DMI_ERR_INVALID_ARG). Covariances per cloud, as
 * InitializePointCloudForGeneralizedICP (GeneralizedICP.cpp:52-80): given ->
 * used as they are; else normals given ->
 * o3dmi_pointcloud_covariances_from_normals; else EstimateNormals with KNN 20
 * on the input cloud, then the same (a cloud of fewer than 3 points: that
 * call's error, unchanged). The nine columns ride through the VoxelDownSample
 * pyramid as three {n,3} row tables per cloud, averaged like any attribute (as
 * the legacy VoxelDownSample does). Per iteration: search, then one launch
 * that gathers by correspondence (o3dmi_icp_generalized_accumulate) with
 * R_source9 = the rotation of the cumulative transformation: the level's
 * source covariance tables are never rewritten (the reference rotates them
 * incrementally with every Transform; equal to rounding). Sharding as for the
 * other estimators; level_sharding slices the covariance tables with the
 * positions. Sizes on the device (options->ns_dev / nt_dev) are
 * O3DMI_ERR_UNSUPPORTED for a cloud whose normals would have to be
 * estimated. */
int o3dmi_registration_multiscale_icp_generalized(
        const void* source_dev, int64_t ns, const void* target_dev,
        const void* target_normals_dev, int64_t nt, int dtype, int num_scales,
        const double* voxel_sizes, const o3dmi_icp_criteria_t* criterias,
        const double* max_correspondence_distances,
        const double* init_source_to_target,
        const o3dmi_icp_generalized_t* generalized,
        const o3dmi_icp_options_t* options, o3dmi_icp_callback_t callback,
        void* callback_user, o3dmi_allreduce_sum_t allreduce,
        void* allreduce_user, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_stream_t stream);

/* TransformationEstimationForGeneralizedICP::ComputeRMSE (GeneralizedICP.cpp:
 * 83-102), the reference's definition kept as it is: sqrt(sum d^T W d / count)
 * with W = (Ct + Cs)^-1/2 -- not W^2 -- over the rows with a correspondence
 * (int64[ns], -1 = none). Covariances {N,3,3} in the point dtype, used as
 * given (the source's are not rotated). No correspondence: 0.0, as the
 * reference. A pair that cannot be whitened adds 0 and stays in the count. An
 * index outside [0, nt) other than -1: O3DMI_ERR_INVALID_ARG. *rmse_out is a
 * host double; the call synchronises. */
int o3dmi_registration_compute_rmse_generalized(
        const void* source_dev, const void* source_covariances_dev, int64_t ns,
        const void* target_dev, const void* target_covariances_dev, int64_t nt,
        int dtype, const int64_t* correspondences_dev, double* rmse_out,
        o3dmi_stream_t stream);

/* TransformationEstimation*::ComputeRMSE (TransformationEstimation.cpp:
 * 101-130 point-to-point, 160-193 point-to-plane, 229-274 symmetric, 296-378
 * coloured) on given correspondences (int64, -1 = none). The reference's
 * definitions are kept as they are: point-to-plane squares every component
 * of (s - t) * n; the coloured estimator returns the SUM of squared geometric
 * and photometric residuals, not a root mean; O3DMI_ICP_DOPPLER (:434-467) has
 * the point-to-plane definition. *rmse_out is a host double; the
 * call synchronises. No correspondence: 0 for the symmetric estimator (as the
 * reference), O3DMI_ERR_NO_INLIERS otherwise (the reference divides by 0). */
int o3dmi_registration_compute_rmse(
        int estimation, const void* source_dev, int64_t ns,
        const void* target_dev, const void* target_normals_dev, int dtype,
        const o3dmi_icp_attributes_t* attrs, const int64_t* correspondences_dev,
        double* rmse_out, o3dmi_stream_t stream);

/* registration::EvaluateRegistration (Registration.cpp:64-91): fitness,
 * inlier_rmse and the correspondence set of `source` moved by `transformation`
 * (host 4x4 float64, NULL = identity) against `target`. result->transformation
 * is `transformation` (identity when nothing matches, Registration.cpp:56-58),
 * converged = 0, num_iterations = 0. correspondences_dev: optional int64[ns]. */
int o3dmi_registration_evaluate(const void* source_dev, int64_t ns,
                                const void* target_dev, int64_t nt, int dtype,
                                double max_correspondence_distance,
                                const double* transformation,
                                int64_t* correspondences_dev,
                                o3dmi_registration_result_t* result,
                                o3dmi_stream_t stream);

/* registration::GetInformationMatrix (Registration.cpp:446-486): 6x6 float64
 * (host, row-major). O3DMI_ERR_NO_INLIERS mirrors "0 correspondence present
 * between the pointclouds. Try increasing the max_correspondence_distance
 * parameter.". */
int o3dmi_registration_information_matrix(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, double max_correspondence_distance,
        const double* transformation, double* information36,
        o3dmi_stream_t stream);

/* ComputeFPFHFeature (t/pipelines/registration/Feature.cpp:23-277): FPFH
 * {rows, 33} of a cloud with normals. Hybrid search when both max_nn and
 * radius are given, KNN search (k = min(max_nn, n)) for max_nn alone, radius
 * search for radius alone. max_nn <= 3, radius <= 0, no normals or neither
 * parameter: O3DMI_ERR_INVALID_ARG; max_nn > 128: O3DMI_ERR_UNSUPPORTED.
 * indices_dev (int64, n_indices >= 0; NULL with n_indices < 0 = all points):
 * one row per DISTINCT index in ascending order, as the reference's mask +
 * NonZero; an index outside [0, n) is O3DMI_ERR_INVALID_ARG; none gives 0
 * rows. fpfhs_dev must hold min(n_indices, n) rows (n without indices);
 * *n_rows_out receives the row count. n must be below 2^27 (the grid index
 * addresses its records by 32-bit byte offsets); larger clouds are
 * O3DMI_ERR_INVALID_ARG. Synchronises. */
int o3dmi_registration_compute_fpfh_feature(
        const void* points_dev, const void* normals_dev, int64_t n, int dtype,
        int has_max_nn, int max_nn, int has_radius, double radius,
        const int64_t* indices_dev, int64_t n_indices, void* fpfhs_dev,
        int64_t* n_rows_out, o3dmi_stream_t stream);

/* CorrespondencesFromFeatures (Feature.cpp:279-333): for every source row i
 * the target row j nearest in feature space, as int64 pairs (i, j) in
 * ascending i. Distance: sum_k (a_k - b_k)^2 in float64 over k = 0..dim-1 in
 * order (exact for Float32 and Float64 features); ties go to the lowest index
 * (stricter than the reference's GEMM-based search). A NaN distance (NaN or
 * inf in a feature) counts as +inf, so every row gets an index in range. With mutual_filter, only
 * pairs whose target row has i as its own nearest source row are kept, unless
 * they number <= mutual_consistency_ratio * n_source (float): then all
 * n_source pairs are returned and *fell_back (optional) is set to 1 (the
 * reference logs a warning). correspondences_dev holds {n_source, 2};
 * *n_correspondences receives the rows written. Synchronises. */
int o3dmi_registration_correspondences_from_features(
        const void* source_dev, int64_t n_source, const void* target_dev,
        int64_t n_target, int dim, int dtype, int mutual_filter,
        float mutual_consistency_ratio, int64_t* correspondences_dev,
        int64_t* n_correspondences, int* fell_back, o3dmi_stream_t stream);

/* RegistrationRANSACBasedOnCorrespondence / ...BasedOnFeatureMatching
 * (legacy pipelines/registration/Registration.cpp:212-406; the one place where
 * this library mirrors a legacy operator: there is no tensor version). The
 * semantics are rules 1-6 of "RANSAC on correspondences" in o3d_mi355x.h: the
 * reference loop run by ONE thread over a stateless sample stream, reproduced
 * exactly whatever batch_size is. RANSACConvergenceCriteria defaults:
 * max_iteration 100000, confidence 0.999. */
typedef struct {
    int num_checkers;            /* <= 3, each kind at most once, in order  */
    int checker_types[3];        /* O3DMI_RANSAC_CHECK_*                     */
    double checker_thresholds[3];/* similarity / distance / normal angle    */
    int max_iteration;
    double confidence;
    uint64_t seed;
    int batch_size;              /* hypotheses per launch; 0 = the library's
                                    choice (adapts to the share that passes
                                    the checks)                              */
} o3dmi_ransac_options_t;

/* What the reference only logs. */
typedef struct {
    int64_t best_iteration;        /* -1: none                               */
    int64_t num_validations;       /* iterations that passed the checks and
                                      took part                              */
    int64_t final_iteration_bound; /* est_k when the loop ended              */
    int64_t iterations_run;        /* hypotheses formed, incl. the discarded
                                      tail of the last batch                 */
    int64_t num_batches;
} o3dmi_ransac_info_t;

/* Rule 7. The fields of the best iteration come from calling
 * o3dmi_registration_evaluate once more on T_best: result (transformation,
 * fitness, inlier_rmse) and the optional correspondences_dev (int64[ns]) are
 * bit for bit what that call returns. No iteration validated, or best fitness
 * 0: identity and zeros (the reference's default-constructed result;
 * correspondences_dev is then filled with -1). ransac_n < 3, fewer
 * correspondences than ransac_n, max_iteration <= 0 or
 * max_correspondence_distance <= 0 return that empty result with O3DMI_OK, as
 * the reference. estimation other than O3DMI_ICP_POINT_TO_POINT, with_scaling
 * or ransac_n > 8: O3DMI_ERR_UNSUPPORTED. A correspondence outside
 * [0, ns) x [0, nt): O3DMI_ERR_INVALID_ARG. corres_dev int64 {n_corres, 2};
 * normals may be NULL (the normal checker then passes). info may be NULL.
 * Synchronises; per batch the host reads back only the per-survivor arrays. */
int o3dmi_registration_ransac_correspondence(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        const void* source_normals_dev, const void* target_normals_dev,
        int dtype, const int64_t* corres_dev, int64_t n_corres,
        double max_correspondence_distance, int estimation, int with_scaling,
        int ransac_n, const o3dmi_ransac_options_t* options,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_ransac_info_t* info, o3dmi_stream_t stream);

/* = o3dmi_registration_correspondences_from_features(source_features,
 * target_features, mutual_filter, mutual consistency ratio 0.1) + the call
 * above. Features {ns, dim} / {nt, dim} of feature_dtype (Float32 / Float64),
 * row r belonging to point r. */
int o3dmi_registration_ransac_feature_matching(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        const void* source_normals_dev, const void* target_normals_dev,
        int dtype, const void* source_features_dev,
        const void* target_features_dev, int dim, int feature_dtype,
        int mutual_filter, double max_correspondence_distance, int estimation,
        int with_scaling, int ransac_n, const o3dmi_ransac_options_t* options,
        int64_t* correspondences_dev, o3dmi_registration_result_t* result,
        o3dmi_ransac_info_t* info, o3dmi_stream_t stream);

/* FastGlobalRegistrationBasedOnCorrespondence / ...BasedOnFeatureMatching
 * (legacy pipelines/registration/FastGlobalRegistration.cpp; legacy only, like
 * RANSAC above). Rules 1-4 are "Fast Global Registration" in o3d_mi355x.h;
 * the rest:
 *
 * 5. Result. With trans of rule 4, the means m_s, m_t and scale_global of rule
 *    1: G = [R | ((-(R m_t)) + t * scale_global) + m_s]
 *    (GetTransformationOriginalScale; R m_t summed left to right), and
 *    T = inverse(G) = [R^T | -(R^T g)], the rigid inverse, equal to rounding
 *    to Eigen's general inverse. fitness, inlier_rmse and the optional
 *    correspondences_dev (int64[ns]) are bit for bit what
 *    o3dmi_registration_evaluate(source, target,
 *    maximum_correspondence_distance, T) returns.
 * 6. Roles (feature entry point with tuple_test). When ns < nt the target is
 *    the query side of rules 2 and 3 (pairs (j, nearest i), the tuple test on
 *    (target, source)) and the pairs are swapped back afterwards, as upstream;
 *    the draws therefore index the swapped list. Without tuple_test the source
 *    is always the query side.
 *
 * iteration_number == 0 or fewer than 10 correspondences run rule 5 on the
 * identity. O3DMI_ERR_INVALID_ARG: maximum_tuple_count <= 0; division_factor,
 * tuple_scale or maximum_correspondence_distance not finite or <= 0;
 * iteration_number < 0; a correspondence outside [0, ns) x [0, nt); an empty
 * cloud; a non-finite coordinate; scale_global <= 0. A refused call writes
 * nothing. upstream defaults: 1.4, 0, 1, 0.025, 64, 0.95, 1000, 1. */
typedef struct {
    double division_factor;
    int use_absolute_scale;
    int decrease_mu;
    double maximum_correspondence_distance;
    int iteration_number;
    double tuple_scale;
    int maximum_tuple_count;
    int tuple_test;
    uint64_t seed;
} o3dmi_fgr_options_t;

/* What the reference only logs. */
typedef struct {
    int64_t n_initial;        /* pairs after rule 2 / pairs given            */
    int64_t n_trials;         /* trials upstream's loop would have run       */
    int64_t n_tuples;
    int64_t n_used;           /* correspondences the optimisation saw        */
    double scale_global;
    double final_par;
    int swapped;              /* rule 6                                      */
    int failed_solves;
    int form;                 /* 0 none (< 10), 1 resident, 2 streamed       */
} o3dmi_fgr_info_t;

/* corres_dev int64 {n_corres, 2} (source row, target row). info may be NULL.
 * The host waits once for the gate (finiteness, range and scales of rule 1 in
 * one download), once per batch of the tuple test, once for trans and in the
 * final evaluate; no wait sits inside the iteration loop. */
int o3dmi_registration_fgr_correspondence(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, const int64_t* corres_dev, int64_t n_corres,
        const o3dmi_fgr_options_t* options, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_fgr_info_t* info,
        o3dmi_stream_t stream);

/* Features {ns, dim} / {nt, dim} of feature_dtype (Float32 / Float64), row r
 * belonging to point r; rules 2 and 6, then as above (one more host wait, for
 * the pair count of rule 2). With tuple_test off the
 * result equals o3dmi_registration_fgr_correspondence on the pairs of rule 2,
 * bit for bit. */
int o3dmi_registration_fgr_feature_matching(
        const void* source_dev, int64_t ns, const void* target_dev, int64_t nt,
        int dtype, const void* source_features_dev,
        const void* target_features_dev, int dim, int feature_dtype,
        const o3dmi_fgr_options_t* options, int64_t* correspondences_dev,
        o3dmi_registration_result_t* result, o3dmi_fgr_info_t* info,
        o3dmi_stream_t stream);

/* GetCorrespondenceSetForPointCloudPair (t/pipelines/slac/SLACOptimizer.cpp:
 * 85-204) for the edge (i, j) of a pose graph: fragment i moved by T_ij is
 * hybrid-searched (radius distance_threshold, k = 1) in fragment j; the
 * matched {a, b} pairs go to corres_dev (int64, room for {ni,2}) in ascending
 * a, *n_corres = C. *n_inliers counts the pairs with
 * |Ti p_a - Tj q_b|^2 <= distance_threshold^2 (float32, <=), *inlier_ratio =
 * (float)n_inliers / (float)C (NaN when C = 0, as the reference's division).
 * *kept = 0 -- the reference returns an empty set -- iff (j != i + 1 and
 * inlier_ratio < fitness_threshold) or C = 0. T_i, T_j, T_ij: host 4x4
 * float64 row-major, cast to float32 first. Float32 positions only (the
 * reference loads every fragment as Float32). Synchronises. */
int o3dmi_slac_correspondence_set(const void* positions_i_dev, int64_t ni,
                                  const void* positions_j_dev, int64_t nj,
                                  int i, int j, const double* T_i,
                                  const double* T_j, const double* T_ij,
                                  float distance_threshold,
                                  float fitness_threshold,
                                  int64_t* corres_dev, int64_t* n_corres,
                                  int64_t* n_inliers, float* inlier_ratio,
                                  int* kept, o3dmi_stream_t stream);

/* RunRigidOptimizerForFragments (SLACOptimizer.cpp:265-286,369-414) on
 * fragments in device memory: "extended ICP to simultaneously align multiple
 * point clouds with dense pairwise point-to-plane distances".
 *   positions_dev / normals_dev [n_nodes]: device pointers, {sizes[k],3} float32
 *   poses {n_nodes,16}: float64 row-major node poses, in/out
 *   edges {n_edges,2} int32 (source, target), T_ij {n_edges,16} float64
 * The correspondence sets are computed once from the input graph (the call
 * above); an edge that is not kept contributes nothing. Per iteration: one
 * o3dmi_slac_rigid_terms launch with threshold = distance_threshold, one
 * download of n_edges x 29 doubles, the dense 6N x 6N float64 system on the
 * host with 1e5 on the first six diagonal entries, x = solve(AtA, -Atb) by LU
 * with partial pivoting, T_k <- PoseToTransformation(x[6k..6k+5]) T_k.
 * Outputs (each may be NULL): losses {max_iterations} = sum of the edges'
 * residuals (the reference's "Loss" log line), kept / n_corres {n_edges},
 * n_inliers {n_edges} = pairs within the threshold in the last iteration
 * (zeros when max_iterations <= 0).
 * Differences from the reference: fragments and correspondence sets are in
 * memory (the reference takes file names and caches .npy / .ply files in
 * slac_folder; its PreprocessPointClouds -- VoxelDownSample, statistical
 * outlier removal, EstimateNormals -- is the caller's); the sums, the solve
 * and the pose update are float64 (the reference: float32 atomics, a float32
 * gesv on a matrix holding 1e5 beside O(1) entries, poses rounded through
 * float32 every iteration). n_nodes > 512: O3DMI_ERR_UNSUPPORTED. i == j or a
 * node id out of range: O3DMI_ERR_INVALID_ARG. A zero or non-finite pivot
 * (for example a node no kept edge reaches; the reference's LAPACK check
 * throws): O3DMI_ERR_SINGULAR, and the poses are left as they came in.
 * Synchronises. */
int o3dmi_slac_rigid_optimize(const void* const* positions_dev,
                              const void* const* normals_dev,
                              const int64_t* sizes, int n_nodes, double* poses,
                              const int32_t* edges, const double* T_ij,
                              int n_edges, int max_iterations,
                              float distance_threshold,
                              float fitness_threshold, double* losses,
                              int32_t* kept, int64_t* n_corres,
                              int64_t* n_inliers, o3dmi_stream_t stream);

/* slac::ControlGrid (t/pipelines/slac/ControlGrid.{h,cpp}): a hashed lattice
 * of control points, key = lattice coordinate (int32 x 3), value = current
 * position (float32 x 3), with trilinear embedding of points and normals.
 * All point data is float32; every call synchronises unless it says otherwise.
 *
 * Differences from the reference: a point with a non-finite coordinate, or
 * whose cell leaves the hash's key range (|floor(p / grid_size)| < 2^20), is
 * never touched and never valid in parameterize (the reference casts such a
 * float to int32, which is undefined); parameterize keeps the INPUT order;
 * deform sums the eight corners in corner order 0..7; the projection's winner
 * on equal depth is the lowest point index (upstream's CUDA rule; its CPU path
 * takes arrival order).
 *
 * create: an empty grid with room for grid_count nodes. create_from: the
 * constructor slac_integrate uses, capacity 2 n, keys {n,3} int32 and values
 * {n,3} float32 on the device. grid_size <= 0, null pointers or negative
 * counts are O3DMI_ERR_INVALID_ARG everywhere. */
typedef struct o3dmi_control_grid o3dmi_control_grid_t;
int o3dmi_control_grid_create(float grid_size, int64_t grid_count,
                              o3dmi_stream_t stream,
                              o3dmi_control_grid_t** out);
int o3dmi_control_grid_create_from(float grid_size, const int32_t* keys_dev,
                                   const float* values_dev, int64_t n,
                                   o3dmi_stream_t stream,
                                   o3dmi_control_grid_t** out);
int o3dmi_control_grid_destroy(o3dmi_control_grid_t* g);
/* Touch (:46-80): inserts the eight corner nodes of the cell of every point,
 * value = key * grid_size. The insert is fed from the kernel (no 8 n candidate
 * list); a map that is too small grows (Reserve(max(wanted, 2 capacity))) and
 * the cloud is replayed, which moves the key / value buffers. */
int o3dmi_control_grid_touch(o3dmi_control_grid_t* g, const float* points_dev,
                             int64_t n, o3dmi_stream_t stream);
/* Compactify (:82-112): Reserve(2 size); the anchor is the active node at
 * position size / 2 of the active keys sorted by (z, y, x) (-1 when empty). */
int o3dmi_control_grid_compactify(o3dmi_control_grid_t* g,
                                  o3dmi_stream_t stream);
int o3dmi_control_grid_size(o3dmi_control_grid_t* g, o3dmi_stream_t stream,
                            int64_t* size);
int o3dmi_control_grid_anchor_idx(const o3dmi_control_grid_t* g);
float o3dmi_control_grid_grid_size(const o3dmi_control_grid_t* g);
/* The node map: o3dmi_hash_active_indices / _find / _key_buffer work on it. */
o3dmi_hash_t* o3dmi_control_grid_hashmap(o3dmi_control_grid_t* g);
/* {capacity,3}: key * grid_size of every buffer row (0 for unused rows).
 * Asynchronous. */
int o3dmi_control_grid_init_positions(o3dmi_control_grid_t* g, float* out_dev,
                                      o3dmi_stream_t stream);
/* The value buffer itself, {capacity,3} float32, writable; a touch, a
 * compactify or a Reserve of the map moves it. */
float* o3dmi_control_grid_curr_positions(o3dmi_control_grid_t* g);
/* GetNeighborGridMap (:114-148): the active buffer indices in ascending order
 * (active_dev, room for `capacity`), and for each the buffer indices {n,6}
 * int32 and masks {n,6} uint8 of its -x +x -y +y -z +z neighbours (index 0
 * where the mask is 0). */
int o3dmi_control_grid_neighbor_grid_map(o3dmi_control_grid_t* g,
                                         int32_t* active_dev,
                                         int32_t* nb_indices_dev,
                                         uint8_t* nb_masks_dev, int64_t* n_out,
                                         o3dmi_stream_t stream);
/* Parameterize (:150-239): the points whose eight corners are all nodes, in
 * input order, with their corner buffer indices {m,8} int32, vertex ratios
 * {m,8} and -- with normals -- normal ratios {m,8}. normals_dev / colors_dev
 * and their outputs may be NULL. *m_out receives the count; more than
 * out_capacity rows: O3DMI_ERR_CAPACITY, nothing written. */
int o3dmi_control_grid_parameterize(
        o3dmi_control_grid_t* g, const float* points_dev,
        const float* normals_dev, const float* colors_dev, int64_t n,
        int64_t out_capacity, float* out_points_dev, float* out_normals_dev,
        float* out_colors_dev, int32_t* out_indices_dev,
        float* out_vertex_ratios_dev, float* out_normal_ratios_dev,
        int64_t* m_out, o3dmi_stream_t stream);
/* Deform (:241-288) of a parameterized cloud: position = sum_k ratio_k curr_k,
 * normal = the same sum with the normal ratios, normalised. An index outside
 * [0, capacity): O3DMI_ERR_INVALID_ARG, nothing written (checked on the
 * device). normal_ratios_dev / out_normals_dev may be NULL. */
int o3dmi_control_grid_deform(o3dmi_control_grid_t* g,
                              const int32_t* indices_dev,
                              const float* vertex_ratios_dev,
                              const float* normal_ratios_dev, int64_t n,
                              float* out_points_dev, float* out_normals_dev,
                              o3dmi_stream_t stream);
/* PointCloud::ProjectToDepthImage / ProjectToRGBDImage (t/geometry/
 * PointCloud.cpp:1471-1530, kernel/PointCloudCUDA.cu:26-160): u, v =
 * round(project); skipped when out of bounds, zc <= 0 or zc > depth_max;
 * d = zc * depth_scale; the smallest (d, point index) of a pixel wins; empty
 * pixels are 0. depth_out_dev {rows,cols} float32, color_out_dev
 * {rows,cols,3} float32. n < 2^32. Two launches; waits for them (the packed
 * words are pooled scratch). */
int o3dmi_project_to_depth_image(const float* points_dev, int64_t n, int rows,
                                 int cols, const double* intrinsic,
                                 const double* extrinsic, float depth_scale,
                                 float depth_max, float* depth_out_dev,
                                 o3dmi_stream_t stream);
int o3dmi_project_to_rgbd_image(const float* points_dev,
                                const float* colors_dev, int64_t n, int rows,
                                int cols, const double* intrinsic,
                                const double* extrinsic, float depth_scale,
                                float depth_max, float* depth_out_dev,
                                float* color_out_dev, o3dmi_stream_t stream);
/* Deform of a depth / RGB-D image (:290-322), fused: bit for bit what
 * o3dmi_unproject (stride 1) -> parameterize -> deform -> project give, in two
 * launches and without the compacted cloud. depth_dtype O3DMI_U16 or
 * O3DMI_F32; color_dtype O3DMI_U8 ({rows,cols,3}, scaled by 1/255 as
 * Image::To does) or O3DMI_F32. Waits for its two launches. */
int o3dmi_control_grid_deform_depth_image(
        o3dmi_control_grid_t* g, const void* depth_dev, int depth_dtype,
        int rows, int cols, const double* intrinsic, const double* extrinsic,
        float depth_scale, float depth_max, float* depth_out_dev,
        o3dmi_stream_t stream);
int o3dmi_control_grid_deform_rgbd_image(
        o3dmi_control_grid_t* g, const void* depth_dev, int depth_dtype,
        const void* color_dev, int color_dtype, int rows, int cols,
        const double* intrinsic, const double* extrinsic, float depth_scale,
        float depth_max, float* depth_out_dev, float* color_out_dev,
        o3dmi_stream_t stream);

/* The non-rigid SLAC optimizer (t/pipelines/slac/SLACOptimizer.cpp:253-367,
 * slac/FillInLinearSystemImpl.h:102-236, kernel/FillInLinearSystemImpl.h:
 * 156-524). Unknowns: 6 per fragment, then 3 per control node, n_vars in all.
 *
 * o3dmi_fill_in_slac_alignment_term is kernel::FillInSLACAlignmentTerm: the
 * 60 x 60 block J J^T, 60 values J r and r r of every pair with
 * |r| <= threshold are added to the float32 AtA {n_vars,n_vars}, Atb {n_vars},
 * residual {1} in place. The nine per-pair arrays ({n,3} float32, {n,8} int32
 * indices, {n,8} float32 ratios) are the reference's, with each ratio array
 * beside its own index array; an index is the reference's raw cgrid_idx, its
 * unknowns are 6 n_frags + 3 idx + {0,1,2}. Differences from the reference:
 * the products are float32 in its expressions but every sum is float64 and
 * each entry of the output is updated once, by the float32 rounding of its
 * sum; 6 n_frags + 3 idx + 2 >= n_vars or idx < 0 (checked on the device) is
 * O3DMI_ERR_INVALID_ARG with nothing written, where the reference indexes out
 * of bounds. n_vars > 32768: O3DMI_ERR_UNSUPPORTED. Cost: every call
 * allocates and zeroes a float64 {n_vars,n_vars} scratch and passes over all
 * n_vars^2 entries of AtA once (8.6 GB at the limit), so a one-fill-per-edge
 * loop is O(E n_vars^2); the seam is for parity and small systems,
 * o3dmi_slac_optimize fills one float64 system for all edges. Synchronises. */
int o3dmi_fill_in_slac_alignment_term(
        float* AtA_dev, float* Atb_dev, float* residual_dev, int64_t n_vars,
        const float* Ti_Cps_dev, const float* Tj_Cqs_dev,
        const float* Cnormal_ps_dev, const float* Ri_Cnormal_ps_dev,
        const float* RjT_Ri_Cnormal_ps_dev, const int32_t* cgrid_idx_ps_dev,
        const int32_t* cgrid_idx_qs_dev, const float* cgrid_ratio_ps_dev,
        const float* cgrid_ratio_qs_dev, int64_t n, int i, int j, int n_frags,
        float threshold, o3dmi_stream_t stream);

/* kernel::FillInSLACRegularizerTerm over GetNeighborGridMap's output
 * (grid_idx {n}, grid_nbs_idx {n,6} int32, grid_nbs_mask {n,6} bytes) and the
 * init / curr positions ({n_positions,3} float32), same seam rules and the
 * same range check as above. A node with fewer than three masked neighbours is
 * skipped; the local rotation comes from a converged float64 Jacobi SVD of the
 * float32 covariance (the reference: its approximate float32 svd3x3), with
 * det = +1 and the identity at anchor_idx. weight = n_frags x
 * regularizer_weight is the caller's product. */
int o3dmi_fill_in_slac_regularizer_term(
        float* AtA_dev, float* Atb_dev, float* residual_dev, int64_t n_vars,
        const int32_t* grid_idx_dev, const int32_t* grid_nbs_idx_dev,
        const uint8_t* grid_nbs_mask_dev, int64_t n,
        const float* positions_init_dev, const float* positions_curr_dev,
        int64_t n_positions, float weight, int n_frags, int anchor_idx,
        o3dmi_stream_t stream);

/* x = solve(A, b) for a symmetric positive definite float64 A {n,n} given by
 * its lower triangle (row-major; the upper triangle is never read or
 * written): blocked Cholesky in place (A becomes L), b becomes x. A pivot that
 * is <= 0 or not finite: O3DMI_ERR_SINGULAR (A and b are then partly
 * overwritten). n > 32768: O3DMI_ERR_UNSUPPORTED before anything is allocated.
 * Synchronises. */
int o3dmi_slac_solve_spd(double* A_dev, double* b_dev, int64_t n,
                         o3dmi_stream_t stream);

/* RunSLACOptimizerForFragments on fragments in device memory. Fragments,
 * poses, edges, T_ij, thresholds, kept / n_corres / n_inliers and the limits
 * (512 nodes, node ids, empty fragments) as o3dmi_slac_rigid_optimize.
 * grid: an empty grid is touched with every fragment and compactified
 * (InitializeControlGrid; the reference creates it with 3.0 / 8 and 8000); one
 * that has nodes is used as it is, so a run can be continued. Node g of the
 * ascending active buffer-index list owns the unknowns 6 n_nodes + 3 g + ..
 * (the reference uses the raw buffer index and leaves the matrix when the
 * indices are not 0..G-1). Per iteration: zero the float64 system, ones on the
 * first six diagonal entries, one launch for the alignment terms of all edges
 * (threshold = distance_threshold), the regularizer with weight n_nodes x
 * regularizer_weight, the anchor node's three unknowns taken out (see below),
 * x = solve_spd(AtA, -Atb), T_k <-
 * PoseToTransformation(x[6k..]) T_k in float64, curr_positions[active[g]] +=
 * (float)x[6 n_nodes + 3 g ..]. A correspondence with a point whose cell has
 * an inactive corner contributes nothing (the reference drops the point in
 * Parameterize and then fails on the length mismatch); *skipped is their
 * number in the last iteration. alignment_losses / regularizer_losses
 * {max_iterations}: the two residuals before each step. Outputs may be NULL.
 * The anchor: the reference's system is singular -- moving every node by t
 * and translating fragment k >= 1 by (R_0 - R_k) t changes no term, and the
 * ones on the first six diagonals only hold fragment 0 -- and its LU returns
 * one of the solutions, chosen by rounding noise. Here the anchor node of
 * Compactify keeps its position (a grid that has nodes but no anchor, one
 * that was never compactified, is O3DMI_ERR_INVALID_ARG): identity rows and columns, rhs 0. Everything that can be observed
 * (residuals, deformed points up to a common translation, nodes relative to
 * the anchor) is the same for every solution.
 * 6 n_nodes + 3 G > 32768: O3DMI_ERR_UNSUPPORTED. A pivot <= 0 (a node no kept
 * edge reaches): O3DMI_ERR_SINGULAR; poses and node positions are then as they
 * came in; the same holds for every other error. A correspondence or node
 * index out of range inside the driver is O3DMI_ERR_INTERNAL, not the seams'
 * O3DMI_ERR_INVALID_ARG: the driver computes both itself. Synchronises. */
int o3dmi_slac_optimize(
        const void* const* positions_dev, const void* const* normals_dev,
        const int64_t* sizes, int n_nodes, double* poses, const int32_t* edges,
        const double* T_ij, int n_edges, o3dmi_control_grid_t* grid,
        int max_iterations, float distance_threshold, float fitness_threshold,
        float regularizer_weight, double* alignment_losses,
        double* regularizer_losses, int32_t* kept, int64_t* n_corres,
        int64_t* n_inliers, int64_t* skipped, o3dmi_stream_t stream);

/* PointCloud::VoxelDownSample (t/geometry/PointCloud.cpp:496-567) for
 * positions (+ optional normals): mean per voxel in float32, voxel order =
 * order of first occurrence. Outputs must hold n rows; *m_out receives the
 * number of voxels (synchronises). */
int o3dmi_voxel_down_sample(const void* positions_dev, const void* normals_dev,
                            int64_t n, int dtype, double voxel_size,
                            void* out_positions_dev, void* out_normals_dev,
                            int64_t* m_out, o3dmi_stream_t stream);

/* PointCloud::EstimateNormals(max_nn, radius) (t/geometry/PointCloud.cpp:
 * 856-976): normals {n,3} (in/out when has_normals). radius > 0 and max_nn > 0
 * = hybrid search; radius <= 0 = KNN search (the reference's default
 * max_nn = 30, radius = nullopt); max_nn <= 0 = radius search (every
 * neighbour within radius); max_nn <= 64 otherwise. Synchronises.
 * Parity: neighbour sets and covariances are the reference's bit for bit;
 * the eigenvector is this library's own float64 routine (see
 * o3dmi_pointcloud_normals_from_covariances): a TOLERANCE against the
 * reference's closed form, with a pinned sign. */
int o3dmi_pointcloud_estimate_normals(const void* points_dev, int64_t n,
                                      int dtype, int max_nn, double radius,
                                      void* normals_dev, int has_normals,
                                      o3dmi_stream_t stream);

/* InitializePointCloudForGeneralizedICP's covariances from normals (legacy
 * GeneralizedICP.cpp:33-80): covariances {n,3,3} = Rx diag(epsilon,1,1) Rx^T
 * with Rx = GetRotationFromE1ToX(normal), one thread per point, the
 * reference's statements in float64 without contraction, narrowed to the point
 * dtype once. Where e1 . x < -0.99 Rx is the identity (the reference's branch,
 * kept); normals are not re-normalised. epsilon <= 0 or non-finite:
 * O3DMI_ERR_INVALID_ARG (the reference does not check). Asynchronous. */
int o3dmi_pointcloud_covariances_from_normals(const void* normals_dev,
                                              int64_t n, int dtype,
                                              double epsilon,
                                              void* covariances_dev,
                                              o3dmi_stream_t stream);

/* PointCloud::EstimateColorGradients(max_nn, radius) (t/geometry/PointCloud.
 * cpp:987-1060): hybrid search when both are given, KNN search when
 * radius <= 0, radius search (every neighbour within radius) when
 * max_nn <= 0; gradients {n,3} in the point dtype. max_nn <= 64 otherwise.
 * Synchronises.
 * Parity is a TOLERANCE, not bits: the reference solves each point's 3x3
 * normal equations with an approximate SVD (core/linalg/kernel/SVD3x3.h, four
 * fixed sweeps; its Float64 instantiation is broken), this library with a
 * converged pseudo-inverse. Against the reference's Float32 body: median
 * 1e-7 of the gradient scale, a percent-level tail on ill-conditioned
 * neighbourhoods (tests bound the 99th percentile at 0.15); against numpy's
 * pseudo-inverse: exact. The reference-arithmetic routine lives on as test
 * infrastructure only (oracle/approx_svd3_oracle.h). */
int o3dmi_pointcloud_estimate_color_gradients(
        const void* points_dev, const void* normals_dev, const void* colors_dev,
        int64_t n, int dtype, int max_nn, double radius, void* gradients_dev,
        o3dmi_stream_t stream);

/* PointCloud::SelectByMask (t/geometry/PointCloud.cpp:435-459) for up to 8
 * attributes at once: attribute a has n rows of row_bytes[a] >= 1 bytes at
 * attrs_in[a] (12 / 24 for positions and normals, 3 for uint8 colours, ...);
 * the rows with (mask != 0) != invert go to attrs_out[a], which must hold n
 * rows, IN INPUT ORDER on every run. mask_dev: uint8 {n}. *m_out receives the
 * number of rows kept (synchronises). n_attrs outside [1, 8], a NULL pointer
 * or n < 0: O3DMI_ERR_INVALID_ARG before anything is written. */
int o3dmi_pointcloud_select_by_mask(int64_t n, const uint8_t* mask_dev,
                                    int invert, int n_attrs,
                                    const void* const* attrs_in,
                                    const int64_t* row_bytes,
                                    void* const* attrs_out, int64_t* m_out,
                                    o3dmi_stream_t stream);

/* PointCloud::SelectByIndex (t/geometry/PointCloud.cpp:461-494). indices_dev:
 * int64 {m}. Plain form (invert = remove_duplicates = 0): a row gather,
 * duplicates repeat, attrs_out hold m rows. Otherwise index -> mask ->
 * SelectByMask as upstream (rows in input order, each once), attrs_out hold n
 * rows. An index outside [0, n) is O3DMI_ERR_INVALID_ARG with nothing written
 * (checked on the device first; upstream reads out of bounds). Synchronises. */
int o3dmi_pointcloud_select_by_index(int64_t n, const int64_t* indices_dev,
                                     int64_t m, int invert,
                                     int remove_duplicates, int n_attrs,
                                     const void* const* attrs_in,
                                     const int64_t* row_bytes,
                                     void* const* attrs_out, int64_t* m_out,
                                     o3dmi_stream_t stream);

/* The Remove* filters below return a uint8 mask {n} (1 = kept) and the number
 * of ones in *m_out; SelectByMask applies it to the attributes. All
 * synchronise. n == 0: O3DMI_OK, *m_out = 0. */

/* PointCloud::RemoveNonFinitePoints (t/geometry/PointCloud.cpp:716-738). */
int o3dmi_pointcloud_remove_non_finite_points(const void* points_dev,
                                              int64_t n, int dtype,
                                              int remove_nan, int remove_inf,
                                              uint8_t* mask_out_dev,
                                              int64_t* m_out,
                                              o3dmi_stream_t stream);

/* PointCloud::RemoveDuplicatedPoints (t/geometry/PointCloud.cpp:740-760): the
 * key is the bit pattern of the three coordinates (+0 and -0 differ, NaNs of
 * equal bits are equal). Of every key the LOWEST index is kept, on every run
 * (upstream: whichever thread inserts first). n < 2^30. */
int o3dmi_pointcloud_remove_duplicated_points(const void* points_dev,
                                              int64_t n, int dtype,
                                              uint8_t* mask_out_dev,
                                              int64_t* m_out,
                                              o3dmi_stream_t stream);

/* PointCloud::RemoveRadiusOutliers (t/geometry/PointCloud.cpp:650-676):
 * mask_i = (points with d2 < r2 of point i, itself included) >= nb_points;
 * r2 = search_radius squared in the point dtype, the comparison strict.
 * nb_points < 1 or search_radius <= 0: O3DMI_ERR_INVALID_ARG; so is a NaN or
 * Inf coordinate (upstream: undefined -- run RemoveNonFinitePoints first),
 * with the mask untouched. */
int o3dmi_pointcloud_remove_radius_outliers(const void* points_dev, int64_t n,
                                            int dtype, int64_t nb_points,
                                            double search_radius,
                                            uint8_t* mask_out_dev,
                                            int64_t* m_out,
                                            o3dmi_stream_t stream);

/* PointCloud::RemoveStatisticalOutliers (t/geometry/PointCloud.cpp:678-714).
 * avg_i = (sum over the k' = min(nb_neighbors, n) nearest points, i itself
 * first, ascending by (d2, index), of sqrt(d2)) / k', summed and divided in
 * the point dtype; no {n, k} neighbour table is allocated. mean = sum avg / n,
 * S = sum ((double)avg - mean)^2 as float64 sums in a fixed tree (same bits on
 * every run), std = sqrt(S / (n - 1)), threshold = mean + std_ratio * std,
 * mask_i = (double)avg_i <= threshold. n == 1: std is NaN, nothing is kept.
 * avg_distances_out_dev (optional): {n} in the point dtype; stats_out
 * (optional, host): {mean, std, threshold}. nb_neighbors < 1, std_ratio <= 0
 * or a NaN / Inf coordinate: O3DMI_ERR_INVALID_ARG, mask untouched;
 * nb_neighbors > 64: O3DMI_ERR_UNSUPPORTED (upstream: no limit). */
int o3dmi_pointcloud_remove_statistical_outliers(
        const void* points_dev, int64_t n, int dtype, int64_t nb_neighbors,
        double std_ratio, uint8_t* mask_out_dev, void* avg_distances_out_dev,
        double* stats_out, int64_t* m_out, o3dmi_stream_t stream);

/* PointCloud::ClusterDBSCAN (t/geometry/PointCloud.cpp:1634-1648 -> legacy
 * geometry/PointCloudCluster.cpp:21-97; upstream has no device path). The
 * labels are those of upstream's sequential loop, the same on every run:
 * neighbourhood of i = the points with d2 < eps^2 (strict, i included, d2 and
 * eps^2 in the point dtype: the radius rule of o3dmi_nns_*); a core point has
 * >= min_points of them (0 and 1 make every point core). A cluster is a
 * connected component of core points under "within eps"; clusters are
 * numbered 0, 1, ... in ascending order of their LOWEST CORE INDEX (the order
 * in which upstream's outer loop meets their seeds). A non-core point with a
 * core neighbour takes the smallest label among its core neighbours
 * (upstream expands clusters one after another, never relabels a label >= 0
 * and overwrites an earlier -1); every other point is -1. Upstream widens
 * Float32 clouds to float64 before the search, so a pair within rounding of
 * eps may differ.
 * labels_out_dev int32 {n}; num_clusters_out / num_noise_out (optional, host)
 * = number of clusters / of -1 labels. n == 0: O3DMI_OK, both 0. eps <= 0,
 * min_points < 0, a NULL pointer or a NaN / Inf coordinate:
 * O3DMI_ERR_INVALID_ARG with the labels untouched. n < 2^27. Synchronises. */
int o3dmi_pointcloud_cluster_dbscan(const void* points_dev, int64_t n,
                                    int dtype, double eps, int64_t min_points,
                                    int32_t* labels_out_dev,
                                    int64_t* num_clusters_out,
                                    int64_t* num_noise_out,
                                    o3dmi_stream_t stream);

/* What upstream's SegmentPlane only logs. */
typedef struct {
    int64_t best_iteration;        /* -1: none                               */
    int64_t iterations_counted;    /* iterations that formed a plane and took
                                      part                                   */
    int64_t final_break_iteration; /* the bound when the loop ended          */
    double fitness;                /* of the best iteration: inliers / n     */
    double inlier_rmse;            /* sqrt(sum d^2 / inliers)                */
} o3dmi_segment_plane_info_t;

/* PointCloud::SegmentPlane (t/geometry/PointCloud.cpp:1650-1666 -> legacy
 * geometry/PointCloudSegmentation.cpp:157-279). The result is that of
 * upstream's loop run by ONE thread in iteration order, whatever the batch
 * size, over the samples of o3dmi_plane_sample(seed, i, ...):
 *  - hypothesis, float64 on the widened coordinates: ransac_n == 3
 *    ComputeTrianglePlane, else GetPlaneFromPoints on the sample; norms are
 *    sqrt((x x + y y) + z z). A zero plane is skipped and NOT counted.
 *  - score: o3dmi_plane_score; fitness = count / n, rmse = sqrt(sum / count).
 *    Upstream adds d^2 in index order and leaves the dot product's order to
 *    Eigen: a rounding difference at the threshold and in the rmse.
 *  - iteration i takes part iff iterations_counted <= break_iteration as the
 *    iterations before it left them; a new best needs a strictly better
 *    (fitness, then rmse), so the lower iteration keeps a tie; then
 *    break_iteration = trunc(min(log(1 - p) / log(1 - fitness^ransac_n),
 *    num_iterations)), 0 when fitness == 1, and num_iterations when the
 *    denominator is 0 or the quotient is not a finite number >= 0 (upstream's
 *    cast is undefined there). Work a batch did past the bound is dropped.
 *  - final: the inliers of the best plane, ascending, in inliers_out_dev
 *    (int64, room for n), *m_out of them; plane_out = GetPlaneFromPoints over
 *    them (centroid and centred sums as float64 partials in a fixed tree, the
 *    closed form on the host). No iteration formed a plane with an inlier:
 *    plane (0,0,0,0), m = 0, O3DMI_OK (upstream returns NaNs).
 * probability <= 0 or > 1, ransac_n < 3, n < ransac_n, num_iterations < 1,
 * distance_threshold <= 0 or a NaN / Inf coordinate: O3DMI_ERR_INVALID_ARG
 * with nothing written (upstream checks none of the last three);
 * ransac_n > 8: O3DMI_ERR_UNSUPPORTED. info_out may be NULL. Synchronises; per
 * batch the host reads back {count, sum, valid} of every hypothesis. */
int o3dmi_pointcloud_segment_plane(const void* points_dev, int64_t n,
                                   int dtype, double distance_threshold,
                                   int ransac_n, int64_t num_iterations,
                                   double probability, uint64_t seed,
                                   double plane_out[4],
                                   int64_t* inliers_out_dev, int64_t* m_out,
                                   o3dmi_segment_plane_info_t* info_out,
                                   o3dmi_stream_t stream);

/* ---- PointCloud sampling, cropping and bounds ----------------------------
 * (t/geometry/PointCloud.cpp:569-648, 1668-1720; kernels t/geometry/kernel/
 * PointCloudImpl.h:147-226.) Float32 / Float64. All synchronise. */

/* The order in which PointCloud::FarthestPointDownSample (t/geometry/
 * PointCloud.cpp:612-648) picks its samples, with the two points upstream
 * leaves open pinned:
 *   dist_j = +inf, sel = start_index;
 *   for i = 0 .. num_samples - 1:
 *       order[i] = sel;
 *       dist_j = min(dist_j, ((dx dx) + dy dy) + dz dz), d = p_j - p_sel, in
 *                the point dtype, no FMA;
 *       sel = the LOWEST INDEX among the maxima of dist.
 * Squares that overflow to +inf are legal and tie at +inf like any other
 * value. Once every remaining point coincides with a chosen one the maximum is
 * 0 and sel is 0 from then on, so order may repeat indices.
 * form 0 picks the kernel form by n, 1 asks for the resident form (one launch,
 * the cloud in one workgroup's registers; n above
 * o3dmi_pointcloud_farthest_point_capacity: O3DMI_ERR_UNSUPPORTED), 2 for the
 * streamed form (one launch per sample, no host wait in between). (max value,
 * min index) is associative and commutative: all forms give the same bits.
 * order_out_dev: int64 {num_samples}. num_samples > n, start_index outside
 * [0, n) (n == 0 with num_samples == 0 is O3DMI_OK), n < 0, n >= 2^27, a NULL
 * pointer, a dtype other than Float32 / Float64, form outside 0..2 or a NaN /
 * Inf coordinate: O3DMI_ERR_INVALID_ARG with the outputs untouched. */
int o3dmi_pointcloud_farthest_point_order(const void* points_dev, int64_t n,
                                          int dtype, int64_t num_samples,
                                          int64_t start_index, int form,
                                          int64_t* order_out_dev,
                                          o3dmi_stream_t stream);

/* Points the resident form holds (0 for an unknown dtype): the largest cloud
 * form 0 gives to it. */
int64_t o3dmi_pointcloud_farthest_point_capacity(int dtype);

/* PointCloud::FarthestPointDownSample as a mask, in the style of the Remove*
 * filters: mask_out_dev uint8 {n} has a one at every index of the order above
 * (form 0), *m_out their number; SelectByMask then gives the rows in input
 * order, as upstream. On a cloud with fewer than num_samples distinct points
 * the mask has FEWER THAN num_samples ONES (upstream's tensor path: the same
 * wherever its ArgMax returns the first maximum; the legacy path re-selects
 * the previous index instead). num_samples == 0 clears the mask; num_samples
 * == n sets all of it (upstream's Clone()) and runs the loop only when
 * order_out_dev (optional, int64 {num_samples}) is given. Errors as above. */
int o3dmi_pointcloud_farthest_point_down_sample(
        const void* points_dev, int64_t n, int dtype, int64_t num_samples,
        int64_t start_index, uint8_t* mask_out_dev, int64_t* order_out_dev,
        int64_t* m_out, o3dmi_stream_t stream);

/* PointCloud::UniformDownSample (t/geometry/PointCloud.cpp:569-585): output
 * row i of every attribute is input row i * every_k_points; *m_out =
 * ceil(n / every_k_points) rows, which attrs_out must hold. Attributes as in
 * o3dmi_pointcloud_select_by_mask. every_k_points < 1: O3DMI_ERR_INVALID_ARG. */
int o3dmi_pointcloud_uniform_down_sample(int64_t n, int64_t every_k_points,
                                         int n_attrs,
                                         const void* const* attrs_in,
                                         const int64_t* row_bytes,
                                         void* const* attrs_out,
                                         int64_t* m_out,
                                         o3dmi_stream_t stream);

/* Entry j of the permutation of [0, n) that seed selects (pure host function;
 * -1 unless 0 <= j < n < 2^62): four Feistel rounds over the lowest even
 * power of two >= n, cycle-walked back into [0, n). */
int64_t o3dmi_sample_index(uint64_t seed, int64_t n, int64_t j);

/* The indices PointCloud::RandomDownSample (t/geometry/PointCloud.cpp:587-610)
 * gathers: *m_out = (int64)(sampling_ratio * n), upstream's truncation;
 * indices_out_dev[j] = o3dmi_sample_index(seed, n, j) for j < m, all distinct.
 * The plain o3dmi_pointcloud_select_by_index then gathers the rows in that
 * order, as upstream gathers in shuffled order. Upstream shuffles with its
 * global Mersenne engine under a mutex; here the sample is a pure function of
 * (seed, n), the same on every run. indices_out_dev: int64, room for n.
 * A ratio outside [0, 1] or NaN: O3DMI_ERR_INVALID_ARG. */
int o3dmi_pointcloud_random_sample_indices(int64_t n, double sampling_ratio,
                                           uint64_t seed,
                                           int64_t* indices_out_dev,
                                           int64_t* m_out,
                                           o3dmi_stream_t stream);

/* AxisAlignedBoundingBox::GetPointIndicesWithinBoundingBox's mask
 * (GetPointMaskWithinAABB, PointCloudImpl.h:147-180): the bounds are rounded
 * to the point dtype, both ends are inclusive. A NaN coordinate fails every
 * comparison: outside (non-finite clouds are not refused here). A box of zero
 * volume is no error. max < min on an axis, a NaN bound or a NULL pointer:
 * O3DMI_ERR_INVALID_ARG. mask_out_dev uint8 {n}, *m_out its ones. */
int o3dmi_pointcloud_aabb_mask(const void* points_dev, int64_t n, int dtype,
                               const double min_bound[3],
                               const double max_bound[3],
                               uint8_t* mask_out_dev, int64_t* m_out,
                               o3dmi_stream_t stream);

/* OrientedBoundingBox's mask (GetPointMaskWithinOBB, PointCloudImpl.h:
 * 183-226), all in the point dtype: pd = p - center, half = extent / 2, axis k
 * = column k of rotation (row-major {3,3}); inside when
 * |((pd0 r0k) + pd1 r1k) + pd2 r2k| <= half_k on all three axes. NaN rows and
 * empty boxes as above. A negative or NaN extent: O3DMI_ERR_INVALID_ARG. */
int o3dmi_pointcloud_obb_mask(const void* points_dev, int64_t n, int dtype,
                              const double center[3], const double rotation[9],
                              const double extent[3], uint8_t* mask_out_dev,
                              int64_t* m_out, o3dmi_stream_t stream);

/* PointCloud::GetMinBound / GetMaxBound (and so GetAxisAlignedBoundingBox):
 * the per-axis minimum and maximum as host doubles, exact. n == 0 gives
 * zeros, as upstream. A NaN coordinate is skipped. */
int o3dmi_pointcloud_min_max_bound(const void* points_dev, int64_t n,
                                   int dtype, double min_out[3],
                                   double max_out[3], o3dmi_stream_t stream);

/* ---- PointCloud metrics and nearest-point distances ------------------------
 * (t/geometry/PointCloud.cpp:1805-1836, t/geometry/kernel/Metrics.cpp;
 * geometry/PointCloud.cpp:133-157. Upstream has no device path: it copies the
 * clouds to the host and searches two k-d trees.) Float32 / Float64. All
 * synchronise. The distance of a query is sqrt(d2) in the point dtype, d2 =
 * the minimum over the target of ((dx dx) + dy dy) + dz dz with dx = query -
 * point in the point dtype, no FMA: the d2 of every search here. The search is
 * exact and has no radius: a group of 16 lanes walks the growing cubes of the
 * finest level of the o3dmi_nns_knn_search index (k = 1) for a query; the
 * queries that level cannot finish go through that search's second pass.
 * Size limits are o3dmi_nns_knn_search's (fewer than 2^31 - 1 points a
 * cloud). */

/* ComputePointCloudDistance with the index as an extra: dist_out_dev {q} in
 * the point dtype, idx_out_dev {q} int32 (optional) = the LOWEST original
 * index among the nearest target points. q == 0 is O3DMI_OK with nothing
 * written. An empty target (upstream: error), n or q negative or out of
 * range, a NULL pointer, a dtype other than Float32 / Float64 or a NaN / Inf
 * coordinate in either cloud: O3DMI_ERR_INVALID_ARG with the outputs
 * untouched. */
int o3dmi_pointcloud_nearest_distance(const void* target_dev, int64_t n,
                                      const void* queries_dev, int64_t q,
                                      int dtype, void* dist_out_dev,
                                      int32_t* idx_out_dev,
                                      o3dmi_stream_t stream);

/* Metric codes: upstream's enum order (t/geometry/Geometry.h). */
typedef enum {
    O3DMI_METRIC_CHAMFER_DISTANCE = 0,
    O3DMI_METRIC_HAUSDORFF_DISTANCE = 1,
    O3DMI_METRIC_FSCORE = 2
} o3dmi_metric_t;

/* What the metrics are made of, per direction: [0] is cloud 1 -> cloud 2 (the
 * n1 distances of upstream's distance12), [1] cloud 2 -> cloud 1.
 *  - sum: the float64 sum of the distances in a fixed tree: consecutive runs
 *    of 512 values are added in index order, the run sums likewise, level by
 *    level until one value is left (the tile convention of o3dmi_plane_score).
 *    The same bits on every run.
 *  - max: the largest distance, widened to double.
 *  - counts: set by the CALLER to an int64 array of 2 * n_radii entries (or
 *    NULL: not wanted); counts[d * n_radii + r] = the number of distances of
 *    direction d with dist < fscore_radius[r] (strict; a Float32 cloud compares
 *    in Float32, a Float64 cloud against the radius widened to double).
 *  - second_pass_queries: the queries the lane-group pass left to the second
 *    pass (far from the target, or in a sparse region of it). */
typedef struct {
    double sum[2];
    double max[2];
    int64_t* counts;
    int64_t second_pass_queries[2];
} o3dmi_pointcloud_metrics_raw_t;

/* ComputeMetricsCommon (t/geometry/kernel/Metrics.cpp:16-66) statement for
 * statement, on sums instead of distance tensors; a pure host function. With
 * mean12 = (float)(sum[0] / n1), mean21 = (float)(sum[1] / n2), in float:
 *   ChamferDistance   = mean21 + mean12
 *   HausdorffDistance = max((float)max[0], (float)max[1])
 *   FScore at radius r: precision = (float)((double)(float)counts[r] *
 *       (100.0 / n1)), recall likewise from counts[n_radii + r] and n2;
 *       2 * precision * recall / (precision + recall), or 0 unless
 *       precision + recall > 0.
 * Values come out in the order of metrics[]; EVERY FScore entry expands to
 * n_radii values (upstream sizes its output for one). n1 or n2 < 1, an unknown
 * code, FScore with n_radii < 1, a negative count or a NULL pointer:
 * O3DMI_ERR_INVALID_ARG; values_capacity below the number of values:
 * O3DMI_ERR_CAPACITY; values_out untouched in both cases. */
int o3dmi_metrics_from_sums(int64_t n1, int64_t n2, const double sum[2],
                            const double max[2], const int64_t* counts,
                            int n_radii, const int32_t* metrics, int n_metrics,
                            float* values_out, int64_t values_capacity);

/* PointCloud::ComputeMetrics: both directed nearest-point distance sets, their
 * reduction on the device and o3dmi_metrics_from_sums. values_out is a HOST
 * float array of values_capacity entries; raw_out (optional) receives the
 * sums. Errors are those of o3dmi_metrics_from_sums and of
 * o3dmi_pointcloud_nearest_distance (an empty cloud and a NaN / Inf coordinate
 * in either cloud included), with values_out, raw_out and raw_out->counts
 * untouched. */
int o3dmi_pointcloud_compute_metrics(
        const void* points1_dev, int64_t n1, const void* points2_dev,
        int64_t n2, int dtype, const int32_t* metrics, int n_metrics,
        const float* fscore_radius, int n_radii, float* values_out,
        int64_t values_capacity, o3dmi_pointcloud_metrics_raw_t* raw_out,
        o3dmi_stream_t stream);

/* The per-fragment step of slac::PreprocessPointClouds (t/pipelines/slac/
 * SLACOptimizer.cpp:47-57). voxel_size > 0: VoxelDownSample ->
 * RemoveStatisticalOutliers(20, 2.0) -> EstimateNormals (KNN, 30); otherwise
 * the filter, then EstimateNormals only when normals_dev is NULL.
 * apply_outlier_mask = 0 reproduces upstream, which computes the filter and
 * DROPS its result (the legacy method returns a tuple nobody reads);
 * 1 applies it. Outputs {n,3} each; *m_out rows are valid. Synchronises. */
int o3dmi_slac_preprocess_point_cloud(const void* points_dev,
                                      const void* normals_dev, int64_t n,
                                      int dtype, double voxel_size,
                                      int apply_outlier_mask,
                                      void* out_points_dev,
                                      void* out_normals_dev, int64_t* m_out,
                                      o3dmi_stream_t stream);

/* ---- PointCloud smoothing, boundary detection, normal orientation --------
 * (t/geometry/PointCloud.cpp:762-854, 986-1050, 1074-1203; kernels
 * t/geometry/kernel/PointCloudImpl.h:229-506, 1339-1753.) Float32 / Float64.
 * One wave serves a point and reduces the point's neighbour list while the
 * search still holds it in the wave's lanes; no {n, k} neighbour, distance or
 * angle table is allocated unless a call says so. A neighbourhood is therefore
 * at most one wave wide (upstream: no limit): a larger max_nn is
 * O3DMI_ERR_UNSUPPORTED. Common rules: n == 0 is O3DMI_OK with nothing
 * written; an output that overlaps an input, or a NaN / Inf coordinate
 * (upstream: undefined -- run RemoveNonFinitePoints first) is
 * O3DMI_ERR_INVALID_ARG. On an argument, limit or finiteness error, and when
 * the search index or a scratch buffer cannot be built, the outputs (*m_out
 * included) keep their contents: they are first written after all of that has
 * succeeded. Only a failed launch or copy after that point (O3DMI_ERR_HIP)
 * can leave them partly written.
 * Neighbour lists are ascending by (d2, index); sums run in list order in the
 * point dtype. All of the Smooth* / Compute* calls synchronise. */

/* PointCloud::SmoothLaplacian. Every pass: self-query KNN with
 * k = min(n, max_nn + 1); mean = sum of the neighbours whose index is not the
 * point's own (with duplicated points the point may sit anywhere in its list
 * or be absent); out = p + (T)lambda * (mean * (T)(1.0 / count) - p); count ==
 * 0 copies the point -- upstream's CPU arithmetic bit for bit.
 * use_fixed_neighborhoods != 0: one search into an int32 {n, k} table read by
 * every pass; else the index is rebuilt on the moved points before every pass
 * and no table exists. iterations == 0 or max_nn <= 0: out_points = points.
 * max_nn > 63: O3DMI_ERR_UNSUPPORTED. */
int o3dmi_pointcloud_smooth_laplacian(const void* points_dev, int64_t n,
                                      int dtype, int64_t iterations,
                                      double lambda, int max_nn,
                                      int use_fixed_neighborhoods,
                                      void* out_points_dev,
                                      o3dmi_stream_t stream);

/* PointCloud::SmoothTaubin: every iteration is a lambda pass, then a mu pass
 * (each with a fresh search unless the neighbourhoods are fixed). Otherwise
 * as o3dmi_pointcloud_smooth_laplacian. */
int o3dmi_pointcloud_smooth_taubin(const void* points_dev, int64_t n, int dtype,
                                   int64_t iterations, double lambda, double mu,
                                   int max_nn, int use_fixed_neighborhoods,
                                   void* out_points_dev,
                                   o3dmi_stream_t stream);

/* PointCloud::SmoothMLS: every point is projected onto the plane through the
 * weighted centroid of its neighbours, weights exp(-d2 / radius^2).
 * radius > 0 and max_nn > 0: hybrid search; radius <= 0: KNN with
 * k = min(n, max_nn) and every weight exp(-0); max_nn <= 0: every neighbour
 * within radius (this mode builds CSR lists); both <= 0: out = in. Fewer than
 * 3 neighbours, or a weight sum <= 0: the point stays. normals_dev (optional)
 * with out_normals_dev: the plane normal is returned, and a point with fewer
 * than 3 neighbours gets its incoming normal normalised; out_normals_dev
 * without normals_dev is O3DMI_ERR_INVALID_ARG. max_nn > 64 (hybrid, KNN):
 * O3DMI_ERR_UNSUPPORTED.
 * Parity: centroid and covariance are upstream's expressions in the point
 * dtype; the normal is this library's converged float64 Jacobi eigenvector
 * (see o3dmi_pointcloud_normals_from_covariances) with its sign rule (last
 * non-zero component positive), not upstream's closed form: a TOLERANCE. The
 * projected position does not depend on the sign; the normal's line agrees
 * with upstream wherever the two smallest eigenvalues are separated. */
int o3dmi_pointcloud_smooth_mls(const void* points_dev, const void* normals_dev,
                                int64_t n, int dtype, double radius, int max_nn,
                                void* out_points_dev, void* out_normals_dev,
                                o3dmi_stream_t stream);

/* PointCloud::SmoothBilateral (hybrid search): the normal is normalised in
 * the point dtype, weight = exp(-d2 / (2 sigma_s^2) - rd^2 / (2 sigma_r^2))
 * with rd = (p - q) . normal; out = weighted mean of the neighbours. A point
 * with count <= 1, a normal of norm <= 0 or a weight sum <= 0 stays.
 * sigma_s <= 0, sigma_r <= 0, radius <= 0, max_nn < 1 or normals_dev == NULL:
 * O3DMI_ERR_INVALID_ARG (the Python mirror estimates missing normals first,
 * as upstream does); max_nn > 64: O3DMI_ERR_UNSUPPORTED. */
int o3dmi_pointcloud_smooth_bilateral(const void* points_dev,
                                      const void* normals_dev, int64_t n,
                                      int dtype, double radius, int max_nn,
                                      double sigma_s, double sigma_r,
                                      void* out_points_dev,
                                      o3dmi_stream_t stream);

/* PointCloud::ComputeBoundaryPoints: hybrid search, then
 * o3dmi_pointcloud_boundary_from_neighbors' test (o3d_mi355x.h) on the list
 * in the wave. mask_out_dev: uint8 {n}, 1 = boundary; *m_out = number of
 * ones. radius <= 0, max_nn < 1 or normals_dev == NULL: O3DMI_ERR_INVALID_ARG;
 * max_nn > 64: O3DMI_ERR_UNSUPPORTED. */
int o3dmi_pointcloud_compute_boundary_points(const void* points_dev,
                                             const void* normals_dev,
                                             int64_t n, int dtype,
                                             double radius, int max_nn,
                                             double angle_threshold,
                                             uint8_t* mask_out_dev,
                                             int64_t* m_out,
                                             o3dmi_stream_t stream);

/* PointCloud::NormalizeNormals / OrientNormalsToAlignWithDirection /
 * OrientNormalsTowardsCameraLocation, in place on normals_dev {n,3},
 * statement by statement (zero normals take the direction, or the normalised
 * vector to the camera, or (0, 0, 1) for a point at the camera). direction3 /
 * camera3: host float64 {3}, converted to the point dtype as upstream's
 * reference.To(dtype), and handed to the kernel by value. All three are
 * queued on the stream and wait for nothing. */
int o3dmi_pointcloud_normalize_normals(void* normals_dev, int64_t n, int dtype,
                                       o3dmi_stream_t stream);
int o3dmi_pointcloud_orient_normals_to_align_with_direction(
        void* normals_dev, int64_t n, int dtype, const double* direction3,
        o3dmi_stream_t stream);
int o3dmi_pointcloud_orient_normals_towards_camera_location(
        const void* points_dev, void* normals_dev, int64_t n, int dtype,
        const double* camera3, o3dmi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* VoxelBlockGrid                                                            */
/* ------------------------------------------------------------------------ */
typedef struct o3dmi_vbg o3dmi_vbg_t;

/* VoxelBlockGrid(attr_names, attr_dtypes, attr_channels, voxel_size,
 * block_resolution, block_count) (VoxelBlockGrid.cpp:65-117). Attribute i has
 * dtype attr_dtypes[i] (O3DMI_F32 / O3DMI_U16 / ...) and attr_channels[i]
 * channels; "tsdf" and "weight" are required by Integrate/RayCast. */
int o3dmi_vbg_create(int n_attrs, const char* const* attr_names,
                     const int* attr_dtypes, const int* attr_channels,
                     float voxel_size, int64_t block_resolution,
                     int64_t block_count, o3dmi_stream_t stream,
                     o3dmi_vbg_t** out);
/* VoxelBlockGrid::To(device, copy = true) (through HashMap::To,
 * core/hashmap/HashMap.cpp:230-255): the grid on HIP device `device` (may be
 * its own: a deep copy) with the same attributes, voxel size, block keys and
 * voxel values; buffer indices are the new grid's own. The caller's current
 * device must be the source grid's; it is restored. The new grid is used with
 * `device` current and streams of that device. */
int o3dmi_vbg_to_device(o3dmi_vbg_t* g, int device, o3dmi_vbg_t** out);
int o3dmi_vbg_destroy(o3dmi_vbg_t* g);
o3dmi_hash_t* o3dmi_vbg_hashmap(o3dmi_vbg_t* g);
/* GetAttribute(name): device pointer of the {capacity,res,res,res,C} buffer
 * (NULL + warning semantics: returns NULL when absent). */
void* o3dmi_vbg_attribute(o3dmi_vbg_t* g, const char* name, int* dtype,
                          int* channels);

/* Block-ownership sharding of a grid across `world` GPUs (one process per
 * GPU): this grid only activates and integrates the blocks it owns
 * (o3dmi_hash_set_ownership); applies to GetUniqueBlockCoordinates and to the
 * frame(s) paths. Explicit block lists given to o3dmi_vbg_integrate_blocks
 * are taken as they are. */
int o3dmi_vbg_set_block_ownership(o3dmi_vbg_t* g, int rank, int world);

/* GetUniqueBlockCoordinates(depth, intrinsic, extrinsic, depth_scale,
 * depth_max, trunc_voxel_multiplier) (VoxelBlockGrid.cpp:212-245).
 * out_coords_dev must hold (rows/4)*(cols/4)*4 rows; *m_out = number of
 * unique blocks (synchronises; O3DMI_ERR_NO_BLOCKS when zero). */
int o3dmi_vbg_get_unique_block_coordinates(
        o3dmi_vbg_t* g, const void* depth_dev, int depth_dtype, int rows,
        int cols, const double* intrinsic, const double* extrinsic,
        float depth_scale, float depth_max, float trunc_voxel_multiplier,
        int32_t* out_coords_dev, int64_t* m_out, o3dmi_stream_t stream);

/* GetUniqueBlockCoordinates(pcd, trunc_voxel_multiplier)
 * (VoxelBlockGrid.cpp:246-267): the blocks within +-voxel_size *
 * trunc_voxel_multiplier of each of the n points {n, 3} Float32. The frustum
 * map is (re)created for n * 8 entries, upstream's estimate; out_coords_dev
 * holds out_capacity rows (n * 8 always suffices); *m_out = number of unique
 * blocks (synchronises). */
int o3dmi_vbg_get_unique_block_coordinates_pcd(
        o3dmi_vbg_t* g, const float* points_dev, int64_t n,
        float trunc_voxel_multiplier, int32_t* out_coords_dev,
        int64_t out_capacity, int64_t* m_out, o3dmi_stream_t stream);

/* GetVoxelIndices(buf_indices) / GetVoxelCoordinates(voxel_indices) /
 * GetVoxelCoordinatesAndFlattenedIndices(buf_indices) of this grid
 * (VoxelBlockGrid.cpp:130-211): the kernel-seam functions of the same names
 * (o3d_mi355x.h) with the grid's key buffer, block resolution and voxel size.
 * The forms without an argument upstream take GetActiveIndices():
 * o3dmi_hash_active_indices(o3dmi_vbg_hashmap(g), ...). get_voxel_coordinates
 * synchronises (a buffer index outside the map is O3DMI_ERR_INVALID_ARG, as
 * upstream's IndexGet throws); the other two are asynchronous. */
int o3dmi_vbg_get_voxel_indices(o3dmi_vbg_t* g, const int32_t* buf_indices_dev,
                                int64_t n_blocks, int64_t* voxel_indices_dev,
                                o3dmi_stream_t stream);
int o3dmi_vbg_get_voxel_coordinates(o3dmi_vbg_t* g,
                                    const int64_t* voxel_indices_dev,
                                    int64_t n_voxels, int64_t* voxel_coords_dev,
                                    o3dmi_stream_t stream);
int o3dmi_vbg_get_voxel_coordinates_and_flattened_indices(
        o3dmi_vbg_t* g, const int32_t* buf_indices_dev, int64_t n_blocks,
        float* voxel_coords_dev, int64_t* flattened_indices_dev,
        o3dmi_stream_t stream);

/* Integrate(block_coords, depth, color, depth_intrinsic, color_intrinsic,
 * extrinsic, depth_scale, depth_max, trunc_voxel_multiplier)
 * (VoxelBlockGrid.cpp:292-326): Activate + Find + per-voxel update. May
 * Reserve (rehash) when size + m exceeds the capacity, as the reference. */
int o3dmi_vbg_integrate_blocks(o3dmi_vbg_t* g, const int32_t* block_coords_dev,
                               int64_t m, const void* depth_dev,
                               int depth_rows, int depth_cols,
                               const void* color_dev, int color_rows,
                               int color_cols, int input_dtype,
                               const double* depth_intrinsic,
                               const double* color_intrinsic,
                               const double* extrinsic, float depth_scale,
                               float depth_max, float trunc_voxel_multiplier,
                               o3dmi_stream_t stream);

/* Frame-stream fast path: GetUniqueBlockCoordinates + Integrate of one frame
 * with every count kept on the device (no host round trip unless the hash map
 * must grow). Results are identical to the two calls above. */
int o3dmi_vbg_integrate_frame(o3dmi_vbg_t* g, const void* depth_dev,
                              int depth_rows, int depth_cols,
                              const void* color_dev, int color_rows,
                              int color_cols, int input_dtype,
                              const double* depth_intrinsic,
                              const double* color_intrinsic,
                              const double* extrinsic, float depth_scale,
                              float depth_max, float trunc_voxel_multiplier,
                              o3dmi_stream_t stream);

/* The same for a batch of frames sharing intrinsics and image sizes:
 * depth_devs / color_devs are host arrays of n_frames device pointers,
 * extrinsics is n_frames x 16 host doubles. Frames are integrated strictly in
 * order (frame f sees the grid left by frame f-1), so the result is identical
 * to n_frames calls of o3dmi_vbg_integrate_frame.
 * frames_per_launch (1..16, <= 0 = 8): consecutive frames are grouped; one
 * launch applies the frames of a group, in order, to each touched block while
 * its voxel state stays in registers (state is read / written once per group
 * instead of once per frame; a block only receives the frames that touched
 * it), and the same launch already carries the touch / prepare work of the
 * next group. All work is issued on `stream`. */
int o3dmi_vbg_integrate_frames(o3dmi_vbg_t* g, int n_frames,
                               const void* const* depth_devs, int depth_rows,
                               int depth_cols, const void* const* color_devs,
                               int color_rows, int color_cols, int input_dtype,
                               const double* depth_intrinsic,
                               const double* color_intrinsic,
                               const double* extrinsics, float depth_scale,
                               float depth_max, float trunc_voxel_multiplier,
                               int frames_per_launch, o3dmi_stream_t stream);

/* ---- block-ownership sharding with a SLICED block touch (scheme
 * A as specified: "every GPU runs DepthTouch on a 1/G pixel slice, all-gathers
 * the candidate keys, keeps hash(key) mod G == rank"; the loop being sliced is
 * DepthTouchCPU, VoxelBlockGridCPU.cpp:117-201).
 *
 * With o3dmi_vbg_set_block_ownership(rank, world > 1) AND a communicator on the
 * calling thread (o3dmi_set_comm), o3dmi_vbg_integrate_frames takes this path
 * by itself whenever depth and colour images share size and intrinsics:
 * frames go in chunks of 16 x frames_per_launch (<= 256); on a side stream
 * rank r touches only its band of ray tiles, the candidate {block key, one bit
 * per frame of the chunk} records of all ranks are all-gathered (ONE
 * collective per chunk, fixed-size segments) and the keys a rank owns are
 * activated; on the caller's stream ONE launch per chunk applies all its
 * frames, in order, to the owned blocks' register-resident voxels, straight
 * from the raw depth / colour images (no per-pixel prepare pass). Each rank's
 * grid is bit-identical to what the replicated touch produces: the blocks it
 * owns of the single-GPU grid.
 *
 * In this mode o3dmi_vbg_integrate_frames is
 *  - COLLECTIVE: every rank calls it with the same frames. A rank that has to
 *    leave it with an error of its own first delivers the all-gather the
 *    others will wait in next with an empty segment flagged "abort"; every
 *    rank then returns O3DMI_ERR_PEER at the same chunk (nobody is left in a
 *    collective), the failing rank its own status, with its map left usable;
 *  - NOT purely stream-ordered on the host: it waits for the previous call's
 *    side-stream work, uploads the call's frame tables synchronously and
 *    follows each chunk's status word, so back-to-back calls serialise on the
 *    host (hand over long batches: bench.py passes 8000 frames per call).
 * The functions below expose the two halves for callers with their own
 * exchange, for tests and for bench.py --emulate-world. */

/* Frames per chunk for a frames_per_launch setting (16 launches). */
int o3dmi_vbg_slice_chunk_frames(int frames_per_launch);
/* Wire format sizes: a rank's segment of a chunk holds `records` 48-byte
 * records {key, 256 frame bits} + a 128-byte header. Default 4096 records and
 * chunk tables of 8192 slots; with a communicator both double by themselves
 * when a chunk does not fit (every rank reads the same headers and takes the
 * same decision), with caller-provided segments an overflow is
 * O3DMI_ERR_CAPACITY. */
int o3dmi_vbg_set_slice_capacity(o3dmi_vbg_t* g, int records,
                                 int table_slots);
int64_t o3dmi_vbg_slice_segment_bytes(const o3dmi_vbg_t* g);
/* Rank slice_rank's band of the ray tiles of up to one chunk of frames ->
 * its wire segment (device buffer of o3dmi_vbg_slice_segment_bytes bytes).
 * The grid only lends its scratch tables; its map is not touched. */
int o3dmi_vbg_touch_slice(o3dmi_vbg_t* g, int n_frames,
                          const void* const* depth_devs, int depth_rows,
                          int depth_cols, const double* depth_intrinsic,
                          const double* extrinsics, float depth_scale,
                          float depth_max, float trunc_voxel_multiplier,
                          int frames_per_launch, int slice_rank,
                          int slice_world, void* segment_out_dev,
                          o3dmi_stream_t stream);
/* o3dmi_vbg_integrate_frames through the sliced path. gathered_devs: for each
 * chunk of the call a device buffer with the `world` wire segments of all
 * ranks (rank-major; the own segment is recomputed and replaced), or NULL: the
 * all-gather runs over the calling thread's communicator. */
int o3dmi_vbg_integrate_frames_sliced(
        o3dmi_vbg_t* g, int n_frames, const void* const* depth_devs,
        int depth_rows, int depth_cols, const void* const* color_devs,
        int color_rows, int color_cols, int input_dtype,
        const double* depth_intrinsic, const double* color_intrinsic,
        const double* extrinsics, float depth_scale, float depth_max,
        float trunc_voxel_multiplier, int frames_per_launch,
        const void* const* gathered_devs, o3dmi_stream_t stream);
/* Chunks integrated through the sliced path, chunks applied a second time
 * (Reserve of the block map, or grown segments), current sizes. */
int o3dmi_vbg_sliced_stats(const o3dmi_vbg_t* g, int64_t* chunks,
                           int64_t* reapplied, int* capacity,
                           int* table_slots);

/* Measurement hook for bench.py: while profiling is on, every stride-th
 * launch that carries integrate work (o3dmi_vbg_integrate_frame(s)) is
 * bracketed with HIP events on the stream it is launched on (stride 0 = none).
 * o3dmi_vbg_profile_end synchronises and returns, over the bracketed launches:
 * their summed duration (ms), their number, the number of block-frames they
 * integrated (sum over touched blocks of the frames applied to each -- the
 * roofline's unit) and the number of frames they carried. */
int o3dmi_vbg_profile_begin(o3dmi_vbg_t* g, int max_launches, int stride);
int o3dmi_vbg_profile_end(o3dmi_vbg_t* g, o3dmi_stream_t stream,
                          double* integrate_ms, int64_t* launches,
                          int64_t* block_frames, int64_t* frames);
/* Sum over the launches bracketed by the last profile_begin / profile_end pair
 * of the DISTINCT blocks each of them worked on (the length of the group's
 * block list): what the voxel state costs in memory traffic when the frames of
 * a group are applied to register-resident blocks -- once in, once out per
 * launch, however many frames the group has. */
int64_t o3dmi_vbg_profile_distinct_blocks(const o3dmi_vbg_t* g);
/* Diagnostics: which of the frame stream's exact short division forms are in
 * use for the truncation distance voxel_size * trunc_voxel_multiplier on the
 * current device -- 0 = IEEE divisions only (the on-device proof is still
 * running, failed, or O3DMI_EXACT_DIV is set), 1 = sdf / trunc and 1 / (w + 1),
 * 2 / 3 = also 1 / z with one / two Newton steps. The proof runs asynchronously
 * (started by o3dmi_vbg_create for multiplier 8 and by the first integration
 * with any other); launches take the IEEE forms until it has finished, the
 * results are the same either way. wait != 0 blocks until it has. */
int o3dmi_vbg_division_forms(float voxel_size, float trunc_voxel_multiplier,
                             int wait);
/* Diagnostics: how many frame-stream launches of this process ran their
 * integrate role in a given form -- 0 = IEEE divisions, 1 = the short
 * divisions, 2 = the short divisions without the per-frame range test of the
 * projection's 1 / z (every pose of the group has |e[2][3]| >= 2^-36 and a
 * third row bounded by 2^59). Results are the same in every form. Returns -1
 * for any other `form`. */
int64_t o3dmi_vbg_step_form_launches(int form);
/* Diagnostics: the frame stream's block touch collects the block keys of one
 * 16 x 16 tile of rays over all the frames of a launch and sends each distinct
 * key through the hash once. This is the number of distinct keys it holds at
 * most: before a frame that could take it further (a frame adds up to 1024)
 * the keys collected so far are sent and the set starts empty. Results do not
 * depend on it. */
int32_t o3dmi_vbg_front_tile_key_limit(void);
/* The same measurement per bracketed launch (any output may be null): HIP-event
 * duration (ms), block-frames, distinct blocks, and the map size (blocks
 * active) the launch's integrate role saw when it started. Returns the number
 * of launches bracketed; at most `capacity` entries are written. */
int64_t o3dmi_vbg_profile_launches(const o3dmi_vbg_t* g, int64_t capacity,
                                   float* ms, int32_t* block_frames,
                                   int32_t* distinct_blocks,
                                   int32_t* map_size);

/* RayCast(block_coords, intrinsic, extrinsic, width, height, attrs, ...)
 * (VoxelBlockGrid.cpp:328-402). Output pointers follow o3dmi_vbg_raycast;
 * range_map_dev {h/down, w/down, 2} is also an output ("range"). */
int o3dmi_vbg_ray_cast(o3dmi_vbg_t* g, const int32_t* block_coords_dev,
                       int64_t m, const double* intrinsic,
                       const double* extrinsic, int width, int height,
                       float* range_map_dev, float* out_depth,
                       float* out_vertex, float* out_color, float* out_normal,
                       int64_t* out_index, uint8_t* out_mask, float* out_ratio,
                       float* out_ratio_dx, float* out_ratio_dy,
                       float* out_ratio_dz, float depth_scale, float depth_min,
                       float depth_max, float weight_threshold,
                       float trunc_voxel_multiplier, int range_map_down_factor,
                       o3dmi_stream_t stream);

/* RayCast of a REPLICATED grid sharded by pixel rows over the ranks of the
 * calling thread's communicator (o3dmi_set_comm; SURVEY 8(e), RayCast row --
 * the tracking frame of a multi-GPU loop, whose model every rank holds): rank
 * r renders rows [r B, (r + 1) B) (B = whole 8-row tiles, ceil(tiles / world)
 * of them) of depth / vertex / colour / normal, one all-gather per requested
 * map delivers every rank's band, and every rank ends with the maps
 * o3dmi_vbg_ray_cast produces, bit for bit. COLLECTIVE: every rank calls it
 * with the same arguments. What can fail on one rank alone (its arguments,
 * scratch memory, the band's launch) happens before the first all-gather and
 * the ranks agree on its status (one 4-byte all-gather, one host wait): the
 * failing rank returns its error, every other rank O3DMI_ERR_PEER, and no
 * rank waits in an exchange. The call blocks the host until the maps are
 * complete. Without a communicator (or with one rank) it is
 * o3dmi_vbg_ray_cast. */
int o3dmi_vbg_ray_cast_sharded(
        o3dmi_vbg_t* g, const int32_t* block_coords_dev, int64_t m,
        const double* intrinsic, const double* extrinsic, int width, int height,
        float* range_map_dev, float* out_depth, float* out_vertex,
        float* out_color, float* out_normal, float depth_scale, float depth_min,
        float depth_max, float weight_threshold, float trunc_voxel_multiplier,
        int range_map_down_factor, o3dmi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* RGB-D odometry (t/pipelines/odometry/RGBDOdometry.h)                      */
/* ------------------------------------------------------------------------ */
/* OdometryConvergenceCriteria (RGBDOdometry.h:30-57): defaults relative_rmse
 * 1e-6, relative_fitness 1e-6. */
typedef struct {
    int max_iteration;
    double relative_rmse;
    double relative_fitness;
} o3dmi_odometry_criteria_t;

/* OdometryResult (RGBDOdometry.h:59-86) + the number of iterations run. */
typedef struct {
    double transformation[16]; /* 4x4 float64, row-major, host */
    double inlier_rmse;
    double fitness;
    int num_iterations;
} o3dmi_odometry_result_t;

/* RGBDOdometryMultiScale(source, target, intrinsics, init_source_to_target,
 * depth_scale, depth_max, criteria_list, method, params)
 * (RGBDOdometry.cpp:56-108; drivers :110-380). depth {rows,cols} U16 or F32;
 * colour {rows,cols,3} U8 or F32, may be NULL for point-to-plane; source and
 * target dtypes are independent (slam::Model tracks a U16 / U8 input frame
 * against the F32 ray-cast frame, slam/Model.cpp:72-92); criteria are
 * ordered coarse to fine, one per pyramid level; OdometryLossParams defaults
 * (RGBDOdometry.h:88-120): depth_outlier_trunc 0.07, depth_huber_delta 0.05,
 * intensity_huber_delta 0.1. init NULL = identity.
 * Status: O3DMI_ERR_NO_INLIERS ("Invalid inlier_count value ..., must be > 0."),
 * O3DMI_ERR_SINGULAR -- the reference's two exceptions on this path. */
int o3dmi_rgbd_odometry_multiscale(
        const void* source_depth_dev, const void* source_color_dev,
        const void* target_depth_dev, const void* target_color_dev,
        int source_depth_dtype, int source_color_dtype, int target_depth_dtype,
        int target_color_dtype, int rows, int cols, const double* intrinsics,
        const double* init_source_to_target, float depth_scale,
        float depth_max, int n_levels,
        const o3dmi_odometry_criteria_t* criteria, int method,
        float depth_outlier_trunc, float depth_huber_delta,
        float intensity_huber_delta, o3dmi_odometry_result_t* result,
        o3dmi_stream_t stream);

/* ComputeOdometryInformationMatrix(source_depth, target_depth, intrinsic,
 * source_to_target, dist_thr, depth_scale, depth_max)
 * (RGBDOdometry.cpp:488-513): 6x6 float64 on the host. */
int o3dmi_rgbd_odometry_information_matrix(
        const void* source_depth_dev, const void* target_depth_dev,
        int depth_dtype, int rows, int cols, const double* intrinsics,
        const double* source_to_target, float dist_thr, float depth_scale,
        float depth_max, double* information_host, o3dmi_stream_t stream);

/* Extension: loads the kernels of the tracking / integration path now. HIP
 * loads a translation unit's device code at the first launch of one of its
 * kernels (1.5-2.8 ms each for the large ones); an application that cares about
 * the latency of its FIRST frame calls this once at start-up. */
int o3dmi_preload(void);

/* Extension (no counterpart in the reference's API): the block coordinates
 * the most recent o3dmi_vbg_integrate_frame (or the last frame of an
 * o3dmi_vbg_integrate_frames call with frames_per_launch = 1) touched -- the
 * set GetUniqueBlockCoordinates returns for that frame's (depth, intrinsic,
 * extrinsic), in the order the touch found them -- copied on the stream to
 * out_coords_dev {capacity,3}, their number to *out_count_dev (device int32):
 * no second block touch and no host round trip for the ray cast that follows
 * an integration (slam::Model uses it the same way). Issue it right behind
 * the integrate call; pass both to o3dmi_vbg_ray_cast_dev. */
int o3dmi_vbg_last_frame_block_coordinates(o3dmi_vbg_t* g,
                                           int32_t* out_coords_dev,
                                           int64_t capacity,
                                           int32_t* out_count_dev,
                                           o3dmi_stream_t stream);

/* RayCast with the number of block coordinates resident on the device
 * (*m_dev <= max_m; m_dev NULL = max_m): no host round trip between the
 * integration that produced the block list and the ray cast that uses it.
 * block_coords_dev NULL: the blocks the most recent frame-stream integration
 * touched (what o3dmi_vbg_last_frame_block_coordinates would copy out), read
 * from the grid's own list -- no export launch; max_m / m_dev are ignored.
 * range_map_dev NULL: the range map is the grid's own scratch, as in the
 * reference (VoxelBlockGrid.cpp:357-360 allocates it inside RayCast); with
 * the default down factor of 8 the ray cast that consumes it leaves it clean
 * for the next call, which then needs no clearing launch. */
int o3dmi_vbg_ray_cast_dev(o3dmi_vbg_t* g, const int32_t* block_coords_dev,
                           int64_t max_m, const int32_t* m_dev,
                           const double* intrinsic, const double* extrinsic,
                           int width, int height, float* range_map_dev,
                           float* out_depth, float* out_vertex,
                           float* out_color, float* out_normal,
                           int64_t* out_index, uint8_t* out_mask,
                           float* out_ratio, float* out_ratio_dx,
                           float* out_ratio_dy, float* out_ratio_dz,
                           float depth_scale, float depth_min, float depth_max,
                           float weight_threshold,
                           float trunc_voxel_multiplier,
                           int range_map_down_factor, o3dmi_stream_t stream);

/* ExtractPointCloud(weight_threshold, estimated_point_number)
 * (VoxelBlockGrid.cpp:404-434). capacity < 0: only counts (the reference's
 * 2-pass estimation) -> *total_out; otherwise writes up to `capacity` points:
 * points / normals {capacity,3} float32, colors {capacity,3} float32 in [0,1]
 * when the grid has a "color" attribute (colors_dev may be NULL).
 * *total_out = number of surface points found (synchronises). Order: active
 * blocks by ascending buffer index, then voxel, then axis. */
int o3dmi_vbg_extract_point_cloud(o3dmi_vbg_t* g, float weight_threshold,
                                  int64_t capacity, float* points_dev,
                                  float* normals_dev, float* colors_dev,
                                  int64_t* total_out, o3dmi_stream_t stream);

/* ExtractTriangleMesh (VoxelBlockGrid.cpp:436-471): marching cubes over
 * every active block. vertex_capacity < 0 counts only (the reference's 2-pass
 * mode); otherwise vertices / normals / colours hold vertex_capacity x 3
 * floats and triangles 3 x vertex_capacity x 3 int32, and O3DMI_ERR_CAPACITY
 * (nothing written) reports too small a capacity or more than INT32_MAX
 * vertices. colors_dev may be NULL; colours are written when the grid has a
 * "color" attribute. *n_vertices_out / *n_triangles_out = the mesh's counts
 * (synchronises). Order: active blocks by ascending buffer index, then voxel,
 * then axis (vertices) or table order (triangles). */
int o3dmi_vbg_extract_triangle_mesh(o3dmi_vbg_t* g, float weight_threshold,
                                    int64_t vertex_capacity,
                                    float* vertices_dev, float* normals_dev,
                                    float* colors_dev, int32_t* triangles_dev,
                                    int64_t* n_vertices_out,
                                    int64_t* n_triangles_out,
                                    o3dmi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* slam::Model (t/pipelines/slam/Model.h:24-137, Model.cpp:23-118)           */
/* ------------------------------------------------------------------------ */
typedef struct o3dmi_slam_model o3dmi_slam_model_t;

/* Model(voxel_size, block_resolution = 16, block_count = 1000, T_init = I):
 * grid attributes ("tsdf" F32 x1, "weight" U16 x1, "color" U16 x3)
 * (Model.cpp:23-38). T_init host 4x4 float64 or NULL. */
int o3dmi_slam_model_create(float voxel_size, int block_resolution,
                            int64_t block_count, const double* T_init,
                            o3dmi_stream_t stream, o3dmi_slam_model_t** out);
int o3dmi_slam_model_destroy(o3dmi_slam_model_t* m);
o3dmi_vbg_t* o3dmi_slam_model_voxel_grid(o3dmi_slam_model_t* m);
/* GetCurrentFramePose / UpdateFramePose (Model.h:45-54); frame ids that do
 * not advance by one only warn in the reference, here they are accepted. */
int o3dmi_slam_model_get_current_frame_pose(const o3dmi_slam_model_t* m,
                                            double* T_frame_to_world);
int o3dmi_slam_model_update_frame_pose(o3dmi_slam_model_t* m, int frame_id,
                                       const double* T_frame_to_world);
int o3dmi_slam_model_frame_id(const o3dmi_slam_model_t* m);
/* SynthesizeModelFrame (Model.cpp:40-68): ray-casts the frustum blocks of the
 * last Integrate at the current pose into depth {h,w,1} F32 (raw units) and,
 * if color_out_dev != NULL, colour {h,w,3} F32 in [0,1]. weight_threshold < 0
 * = min(frame_id, 3). */
int o3dmi_slam_model_synthesize_model_frame(
        o3dmi_slam_model_t* m, const double* intrinsics, int width, int height,
        float depth_scale, float depth_min, float depth_max,
        float trunc_voxel_multiplier, float weight_threshold,
        float* depth_out_dev, float* color_out_dev, o3dmi_stream_t stream);
/* TrackFrameToModel (Model.cpp:70-92): RGBDOdometryMultiScale(input frame,
 * ray-cast frame, intrinsics, identity, depth_scale, depth_max, criteria,
 * method, OdometryLossParams(depth_diff)). Defaults: depth_diff 0.07, method
 * point-to-plane, criteria {6, 3, 1}. raycast_* are Float32. */
int o3dmi_slam_model_track_frame_to_model(
        o3dmi_slam_model_t* m, const void* input_depth_dev,
        int input_depth_dtype, const void* input_color_dev,
        int input_color_dtype, const float* raycast_depth_dev,
        const float* raycast_color_dev, int rows, int cols,
        const double* intrinsics, float depth_scale, float depth_max,
        float depth_diff, int method, int n_levels,
        const o3dmi_odometry_criteria_t* criteria,
        o3dmi_odometry_result_t* result, o3dmi_stream_t stream);
/* Integrate (Model.cpp:94-108): GetUniqueBlockCoordinates + Integrate at
 * InverseTransformation(current pose); remembers the frustum blocks. Colour
 * may be NULL (depth-only integration). */
int o3dmi_slam_model_integrate(o3dmi_slam_model_t* m, const void* depth_dev,
                               int depth_dtype, const void* color_dev,
                               int rows, int cols, const double* intrinsics,
                               float depth_scale, float depth_max,
                               float trunc_voxel_multiplier,
                               o3dmi_stream_t stream);
/* Number of frustum blocks of the last Integrate (reads the device-resident
 * count back: synchronises) and their keys (device, {n,3} int32; valid until
 * the next Integrate). */
int64_t o3dmi_slam_model_frustum_block_count(const o3dmi_slam_model_t* m);
const int32_t* o3dmi_slam_model_frustum_block_coords(const o3dmi_slam_model_t* m);
/* ExtractPointCloud (Model.cpp:110-113). */
int o3dmi_slam_model_extract_point_cloud(o3dmi_slam_model_t* m,
                                         float weight_threshold,
                                         int64_t capacity, float* points_dev,
                                         float* normals_dev, float* colors_dev,
                                         int64_t* total_out,
                                         o3dmi_stream_t stream);

/* ExtractTriangleMesh (Model.cpp:113-116). */
int o3dmi_slam_model_extract_triangle_mesh(
        o3dmi_slam_model_t* m, float weight_threshold, int64_t vertex_capacity,
        float* vertices_dev, float* normals_dev, float* colors_dev,
        int32_t* triangles_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* NPZ interchange (t/io/NumpyIO.cpp) and VoxelBlockGrid::Save / Load        */
/* ------------------------------------------------------------------------ */
/* An in-memory set of named host arrays. o3dmi_npz_write = t::io::WriteNpz
 * (NumpyIO.cpp:759-789; NPY 1.0 headers and stored zip entries formatted as
 * the reference does, ZIP64 where its 32-bit fields would wrap);
 * o3dmi_npz_read = t::io::ReadNpz (:675-757; also reads numpy's own savez /
 * savez_compressed output). Little-endian C-order arrays only. */
typedef struct o3dmi_npz o3dmi_npz_t;
int o3dmi_npz_create(o3dmi_npz_t** out);
int o3dmi_npz_destroy(o3dmi_npz_t* z);
/* Copies `data_host`; an existing entry of the same name is replaced. */
int o3dmi_npz_add(o3dmi_npz_t* z, const char* name, int dtype, int ndim,
                  const int64_t* shape, const void* data_host);
int o3dmi_npz_count(const o3dmi_npz_t* z);
const char* o3dmi_npz_name(const o3dmi_npz_t* z, int i);
/* shape8 must hold 8 entries; *data_host points into the set. */
int o3dmi_npz_get(const o3dmi_npz_t* z, const char* name, int* dtype, int* ndim,
                  int64_t* shape8, const void** data_host);
int o3dmi_npz_write(const o3dmi_npz_t* z, const char* file_name);
int o3dmi_npz_read(const char* file_name, o3dmi_npz_t** out);

/* VoxelBlockGrid::Save(file_name) (VoxelBlockGrid.cpp:474-524): entries
 * "voxel_size" {1} f32, "block_resolution" {1} i64, a 0-d u8 placeholder named
 * after the device ("HIP:0" -- stock Open3D ignores unknown prefixes and loads
 * on CPU:0), "attr_name_<name>" {1} i32 = value index, "key" {n,3} i32 and
 * "value_%03d" {n,res,res,res,C} of the ACTIVE blocks (ascending buffer
 * index). ".npz" is appended when missing, as the reference. */
int o3dmi_vbg_save(o3dmi_vbg_t* g, const char* file_name,
                   o3dmi_stream_t stream);
/* VoxelBlockGrid::Load(file_name) (VoxelBlockGrid.cpp:538-596): capacity =
 * number of stored keys; keys and value rows are inserted into a new grid on
 * the current device. */
int o3dmi_vbg_load(const char* file_name, o3dmi_stream_t stream,
                   o3dmi_vbg_t** out);
/* Frame-sharded multi-GPU integration, the merge step (SURVEY section 8e
 * scheme B; no counterpart in the reference, which is single-device). Each
 * rank integrates its own frames into a private grid; the grids are then
 * combined block by block.
 * o3dmi_vbg_export_blocks writes the ACTIVE blocks in ascending buffer index
 * (the order of Save): keys {n,3} int32 and, per attribute i, the value rows
 * {n,res,res,res,C_i} into values_dev[i] (device, caller-allocated for
 * `capacity` blocks). keys_dev == NULL only counts. *n_out = number of active
 * blocks (synchronises); O3DMI_ERR_CAPACITY if it exceeds `capacity`.
 * o3dmi_vbg_merge_blocks folds n foreign blocks of the same attribute layout
 * into `g`: missing blocks are activated (HashMap::Activate's capacity policy),
 * then per voxel, with w1 / w2 the weights of `g` / of the foreign block:
 *   w2 == 0: unchanged;  w1 == 0: the foreign voxel is copied;
 *   else inv = 1 / (w1 + w2), tsdf = (w1 tsdf1 + w2 tsdf2) inv,
 *        colour likewise per channel, weight = w1 + w2 (uint16 grids:
 *        saturating at 65535)
 * in float32 with Integrate's store conversions -- the running mean Integrate
 * itself computes (VoxelBlockGridImpl.h:258-300), so folding a one-frame grid
 * in is bit-identical to integrating that frame. Precondition (not checked):
 * the n keys are pairwise distinct -- two rows with one key would race on
 * the same voxels. */
int o3dmi_vbg_export_blocks(o3dmi_vbg_t* g, int64_t capacity,
                            int32_t* keys_dev, void* const* values_dev,
                            int64_t* n_out, o3dmi_stream_t stream);
int o3dmi_vbg_merge_blocks(o3dmi_vbg_t* g, const int32_t* keys_dev,
                           const void* const* values_dev, int64_t n,
                           o3dmi_stream_t stream);

/* The payload exchange of the frame-sharded scheme,
 * owner-partitioned: every active block of this rank's private grid travels
 * to the rank that OWNS it (the fixed key hash of the block-ownership scheme,
 * o3dmi_hash_set_ownership) with one all-to-all per tensor -- keys, then each
 * attribute's rows -- and the owner folds the partial blocks of all ranks in
 * (o3dmi_vbg_merge_blocks, own partial first, then ascending source rank).
 * Blocks sent away are erased and their value rows zeroed, so afterwards the
 * ranks hold DISJOINT grids whose union is the model of the whole stream: the
 * same layout block-ownership sharding produces. A rank moves (world - 1) /
 * world of its blocks once (an all-gather of everything would move world x
 * as much to every rank). Collective: every rank of `comm` must call it. A
 * rank that cannot list its blocks, or cannot reserve room for the arriving
 * ones, says so in the count exchange / in a status all-gather before the
 * first payload all-to-all: it returns its own error, the others
 * O3DMI_ERR_PEER, and every grid still holds what it held (same for the
 * counting and export stages of o3dmi_vbg_allgather_owned_blocks). Room for
 * the arriving blocks is reserved BEFORE anything is erased; after
 * o3dmi_vbg_allgather_owned_blocks a further merge is refused (the replicated
 * blocks would be counted again).
 * o3dmi_vbg_allgather_owned_blocks then replicates the finished blocks on
 * every rank (when each GPU is to ray-cast the whole model). */
int o3dmi_vbg_merge_frame_sharded(o3dmi_vbg_t* g, o3dmi_comm_t* comm,
                                  o3dmi_stream_t stream);
int o3dmi_vbg_allgather_owned_blocks(o3dmi_vbg_t* g, o3dmi_comm_t* comm,
                                     o3dmi_stream_t stream);

/* Introspection of a grid (needed after Load): attribute count / i-th name,
 * voxel size, block resolution. */
int o3dmi_vbg_attribute_count(const o3dmi_vbg_t* g);
const char* o3dmi_vbg_attribute_name(const o3dmi_vbg_t* g, int i);
float o3dmi_vbg_voxel_size(const o3dmi_vbg_t* g);
int64_t o3dmi_vbg_block_resolution(const o3dmi_vbg_t* g);

/* ---- TriangleMesh operators --------------------------------------------------
 * (t/geometry/kernel/TriangleMeshImpl.h, TriangleMeshCPU.cpp:22-56; the host
 * loops of t/geometry/TriangleMesh.cpp:1221-1452 and 1826-1864; legacy
 * geometry/TriangleMesh.cpp:1459-1528.) A mesh is positions {v,3} in `dtype`
 * (O3DMI_F32 / O3DMI_F64) and triangles {m,3} in `index_dtype` (O3DMI_I32 /
 * O3DMI_I64, narrowed on load). v < 2^31, m <= 2^29. Common rules:
 *  - EVERY triangle index is range-checked on the device before anything is
 *    written: an index outside [0, v) is O3DMI_ERR_INVALID_ARG with every
 *    output untouched (upstream reads out of bounds).
 *  - m == 0 or v == 0 is legal wherever upstream returns an empty or zero
 *    result.
 *  - Arithmetic is in the position dtype without contraction.
 *  - A NULL pointer where one is needed, a dtype outside the two, v or m out
 *    of range: O3DMI_ERR_INVALID_ARG before anything is allocated.
 * All synchronise. */

/* ComputeTriangleNormalsCPU / CUDA: normals_out {m,3} = cross_3x1(p2 - p1,
 * p3 - p1) (core/linalg/kernel/Matrix.h:63-73), NOT normalised: normalising
 * is a second call, as upstream. */
int o3dmi_trianglemesh_compute_triangle_normals(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* normals_out_dev, o3dmi_stream_t stream);

/* ComputeTriangleAreasCPU / CUDA: areas_out {m} = 0.5 * sqrt((t0 t0 + t1 t1) +
 * t2 t2) of the same cross product. */
int o3dmi_trianglemesh_compute_triangle_areas(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* areas_out_dev, o3dmi_stream_t stream);

/* TriangleMesh::GetSurfaceArea: *area_out = the float64 sum of those areas in
 * the fixed tree of o3dmi_pointcloud_compute_metrics (runs of 512 in index
 * order, the run sums likewise). Upstream: Sum({0}) in the dtype, order
 * unspecified. m == 0 gives 0. */
int o3dmi_trianglemesh_surface_area(const void* positions_dev, int64_t v,
                                    int dtype, const void* triangles_dev,
                                    int64_t m, int index_dtype,
                                    double* area_out, o3dmi_stream_t stream);

/* NormalizeNormalsCPU / CUDA (TriangleMeshImpl.h:40-69), in place on
 * normals_dev {n,3}: norm = sqrt((x x + y y) + z z); the row is divided when
 * norm > 0. THE MESH RULE, NOT THE POINTCLOUD ONE: a row whose x is NaN is
 * left exactly as it is (upstream assigns (0, 0, 1) to locals it never
 * stores). */
int o3dmi_trianglemesh_normalize_normals(void* normals_dev, int64_t n,
                                         int dtype, o3dmi_stream_t stream);

/* ComputeVertexNormalsCPU bit for bit: component c of vertex u of
 * vertex_normals_out {v,3} is ((0 + n_a[c]) + n_b[c]) + ... in `dtype` over
 * the corners 3 t + k that name u, in ascending corner order (a triangle that
 * lists a vertex twice adds twice; an unreferenced vertex is +0). No float
 * atomics: the corners are stable-sorted by vertex and every vertex's list is
 * walked in order. The same bits on every run. */
int o3dmi_trianglemesh_compute_vertex_normals(
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* triangle_normals_dev, int dtype, int64_t v,
        void* vertex_normals_out_dev, o3dmi_stream_t stream);

/* TriangleMesh::ComputeVertexNormals(normalized): triangle normals (not
 * normalised), the sum above, then o3dmi_trianglemesh_normalize_normals when
 * `normalized`. triangle_normals_out_dev {m,3} is optional (NULL: pooled
 * scratch). */
int o3dmi_trianglemesh_vertex_normals(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* triangle_normals_out_dev, void* vertex_normals_out_dev,
        int normalized, o3dmi_stream_t stream);

/* TriangleMesh::GetNonManifoldEdges. Edge slot 3 t + k is the ordered pair
 * (lo, hi) of (v_k, v_(k+1)%3); an edge's multiplicity is its number of slots
 * (upstream's GetEdgeToTrianglesMap: a triangle (6,6,7) gives (6,6) once and
 * (6,7) twice). Emits the edges of multiplicity > 2 (allow_boundary_edges) or
 * != 2 into edges_out_dev {capacity,2} in the index dtype, in ASCENDING
 * (lo, hi) ORDER (upstream: unordered_map iteration order), and their number
 * into *n_edges_out. capacity < 0 only counts; 0 <= capacity < the number is
 * O3DMI_ERR_CAPACITY with nothing written (*n_edges_out is still set). */
int o3dmi_trianglemesh_get_non_manifold_edges(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int allow_boundary_edges, void* edges_out_dev, int64_t capacity,
        int64_t* n_edges_out, o3dmi_stream_t stream);

/* Legacy TriangleMesh::ClusterConnectedTriangles. Two triangles are adjacent
 * when they share an edge of the table above (a shared vertex alone does not
 * connect them); clusters are the connected components, NUMBERED BY THEIR
 * LOWEST TRIANGLE INDEX, which is the order in which the legacy loop meets
 * their seeds: labels_out_dev int32 {m} equals upstream's.
 * cluster_n_triangles_out_dev int64 {capacity} and cluster_area_out_dev
 * float64 {capacity} are optional (NULL). *n_clusters_out is always set;
 * capacity < 0 only counts and 0 <= capacity < the count is
 * O3DMI_ERR_CAPACITY, both with nothing written, labels_out_dev included (a
 * caller who wants the labels alone passes capacity = m). A triangle's area is
 * 0.5 |(p0 - p1) x (p0 - p2)| in float64 from the positions widened (legacy
 * is float64
 * throughout); a cluster's area adds its triangles in ascending triangle
 * index, runs of 512 members first, the run sums in order then (upstream:
 * BFS order; equal to rounding). positions_dev may be NULL when no area is
 * wanted. m == 0: zero clusters, O3DMI_OK. */
int o3dmi_trianglemesh_cluster_connected_triangles(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int32_t* labels_out_dev, int64_t* n_clusters_out,
        int64_t* cluster_n_triangles_out_dev, double* cluster_area_out_dev,
        int64_t capacity, o3dmi_stream_t stream);

/* The selections share one chain: a vertex mask, its exclusive prefix sum (the
 * new index of a kept vertex: upstream's UpdateTriangleIndicesByVertexMask) and
 * the remap of the kept triangles, which keep their input order; kept
 * vertices keep ascending original index. Masks are uint8 {v} / {m} holding
 * 0 / 1 and go to o3dmi_pointcloud_select_by_mask for the attribute rows of
 * the vertices and of the triangles. triangles_out_dev holds m rows in the
 * index dtype. */

/* TriangleMesh::SelectFacesByMask: keeps the triangles with tri_mask_dev != 0
 * and the vertices they name. */
int o3dmi_trianglemesh_select_faces_by_mask(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        const uint8_t* tri_mask_dev, uint8_t* vertex_mask_out_dev,
        void* triangles_out_dev, int64_t* n_triangles_out,
        int64_t* n_vertices_out, o3dmi_stream_t stream);

/* TriangleMesh::SelectByIndex: keeps the vertices named by indices_dev int64
 * {k} (duplicates count once; an index outside [0, v) is ignored and counted
 * in *n_ignored_out, as upstream warns and continues) and the triangles all
 * three of whose vertices are kept (tri_mask_out_dev {m}). */
int o3dmi_trianglemesh_select_by_index(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        const int64_t* indices_dev, int64_t k, uint8_t* vertex_mask_out_dev,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, int64_t* n_vertices_out,
        int64_t* n_ignored_out, o3dmi_stream_t stream);

/* TriangleMesh::RemoveUnreferencedVertices: SelectFacesByMask with every
 * triangle kept. */
int o3dmi_trianglemesh_remove_unreferenced_vertices(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* vertex_mask_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, o3dmi_stream_t stream);

/* ---- TriangleMesh sampling, closest points and metrics -----------------------
 * (t/geometry/TriangleMesh.cpp:1866-1967, kernel/TriangleMeshCPU.cpp:75-186,
 * t/geometry/RaycastingScene.cpp:206-353 and 1464-1517. Upstream runs all of
 * it on the host: a sequential sampling loop and Embree point queries.) The
 * mesh rules above hold. All synchronise. */

/* The draw of sampled point j >= 0, a pure host function of (seed, j), in
 * uint64 arithmetic that wraps: h_k = SplitMix64(seed + 0x9E3779B97F4A7C15 *
 * (3 j + k + 1)), k = 0, 1, 2 (the finaliser of o3dmi_sample_index), and
 *   *u_out  = (double)(h_0 >> 11) * 2^-53, which picks the triangle,
 *   *r1_out = (float)(h_1 >> 40) * 2^-24,
 *   *r2_out = (float)(h_2 >> 40) * 2^-24,
 * all in [0, 1) and exact. */
int o3dmi_mesh_sample_draw(uint64_t seed, int64_t j, double* u_out,
                           float* r1_out, float* r2_out);

/* TriangleMesh::SamplePointsUniformly, every point a pure function of the
 * mesh, seed and its index (upstream: a global Mersenne engine and
 * std::discrete_distribution).
 *  - The triangle. The areas are those of
 *    o3dmi_trianglemesh_compute_triangle_areas, widened to double. Level 0 is
 *    the areas in consecutive groups of 512, P[i] the inclusive prefix inside
 *    i's group, added in index order; level k + 1 holds each group's last
 *    prefix, grouped the same way, until one group is left. A = the top
 *    group's last prefix, x = u * A. From the top: in the current group the
 *    first i with x < P[i] (none, by rounding: the last i whose own value is
 *    > 0); x -= the prefix before i; on to group i one level down. No
 *    floating-point scan across groups, and A TRIANGLE OF AREA 0 IS NEVER
 *    DRAWN.
 *  - The point, upstream's statements without contraction: wts = {1 -
 *    sqrt(r1), sqrt(r1) * (1 - r2), sqrt(r1) * r2} in float, out[c] = (wts[0]
 *    * a[c] + wts[1] * b[c]) + wts[2] * c[c] in the position dtype (a float
 *    times a double widens).
 *  - normals_out_dev {n,3} (optional): vertex_normals_dev {v,3} mixed the
 *    same way when given, else triangle_normals_dev {m,3} copied; both in the
 *    position dtype. colors_out_dev {n,3} float (optional): vertex_colors_dev
 *    {v,3} of color_dtype O3DMI_F32, or O3DMI_U8 / O3DMI_U16 divided by 255 /
 *    65535 in float first, mixed in float. triangles_out_dev int32 {n}
 *    (optional): the triangle of every point. The albedo / texture_uvs path
 *    is not offered.
 * number_of_points <= 0 or >= 2^31, m == 0, v == 0, an area that is not
 * finite, A not finite or not > 0, an output wanted without its input, a NULL
 * pointer: O3DMI_ERR_INVALID_ARG with the outputs untouched. */
int o3dmi_trianglemesh_sample_points_uniformly(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int64_t number_of_points, uint64_t seed,
        const void* vertex_normals_dev, const void* triangle_normals_dev,
        const void* vertex_colors_dev, int color_dtype, void* points_out_dev,
        void* normals_out_dev, float* colors_out_dev,
        int32_t* triangles_out_dev, o3dmi_stream_t stream);

/* Closest points on a mesh: RaycastingScene::ComputeClosestPoints /
 * ComputeDistance for one triangle geometry. Float32 positions and queries
 * only, as upstream's scene (Float64: O3DMI_ERR_UNSUPPORTED).
 *
 * The distance of a query q to a triangle t = (a, b, c), in float without
 * contraction, every dot product (x x + y y) + z z: p, u, v = upstream's
 * closestPointTriangle branch for branch; e2 = ((dx dx) + dy dy) + dz dz of
 * q - p; b2 = the same expression on the per-axis gap max(lo - q, q - hi, 0)
 * between q and t's own bounding box; d2(q, t) = max(e2, b2), a NaN e2 (a
 * degenerate triangle) staying NaN. The clamp by b2 makes pruning on box
 * distances exact (closestPointTriangle has no error bound on slivers) and
 * changes e2 only where it is a rounding artefact.
 *
 * The result of a query is the minimum of d2 over ALL triangles, the LOWEST
 * triangle index on equal d2 (upstream: the first in Embree's traversal
 * order): a pure function of mesh and query, whatever the tree. Outputs, each
 * optional (NULL): points {q,3}; primitive_ids uint32 {q}; primitive_uvs
 * {q,2}; primitive_normals {q,3} = cross(b - a, c - a) of the winner divided
 * by its norm sqrt((x x + y y) + z z) when that is > 0; distance {q} =
 * sqrt(d2). When no triangle has a non-NaN d2: id 0xFFFFFFFF, distance +inf,
 * the other rows 0 (upstream leaves them uninitialised).
 *
 * The structure is a linear BVH: 30-bit Morton codes of the triangle boxes'
 * centres in the box of the referenced vertices, the stable pair sort, a
 * Karras radix tree over (code, sorted position), boxes refitted bottom-up.
 * The handle owns copies of what it needs: the caller may free the mesh.
 * A triangle index out of range, a NaN / Inf vertex or query coordinate,
 * m == 0, a NULL pointer, a negative count: O3DMI_ERR_INVALID_ARG with the
 * outputs untouched. q == 0 is O3DMI_OK with nothing written. */
typedef struct o3dmi_mesh_bvh o3dmi_mesh_bvh_t;
int o3dmi_mesh_bvh_create(const void* positions_dev, int64_t v, int dtype,
                          const void* triangles_dev, int64_t m,
                          int index_dtype, o3dmi_mesh_bvh_t** bvh_out,
                          o3dmi_stream_t stream);
int o3dmi_mesh_bvh_destroy(o3dmi_mesh_bvh_t* bvh);
int o3dmi_mesh_bvh_closest_points(const o3dmi_mesh_bvh_t* bvh,
                                  const void* queries_dev, int64_t q,
                                  int dtype, void* points_out_dev,
                                  uint32_t* primitive_ids_out_dev,
                                  void* primitive_uvs_out_dev,
                                  void* primitive_normals_out_dev,
                                  void* distance_out_dev,
                                  o3dmi_stream_t stream);
/* The one-shot forms: build, query, free. `dtype` is that of the positions
 * and of the queries. */
int o3dmi_trianglemesh_closest_points(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* queries_dev, int64_t q, void* points_out_dev,
        uint32_t* primitive_ids_out_dev, void* primitive_uvs_out_dev,
        void* primitive_normals_out_dev, void* distance_out_dev,
        o3dmi_stream_t stream);
int o3dmi_trianglemesh_compute_distance(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* queries_dev, int64_t q, void* distance_out_dev,
        o3dmi_stream_t stream);

/* TriangleMesh::ComputeMetrics: n_sampled_points points on either mesh
 * (o3dmi_trianglemesh_sample_points_uniformly; MESH 1 WITH `seed`, MESH 2
 * WITH seed + 1), distance12 = the samples of mesh 1 against mesh 2 and
 * distance21 likewise (the d2 above), the reduction of
 * o3dmi_pointcloud_compute_metrics on the device and o3dmi_metrics_from_sums
 * with n1 = n2 = n_sampled_points. Float32 meshes only (upstream's chain
 * throws on Float64 at the scene). values_out is a HOST array; raw_out
 * (optional) receives the sums, second_pass_queries = 0. Errors are those of
 * the parts, raised before any output is written. */
int o3dmi_trianglemesh_compute_metrics(
        const void* positions1_dev, int64_t v1, const void* triangles1_dev,
        int64_t m1, int index_dtype1, const void* positions2_dev, int64_t v2,
        const void* triangles2_dev, int64_t m2, int index_dtype2, int dtype,
        const int32_t* metrics, int n_metrics, const float* fscore_radius,
        int n_radii, int64_t n_sampled_points, uint64_t seed,
        float* values_out, int64_t values_capacity,
        o3dmi_pointcloud_metrics_raw_t* raw_out, o3dmi_stream_t stream);

/* ---- Ray queries on a mesh ----------------------------------------------------
 * RaycastingScene::CastRays, TestOcclusions, CountIntersections,
 * ListIntersections, ComputeOccupancy, ComputeSignedDistance and
 * CreateRaysPinhole (t/geometry/RaycastingScene.cpp:486-1100, 1325-1462,
 * 1520-1674) for one triangle geometry, on the tree of o3dmi_mesh_bvh_create.
 * Upstream runs them on the host through Embree, whose intersector and
 * traversal order cannot be matched bit for bit; as for the closest points,
 * every answer here is a PURE FUNCTION OF THE MESH AND THE RAY, the same for
 * any tree, traversal order and launch shape. Float32 only (Float64:
 * O3DMI_ERR_UNSUPPORTED). All synchronise.
 *
 * A ray is six floats (o, d); d is not normalised and t is in units of |d|.
 * The pair of a ray with range (tnear, tfar] and a triangle t = (a, b, c), in
 * float without contraction, every dot product (x x + y y) + z z:
 *   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p; a miss when det == 0 or
 *   det is NaN (a degenerate triangle, a zero direction); no back-face
 *   culling; inv = 1 / det, s = o - a, u = (s . p) inv, q = s x e1,
 *   v = (d . q) inv, t_e = (e2 . q) inv; hit_e = u >= 0 && v >= 0 &&
 *   u + v <= 1 (u weighs vertex 1 and v vertex 2, as primitive_uvs above).
 *   The slab interval of t's own bounding box: per axis with d_k != 0,
 *   (lo_k - o_k) / d_k and (hi_k - o_k) / d_k (divisions), their min entering
 *   and their max leaving; an axis with d_k == 0 empties the interval when
 *   o_k is outside [lo_k, hi_k]; T0 = max(the entries, tnear), T1 = min(the
 *   exits, tfar).
 *   The pair HITS iff hit_e && T0 <= T1 && t_e > tnear && t_e <= tfar (a ray
 *   that starts on the surface does not hit it at t = 0), with the parameter
 *   t = min(max(t_e, T0), T1), a zero made positive. The clamp makes pruning
 *   on node boxes exact (subtract, divide, min and max are monotone, so a
 *   containing box's interval contains t) and moves t_e only where it already
 *   disagrees with the triangle's own box.
 * Moeller-Trumbore is not watertight: a ray through a shared edge can be
 * counted twice or not at all, which is why upstream votes with three rays.
 *
 * A NaN / Inf ray or point component, a NaN tnear / tfar, a NULL pointer, a
 * negative count: O3DMI_ERR_INVALID_ARG with the outputs untouched (upstream:
 * undefined). q == 0 is O3DMI_OK with nothing written. */

#define O3DMI_RAYCAST_INVALID_ID 0xFFFFFFFFu

/* CastRays (tnear = 0, tfar = +inf): the minimum t over the hitting pairs, the
 * LOWEST triangle index on equal t (upstream: Embree's first). Outputs, each
 * optional (NULL): t_hit {q}; geometry_ids uint32 {q} (0); primitive_ids
 * uint32 {q}; primitive_uvs {q,2} recomputed from the winner;
 * primitive_normals {q,3} = cross(b - a, c - a) by the closest points' rule.
 * No hit: t_hit +inf, both ids O3DMI_RAYCAST_INVALID_ID, the other rows 0. */
int o3dmi_mesh_bvh_cast_rays(const o3dmi_mesh_bvh_t* bvh, const void* rays_dev,
                             int64_t q, int dtype, void* t_hit_out_dev,
                             uint32_t* geometry_ids_out_dev,
                             uint32_t* primitive_ids_out_dev,
                             void* primitive_uvs_out_dev,
                             void* primitive_normals_out_dev,
                             o3dmi_stream_t stream);

/* TestOcclusions: occluded_out_dev uint8 {q} = 1 when a pair hits within
 * (tnear, tfar], else 0. */
int o3dmi_mesh_bvh_test_occlusions(const o3dmi_mesh_bvh_t* bvh,
                                   const void* rays_dev, int64_t q, int dtype,
                                   float tnear, float tfar,
                                   uint8_t* occluded_out_dev,
                                   o3dmi_stream_t stream);

/* CountIntersections: counts_out_dev int32 {q} = the number of DISTINCT
 * VALUES OF t among the hitting pairs on (0, +inf] (upstream: one more
 * whenever a candidate's t differs from the previous candidate's in Embree's
 * traversal order, which approximates that number and is not a function of
 * the input). A duplicated triangle does not raise the count. */
int o3dmi_mesh_bvh_count_intersections(const o3dmi_mesh_bvh_t* bvh,
                                       const void* rays_dev, int64_t q,
                                       int dtype, int32_t* counts_out_dev,
                                       o3dmi_stream_t stream);

/* ListIntersections: one entry per distinct t, IN ASCENDING t PER RAY, with
 * the lowest triangle index at that t (upstream: Embree's order). The entries
 * of ray i are [ray_splits[i], ray_splits[i + 1]). ray_splits_out_dev int64
 * {q + 1} (optional) and *total_out = ray_splits[q] are always written;
 * capacity < 0 only counts; 0 <= capacity < the total is O3DMI_ERR_CAPACITY
 * with nothing else written; a total above 2^31 - 1 is
 * O3DMI_ERR_UNSUPPORTED. The entry arrays hold `capacity` rows, each optional
 * (NULL): ray_ids int64, t_hit, geometry_ids uint32 (0), primitive_ids uint32,
 * primitive_uvs {.,2} (upstream: uint32 ray_splits and ray_ids). */
int o3dmi_mesh_bvh_list_intersections(
        const o3dmi_mesh_bvh_t* bvh, const void* rays_dev, int64_t q,
        int dtype, int64_t* ray_splits_out_dev, int64_t capacity,
        int64_t* total_out, int64_t* ray_ids_out_dev, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, o3dmi_stream_t stream);

/* VoteInsideOutside's ray directions on the host: out[3 j + k] = 1 + r, r
 * drawn with upstream's statements (std::mt19937 gen(42),
 * std::uniform_real_distribution<float>(-0.001, 0.001)) in the column-major
 * order of upstream's 3 x nsamples matrix, so direction j is out[3 j .. 3 j +
 * 2]. nsamples must be odd and >= 1, here and below. */
int o3dmi_raycast_vote_directions(int nsamples, float* out);

/* ComputeOccupancy / ComputeSignedDistance: a point is inside when more than
 * nsamples / 2 of its rays (the point, direction j) have an odd count.
 * Occupancy is 1 inside and 0 outside; the signed distance is the closest
 * points' distance times -1 inside and +1 outside. The rays of a point run in
 * neighbouring lanes of one wave and the vote is written directly:
 * upstream's {nsamples q, 6} ray tensor and its count tensor never exist. */
int o3dmi_mesh_bvh_compute_occupancy(const o3dmi_mesh_bvh_t* bvh,
                                     const void* points_dev, int64_t q,
                                     int dtype, int nsamples,
                                     void* occupancy_out_dev,
                                     o3dmi_stream_t stream);
int o3dmi_mesh_bvh_compute_signed_distance(const o3dmi_mesh_bvh_t* bvh,
                                           const void* points_dev, int64_t q,
                                           int dtype, int nsamples,
                                           void* distance_out_dev,
                                           o3dmi_stream_t stream);

/* CreateRaysPinhole: intrinsic (3 x 3) and extrinsic (4 x 4) are row-major
 * HOST doubles. K^-1 (the adjugate over the determinant), R^T, C = -(R^T t)
 * and R^T K^-1 are formed in double, every sum (x + y) + z, and narrowed
 * once (upstream: Eigen's inverse). rays_out_dev {height, width, 6} float:
 * C and the rows (m0 (x + 0.5) + m1 (y + 0.5)) + m2 of R^T K^-1. A matrix
 * that is not finite or whose K is singular: O3DMI_ERR_INVALID_ARG. */
int o3dmi_create_rays_pinhole(const double* intrinsic, const double* extrinsic,
                              int width, int height, void* rays_out_dev,
                              o3dmi_stream_t stream);

/* The one-shot forms: build, query, free. `dtype` is that of the positions
 * and of the rays / points. */
int o3dmi_trianglemesh_cast_rays(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* rays_dev, int64_t q, void* t_hit_out_dev,
        uint32_t* geometry_ids_out_dev, uint32_t* primitive_ids_out_dev,
        void* primitive_uvs_out_dev, void* primitive_normals_out_dev,
        o3dmi_stream_t stream);
int o3dmi_trianglemesh_compute_signed_distance(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* points_dev, int64_t q, int nsamples,
        void* distance_out_dev, o3dmi_stream_t stream);

/* ---- TriangleMesh clean-up, smoothing filters and vertex clustering ----------
 * (legacy geometry/TriangleMesh.cpp:153-440 and 680-860, Smoothing.h:29-65,
 * TriangleMeshSimplification.cpp:72-244. Upstream has these as sequential host
 * loops of the legacy class only.) The rules of the TriangleMesh operators
 * above hold: the triangle indices are range-checked on the device before
 * anything is written, v < 2^31 (v < 2^30 where a vertex table is built:
 * remove_duplicated_vertices, simplify_vertex_clustering), m <= 2^29, all
 * synchronise. The filters and the clustering refuse a NaN / Inf position with
 * O3DMI_ERR_INVALID_ARG and the outputs untouched. Vertex normals and colours,
 * where taken, are {v,3} of attr_dtype, which must be the position dtype:
 * another one is O3DMI_ERR_UNSUPPORTED.
 *
 * The de-duplications share one table: rep[i] = THE LOWEST INDEX j <= i WHOSE
 * KEY EQUALS KEY i, a pure function of the input whatever the arrival order
 * (equal keys meet in one slot of an open-addressing table of indices and keep
 * the lowest with an integer atomic minimum). The first occurrence of a key is
 * kept, as legacy's loops keep it. */

/* Legacy RemoveDuplicatedVertices. The key is the coordinate triple by VALUE
 * (std::tuple<double, double, double> equality; Float32 widens exactly): -0
 * equals +0, and a row with a NaN coordinate equals nothing, itself included,
 * so it is kept. vertex_mask_out_dev uint8 {v}: 1 = first occurrence (kept
 * vertices keep ascending index; compact the attribute rows with
 * o3dmi_pointcloud_select_by_mask). triangles_out_dev {m,3} in the index
 * dtype: the triangles, in order, remapped through index_old_to_new[i] =
 * rank(rep[i]). */
int o3dmi_trianglemesh_remove_duplicated_vertices(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        uint8_t* vertex_mask_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, o3dmi_stream_t stream);

/* Legacy RemoveDuplicatedTriangles. The key is the index triple rotated by
 * legacy's branch statements (TriangleMesh.cpp:744-760, ties included):
 * t0 <= t1 ? (t0 <= t2 ? (t0,t1,t2) : (t2,t0,t1))
 *          : (t1 <= t2 ? (t1,t2,t0) : (t2,t0,t1)).
 * Orientation is kept: (0,1,2), (1,2,0), (2,0,1) are one key, (0,2,1) another.
 * tri_mask_out_dev uint8 {m}: 1 = first occurrence; triangles_out_dev: the kept
 * rows in input order, unchanged, in the index dtype. */
int o3dmi_trianglemesh_remove_duplicated_triangles(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, o3dmi_stream_t stream);

/* Legacy RemoveDegenerateTriangles: keeps t0 != t1 && t1 != t2 && t2 != t0
 * (indices only, as legacy). Outputs as above. */
int o3dmi_trianglemesh_remove_degenerate_triangles(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        uint8_t* tri_mask_out_dev, void* triangles_out_dev,
        int64_t* n_triangles_out, o3dmi_stream_t stream);

/* Legacy ComputeAdjacencyList as CSR: the neighbours of vertex u are
 * neighbours_out_dev[row_splits[u] .. row_splits[u + 1]) in the index dtype,
 * IN ASCENDING INDEX WITHOUT REPEATS (upstream: an unordered_set's order).
 * The set is that of legacy's six inserts per triangle: a triangle (6,6,7)
 * makes 6 its own neighbour. Built from the unique (lo, hi) runs of the edge
 * table of o3dmi_trianglemesh_get_non_manifold_edges and one more pair sort
 * by hi. row_splits_out_dev int64 {v + 1}. *n_entries_out is always set;
 * capacity < 0 only counts and 0 <= capacity < the number is
 * O3DMI_ERR_CAPACITY, both with nothing written. */
int o3dmi_trianglemesh_compute_adjacency_list(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int64_t* row_splits_out_dev, void* neighbours_out_dev,
        int64_t capacity, int64_t* n_entries_out, o3dmi_stream_t stream);

/* The four filters share one driver. The arithmetic is legacy's, float64
 * throughout: the inputs are widened on load, the buffers between passes are
 * float64 and the result is narrowed once at the end, so a Float64 mesh
 * reproduces the legacy statements bit for bit GIVEN THE NEIGHBOUR ORDER,
 * which is pinned to ascending index: every sum is ((0 + x_a) + x_b) + ...
 * over the adjacency list above, without contraction or float atomics.
 *   sharpen    next = prev + strength * (prev * nb - sum)       (:192-233)
 *   simple     next = (prev + sum) / (1 + nb)                   (:263-300)
 *     with sum the neighbours' values and nb the list length as a double;
 *   laplacian  per neighbour dist = sqrt((dx dx + dy dy) + dz dz) on the
 *              CURRENT positions, w = 1.0 / (dist + 1e-12), total += w,
 *              sum += w * x_nb (a multiply, then an add);
 *              next = prev + factor * (sum / total - prev) when total > 0,
 *              else prev                    (Smoothing.h:44-62, :336-342)
 *   taubin     per iteration the laplacian pass with lambda, then with mu; the
 *              second weighs with the positions the first one made.
 * scope is upstream's FilterScope: 0 All, 1 Color, 2 Normal, 3 Vertex.
 * normals_dev / colors_dev may be NULL (the mesh has none); an output is
 * needed for every input given and may not overlap any input. DIFFERENCES
 * FROM UPSTREAM: an attribute outside the scope is copied unchanged and the
 * weights always use the current positions (upstream leaves such vectors
 * unwritten and, for the Normal / Color scopes with several iterations, swaps
 * them into the weight positions); iterations <= 0 returns a copy (upstream:
 * unwritten vectors). */
int o3dmi_trianglemesh_filter_sharpen(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double strength, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream);
int o3dmi_trianglemesh_filter_smooth_simple(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        int scope, void* positions_out_dev, void* normals_out_dev,
        void* colors_out_dev, o3dmi_stream_t stream);
int o3dmi_trianglemesh_filter_smooth_laplacian(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double lambda_filter, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream);
int o3dmi_trianglemesh_filter_smooth_taubin(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double lambda_filter, double mu, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream);

/* Legacy SimplifyVertexClustering. min_bound = GetMinBound() - 0.5 *
 * voxel_size in float64 from the positions widened; a vertex's voxel is
 * int(floor((p - min_bound) / voxel_size)) per axis. voxel_size <= 0 (or not
 * finite), or voxel_size * INT_MAX < the largest extent of the padded bounds
 * (upstream's own check): O3DMI_ERR_INVALID_ARG. A cluster's new index is the
 * rank of its first vertex in vertex order (legacy's voxel_vert_ind); its
 * members are listed in ascending old index by a stable pair sort.
 *   contraction 0 (Average): the float64 sum of the members in that order,
 *     divided by their number, for positions, normals and colours (upstream:
 *     its unordered_set's order; equal to rounding).
 *   contraction 1 (Quadric): for each member in order, each triangle that
 *     names it in ascending triangle index, once per member, adds
 *     Quadric(plane, area): plane is ComputeTrianglePlane statement for
 *     statement (TriangleMesh.cpp:1248-1262, every dot product (x x + y y) +
 *     z z, the zero plane when the norm is 0), area the float64 triangle area
 *     of o3dmi_trianglemesh_cluster_connected_triangles, A_ij += (w n_i) n_j,
 *     b_i += (w d) n_i. With det = a00 (a11 a22 - a12 a21) - a01 (a10 a22 -
 *     a12 a20) + a02 (a10 a21 - a11 a20) and C the cofactor matrix from the
 *     same products, |det| > 1e-4 gives x_i = -((C_i0 b0 + C_i1 b1) + C_i2 b2)
 *     / det (upstream: Eigen's pivoted LDLT; equal to rounding), else the
 *     Average. Normals and colours are averaged either way.
 * Triangles: the three vertices mapped; a triangle with two equal new indices
 * is dropped; the rest is rotated by legacy's statements (:217-227) and the
 * first occurrence of each triple is kept in input order (upstream: its
 * unordered_set's order). Opposite orientations both stay. Outputs are sized
 * by the input: positions_out_dev / normals_out_dev / colors_out_dev {v,3}
 * (the first *n_vertices_out rows are written), triangles_out_dev {m,3} in the
 * index dtype (the first *n_triangles_out rows). normals_dev / colors_dev may
 * be NULL; an output is needed for every input given. */
int o3dmi_trianglemesh_simplify_vertex_clustering(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        double voxel_size, int contraction, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, void* triangles_out_dev,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream);

/* Legacy SubdivideMidpoint / SubdivideLoop (geometry/TriangleMeshSubdivide.cpp:
 * 18-94, 96-357), statement for statement in float64 on the positions, normals
 * and colours widened: a Float32 mesh is widened once, stays float64 across
 * the iterations and is narrowed once at the end. No sum is contracted or
 * atomic; each has the order stated here.
 *   Numbering, per iteration: the old vertices keep their indices; the new
 *     vertex of the unordered edge (lo, hi) is v_old + r, r the rank of the
 *     edge's lowest slot e = 3 t + k (k = 0, 1, 2 for (v0, v1), (v1, v2),
 *     (v2, v0)) among the lowest slots of all edges. That is upstream's
 *     first-encounter order (:57-58, :236), exactly. The edge (a, a) of a
 *     degenerate triangle is an edge like any other and gets a vertex, so
 *     *n_vertices_out follows the walk, not E' = 2 E + 3 M.
 *   Triangles: triangle t becomes rows 4 t .. 4 t + 3 = (v0, v01, v20), (v01,
 *     v1, v12), (v12, v2, v20), (v01, v12, v20) (:77-84, :337-344);
 *     *n_triangles_out = 4^n m.
 *   Midpoint: the new vertex is 0.5 * (x[lo] + x[hi]) per component of every
 *     attribute; the old ones are copied. Bit for bit upstream's result on a
 *     Float64 mesh.
 *   Loop, new vertex (:186-234): s = x[v0] + x[v1]; the edge's multiplicity n
 *     is the number of DISTINCT triangles that name it (upstream's set of
 *     triangle indices: (a, a, b) names (a, b) twice and counts once, a
 *     triangle listed twice counts twice; o3dmi_trianglemesh_get_non_manifold_
 *     edges counts slots instead). n < 2: s * 0.5. Else s * (3. / 8.), then
 *     += (1. / (4. * n)) * x[opp] over the edge's triangles in ascending
 *     triangle index (upstream: its unordered_set's order; equal to rounding),
 *     opp the first of t0, t1, else t2, that differs from both ends.
 *   Loop, old vertex (:119-176): nbs is the list of
 *     o3dmi_trianglemesh_compute_adjacency_list (ascending, no repeats, the
 *     vertex itself for (a, a, b)), the boundary ones those whose edge has
 *     multiplicity 1. >= 2 boundary neighbours: beta = 1. / 8. over them;
 *     else |nbs| == 3: beta = 3. / 16.; else beta = 3. / (8. * |nbs|), over
 *     all; alpha = 1. - count * beta; alpha * x[v], then += beta * x[nb] in
 *     ascending neighbour index (upstream: set order; equal to rounding).
 *     A vertex WITHOUT neighbours is copied unchanged; upstream computes beta
 *     = 3 / (8 * 0) = inf and alpha = NaN and turns every unreferenced vertex
 *     into NaN. Upstream's two warnings (non-manifold edge, > 2 boundary
 *     neighbours) are no errors; the statements run as written. The topology
 *     is rebuilt from each iteration's triangle list.
 * number_of_iterations <= 0 (or m == 0) copies the mesh. normals_dev /
 * colors_dev may be NULL; given, they need the position dtype
 * (O3DMI_ERR_UNSUPPORTED) and, unless only counting, an output. Refused with
 * O3DMI_ERR_INVALID_ARG before anything is allocated: 4^n m > 2^29, or v +
 * (4^n - 1) m >= 2^31 (the most vertices n iterations can add; vertex ids are
 * int32 in the tables); before anything is written: a triangle index outside
 * [0, v), a position, normal or colour that is not finite (referenced or
 * not). The vertex count is data dependent, so the protocol is
 * o3dmi_trianglemesh_compute_adjacency_list's: vertex_capacity < 0 only sets
 * *n_vertices_out and *n_triangles_out (the outputs may be NULL; the index
 * side runs, no attribute is touched beyond the finiteness check);
 * vertex_capacity < *n_vertices_out sets both and is O3DMI_ERR_CAPACITY with
 * the outputs untouched; else positions_out_dev / normals_out_dev /
 * colors_out_dev {vertex_capacity,3} get *n_vertices_out rows and
 * triangles_out_dev {4^n m,3} in the index dtype every row. */
int o3dmi_trianglemesh_subdivide_midpoint(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int number_of_iterations, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream);
int o3dmi_trianglemesh_subdivide_loop(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int number_of_iterations, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream);

/* ---- ClipPlane / SlicePlane ---------------------------------------------------
 * t::geometry::TriangleMesh::ClipPlane / SlicePlane (t/geometry/
 * TriangleMesh.cpp:649-716). Upstream hands both to VTK on a host copy
 * (vtkClipPolyData + vtkCleanPolyData, vtkCutter), which cannot be matched bit
 * for bit; here the result is a pure function of the input by the rules
 * below. All arithmetic is float64 on the positions (normals, colours)
 * widened, without contraction, narrowed once on the store. Float32 / Float64
 * positions, Int32 / Int64 indices.
 *   Signed value: s_i = ((n.x (x_i - o.x) + n.y (y_i - o.y)) + n.z (z_i -
 *     o.z)), o = point and n = normal, host doubles {3}. The normal is NOT
 *     normalised (vtkPlane::EvaluateFunction): a contour value is in units of
 *     |n| times distance; upstream's "signed distance" holds for a unit normal.
 *   Inside: vertex i is inside for the contour value c iff s_i >= c (VTK's
 *     clip case index). Clip is the contour c = 0.
 *   Cut point of an edge with one end u inside and the other outside: if s_u
 *     == c it IS vertex u, no new point is made and all such edges at u share
 *     it. Otherwise it belongs to the unordered edge (lo, hi), lo < hi by
 *     index, whichever triangle names it and in whichever direction: t = (c -
 *     s_lo) / (s_hi - s_lo), every attribute x_lo + t * (x_hi - x_lo)
 *     (positions, and normals and colours if given; normals are not
 *     renormalised). Two triangles sharing the edge get the same bits.
 *   Rotation: a triangle keeps its winding; with one vertex inside it is
 *     rotated so that this vertex is first, with two inside so that the
 *     outside one is last: (a, b, c), and ab, bc, ca are the cut points of
 *     those edges. Edge k of triangle t is (t_k, t_(k+1)%3) and its slot 3 t +
 *     k, as in subdivision.
 *   Coincident input vertices are NOT merged (upstream's vtkCleanPolyData
 *     merges them): call o3dmi_trianglemesh_remove_duplicated_vertices first.
 * Refused with O3DMI_ERR_INVALID_ARG, outputs untouched: from the sizes
 * alone, before anything is allocated or read, clip m > 2^28 (up to 2 m output
 * triangles), slice K m > 2^29, either v + 3 m >= 2^31; a non-finite point,
 * normal or contour value; normal == (0, 0, 0); a triangle index outside [0,
 * v); a position, given normal or colour that is not finite, referenced or
 * not; an s_i that is not finite. Normals / colours of another dtype than the
 * positions: O3DMI_ERR_UNSUPPORTED.
 *
 * o3dmi_trianglemesh_clip_plane keeps the part with s >= 0. Pieces per input
 * triangle, in ascending triangle index: none inside, nothing; all inside,
 * the triangle itself; one inside, (a, ab, ca); two inside, (a, b, bc), then
 * (a, bc, ca) (upstream: VTK's case table picks the diagonal). Any output
 * triangle that names a vertex twice is dropped, whatever its origin: a
 * triangle touching the plane from the negative side with one vertex or one
 * edge vanishes, a triangle lying in the plane stays, a degenerate input
 * triangle vanishes (upstream's cleaner turns it into a line).
 *   Vertices: first the old vertices that at least one output triangle names,
 *     in ascending old index, copied bit for bit (unreferenced and outside
 *     vertices are gone, as upstream); then the new cut vertices, in ascending
 *     order of their edge's lowest slot among the slots whose cut point an
 *     output triangle names. Every new vertex is named by an output triangle.
 *   Outputs: positions_out_dev / normals_out_dev / colors_out_dev
 *     {vertex_capacity,3}; triangles_out_dev {triangle_capacity,3} in the
 *     index dtype; optional (may be NULL) triangle_source_out_dev
 *     {triangle_capacity} in the index dtype, the input triangle of each
 *     output triangle; optional vertex_source_out_dev {vertex_capacity,2} in
 *     the index dtype together with vertex_t_out_dev {vertex_capacity}
 *     Float64: (i, i) and 0 for an old vertex, (lo, hi) and t for a cut
 *     vertex, from which a caller carries any other attribute.
 *   Protocol (o3dmi_trianglemesh_subdivide_midpoint's): vertex_capacity < 0
 *     only sets *n_vertices_out and *n_triangles_out; either capacity below
 *     its count sets both and is O3DMI_ERR_CAPACITY with nothing written. An
 *     empty mesh or one wholly outside gives 0 and 0. */
int o3dmi_trianglemesh_clip_plane(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const double* point, const double* normal, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity,
        void* triangle_source_out_dev, void* vertex_source_out_dev,
        double* vertex_t_out_dev, int64_t* n_vertices_out,
        int64_t* n_triangles_out, o3dmi_stream_t stream);

/* o3dmi_trianglemesh_slice_plane: the cross-sections at the n_contours values
 * contour_values (a host array; 0 of them give an empty result). For each
 * contour in the order given and each triangle in ascending index, one line
 * from where the winding leaves the inside to where it re-enters: one inside,
 * (ab, ca); two inside, (bc, ca); none or all inside, nothing. A line whose
 * two ends are the same point is dropped and numbers nothing: a triangle
 * touching the contour with one vertex from below gives nothing, a triangle
 * in the contour plane gives nothing, an in-plane edge is emitted by each
 * adjacent triangle whose third vertex is below (once for a surface crossing
 * the plane there).
 *   Points: a point is a vertex point (s_u == c) or an edge point, unique per
 *     contour and not shared between contours (vtkCutter's per-contour merge).
 *     Numbering is contour-major; within a contour a point's place is the
 *     lowest slot 3 t + k among the kept lines' end uses, each end attached
 *     to the edge slot it lies on. For c = 0 an edge point has the bits of
 *     clip's cut vertex of the same edge.
 *   Outputs: points_out_dev (normals_out_dev / colors_out_dev interpolated
 *     when given) {point_capacity,3}; lines_out_dev {line_capacity,2} in the
 *     index dtype; optional line_triangle_out_dev {line_capacity} in the index
 *     dtype, line_contour_out_dev {line_capacity} Int32, and point_source_out_
 *     dev {point_capacity,2} with point_t_out_dev as for clip. point_capacity
 *     < 0 only counts; either capacity below its count sets both counts and
 *     is O3DMI_ERR_CAPACITY with nothing written. */
int o3dmi_trianglemesh_slice_plane(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const double* point, const double* normal,
        const double* contour_values, int64_t n_contours, void* points_out_dev,
        void* normals_out_dev, void* colors_out_dev, int64_t point_capacity,
        void* lines_out_dev, int64_t line_capacity,
        void* line_triangle_out_dev, int32_t* line_contour_out_dev,
        void* point_source_out_dev, double* point_t_out_dev,
        int64_t* n_points_out, int64_t* n_lines_out, o3dmi_stream_t stream);

/* ---- mesh topology and intersection queries ---------------------------------
 * Legacy geometry/TriangleMesh.cpp:1016-1135, 1212-1246, 1272-1457 and
 * geometry/IntersectionTest.cpp:18-56. Every result is a pure function of the
 * mesh: it depends on no tree shape, traversal order or launch shape, and
 * lists come back in a stated order. The index calls take (triangles, m,
 * index dtype, v) as o3dmi_trianglemesh_get_non_manifold_edges does, whose
 * edge table (runs of equal (lo, hi) slots, a run's length the edge's
 * multiplicity) and count / fill protocol they share. */

/* EulerPoincareCharacteristic (:1272-1285): v + m - E, with E the number of
 * runs of the edge table; a self edge (6,6) of a triangle (6,6,7) counts, as
 * upstream's set counts it. m == 0: v. */
int o3dmi_trianglemesh_euler_poincare_characteristic(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        int64_t* characteristic_out, o3dmi_stream_t stream);

/* IsEdgeManifold (:1301-1312): *manifold_out = 1 iff no edge has multiplicity
 * > 2 (allow_boundary_edges) or != 2. m == 0: 1. */
int o3dmi_trianglemesh_is_edge_manifold(const void* triangles_dev, int64_t m,
                                        int index_dtype, int64_t v,
                                        int allow_boundary_edges,
                                        int* manifold_out,
                                        o3dmi_stream_t stream);

/* GetNonManifoldVertices (:1314-1368), upstream's loop read exactly: vertex x
 * has a WEDGE in triangle t iff x occurs exactly once in t (what the three
 * if / else if branches at :1334-1343 amount to), the wedge's link edge is
 * t's other two vertices (they may be equal), and x is non-manifold iff the
 * graph of its link edges has more than one connected component. The indices
 * are written ASCENDING into vertices_out_dev {capacity} in the index dtype;
 * capacity < 0 only counts, 0 <= capacity < the number is O3DMI_ERR_CAPACITY
 * with nothing written (*n_vertices_out is still set). DIFFERENCE FROM
 * UPSTREAM: a vertex that triangles name but that has no wedge (every such
 * triangle names it twice) is not reported; upstream dereferences begin() of
 * an empty map there, which is undefined. */
int o3dmi_trianglemesh_get_non_manifold_vertices(
        const void* triangles_dev, int64_t m, int index_dtype, int64_t v,
        void* vertices_out_dev, int64_t capacity, int64_t* n_vertices_out,
        o3dmi_stream_t stream);

/* IsOrientable / OrientTriangles (:1016-1135). Slot 3 t + k runs FORWARD iff
 * v_k < v_(k+1)%3; self edges are ignored. An edge of multiplicity 2 whose
 * slots belong to two different triangles constrains them: run the same way,
 * exactly one of the two must be flipped; run opposite ways, both or neither
 * (two slots of one triangle constrain nothing). The mesh is orientable iff
 * the constraints can all be met and no edge has multiplicity > 2.
 * triangles_out_dev {m,3} in the index dtype (NULL: not wanted): when
 * orientable, the LOWEST-INDEXED TRIANGLE OF EVERY CONNECTED COMPONENT KEEPS
 * ITS WINDING, a flipped (a, b, c) is written (a, c, b) and the rest is
 * copied; when not, a copy of the input. DIFFERENCES FROM UPSTREAM, whose
 * breadth-first search starts at *unordered_set.begin() and is therefore no
 * function of the mesh: an edge of multiplicity > 2 always makes the mesh not
 * orientable (two of its triangles must run it the same way; upstream may say
 * true, depending on its visiting order); the flip set is the canonical one
 * above (upstream: that of its visiting order, a swap of the offending pair);
 * a mesh that is not orientable is left as it was (upstream: half flipped).
 * m == 0: orientable. */
int o3dmi_trianglemesh_orient_triangles(const void* triangles_dev, int64_t m,
                                        int index_dtype, int64_t v,
                                        void* triangles_out_dev,
                                        int* orientable_out,
                                        o3dmi_stream_t stream);

/* GetSelfIntersectingTriangles (:1374-1426). The per-pair function of
 * triangles P (the lower index) and Q, in float64 on the positions widened,
 * without contraction: the pair COUNTS iff box(P) and box(Q), the exact min /
 * max of three doubles, overlap by IntersectionTest::AABBAABB's closed
 * comparisons, and IntersectionTest::TriangleTriangle3d says so: per axis mu =
 * the six points added left to right / 6, sigma = sqrt(the six squared
 * deviations added left to right / 5) + 1e-12, every deviation / sigma, then
 * Moeller's no-division test with its 1e-6 snap of the six plane distances,
 * its interval test and its coplanar branch, operation for operation (IEEE
 * sqrt and divide: the bits of an SSE2 build). The result is the set of (i,
 * j), i < j, that share no vertex INDEX (upstream's nine comparisons) and
 * count, written {n,2} in the index dtype in ASCENDING (i, j) (upstream: a
 * concurrent_vector in arbitrary order); capacity as above, < 2^31. The pairs
 * are found on the tree of o3dmi_mesh_bvh_create over the positions narrowed
 * to float with round-to-nearest, which prunes exactly: rounding is monotone,
 * so closed overlap in double implies closed overlap of the narrowed boxes,
 * and the exact test at a leaf uses the doubles. A referenced coordinate that
 * is not finite, as given or narrowed, is O3DMI_ERR_INVALID_ARG. */
int o3dmi_trianglemesh_get_self_intersecting_triangles(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        void* pairs_out_dev, int64_t capacity, int64_t* n_pairs_out,
        o3dmi_stream_t stream);

/* IsSelfIntersecting (:1428-1430): whether that set is non-empty. */
int o3dmi_trianglemesh_is_self_intersecting(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        int* intersecting_out, o3dmi_stream_t stream);

/* IsIntersecting (:1432-1457): 0 unless the two meshes' bounding boxes
 * (GetMinBound / GetMaxBound, over ALL vertices) overlap; then 1 iff some pair
 * (triangle P of this mesh, triangle Q of the other) counts by the per-pair
 * function above. DIFFERENCE FROM UPSTREAM, which applies no per-pair box
 * test here: its 1e-6 snap can report two nearly coplanar triangles whose
 * boxes are disjoint along the dropped axis; this call never does. Either
 * mesh without triangles: 0. */
int o3dmi_trianglemesh_is_intersecting(
        const void* positions_dev, int64_t v, int dtype,
        const void* triangles_dev, int64_t m, int index_dtype,
        const void* other_positions_dev, int64_t other_v, int other_dtype,
        const void* other_triangles_dev, int64_t other_m,
        int other_index_dtype, int* intersecting_out, o3dmi_stream_t stream);

/* IsWatertight (:1126-1128): is_edge_manifold(0) && no non-manifold vertex &&
 * !is_self_intersecting, in that order, stopping at the first that fails.
 * m == 0: 1. */
int o3dmi_trianglemesh_is_watertight(const void* positions_dev, int64_t v,
                                     int dtype, const void* triangles_dev,
                                     int64_t m, int index_dtype,
                                     int* watertight_out,
                                     o3dmi_stream_t stream);

/* GetVolume (:1212-1246): O3DMI_ERR_INVALID_ARG with upstream's messages when
 * the mesh is not watertight or not orientable (by the calls above). Each
 * term is p0 . (p1 x p2) / 6 in float64 from the positions widened, every
 * cross component a b - c d, the dot (x x + y y) + z z, with p0, p1, p2 the
 * triangle's vertices in index order; the terms are added by the fixed tree
 * of o3dmi_trianglemesh_surface_area (runs of 512 in index order, the run sums
 * likewise; upstream: parallel_deterministic_reduce; equal to rounding) and
 * the result is the absolute value. m == 0: 0. */
int o3dmi_trianglemesh_get_volume(const void* positions_dev, int64_t v,
                                  int dtype, const void* triangles_dev,
                                  int64_t m, int index_dtype,
                                  double* volume_out, o3dmi_stream_t stream);

/* ---- ComputeConvexHull / HiddenPointRemoval ------------------------------------
 * t::geometry::PointCloud::ComputeConvexHull / HiddenPointRemoval
 * (t/geometry/PointCloud.cpp:1668, 1608; TriangleMesh::ComputeConvexHull is
 * the hull of the vertex positions). Upstream copies the cloud to the host,
 * widens it to float64 and runs Qhull; here a quickhull runs on the device and
 * the result is a pure function of the input by the rules below
 * (docs/pointcloud_convex_hull.md). All geometry is float64 on the widened
 * coordinates, without contraction. Float32 / Float64 positions; the index
 * dtype, Int32 or Int64, holds for triangles_out_dev and
 * point_indices_out_dev alike.
 *   Predicate: point p is outside facet (a, b, c), n = (b - a) x (c - a), iff
 *     (n.x w.x + n.y w.y) + n.z w.z > eps |n| with w = p - a, eps =
 *     O3DMI_HULL_EPS_ULPS * 2^-52 * E, E the largest extent of the bounding
 *     box (o3dmi_pointcloud_min_max_bound). A point that is outside of no
 *     facet it is tested against is inside for good; Qhull's joggle is not
 *     reproduced, degenerate inputs are settled by this rule.
 *   Initial simplex: the points of lowest and highest x, the point farthest
 *     from their line, the point farthest from the plane of the three; ties go
 *     to the lowest point index. If the fourth is not outside that plane by
 *     more than eps on either side, the cloud is flat: O3DMI_ERR_SINGULAR
 *     (Qhull's QH6154), nothing written. Collinear points and copies of one
 *     point are flat.
 *   Output (the one deliberate difference from upstream, whose order is
 *     Qhull's facet traversal order and is specified nowhere): no trace of the
 *     insertion order is left. Hull vertices come in ascending input point
 *     index, point_indices_out_dev names them, positions_out_dev holds bit
 *     copies of those input rows in the input dtype. Each triangle is wound
 *     counter-clockwise seen from outside, rotated so that its lowest vertex
 *     index is first, and the triangles are sorted by (v0, v1, v2). There are
 *     2 V - 4 of them. Among coincident points only the lowest index can
 *     become a vertex (the tie rule and the strict >). Points in the plane of
 *     a facet within eps are not vertices, but an extreme point in a face of
 *     the cloud may be: it may be picked by the initial simplex.
 *   Protocol (o3dmi_trianglemesh_clip_plane's): vertex_capacity < 0 only sets
 *     *n_vertices_out and *n_triangles_out; either capacity below its count
 *     sets both and is O3DMI_ERR_CAPACITY with nothing written. V <= n and T
 *     <= 2 n - 4 always suffice.
 * Refused with O3DMI_ERR_INVALID_ARG before anything is allocated: n < 4
 * (hidden-point removal: n < 3), n >= 2^31 - 1, a NULL argument, another
 * dtype; after the finiteness gate: a NaN or Inf coordinate. Outputs are
 * untouched by every refusal. The call waits once per round of insertions
 * (the driver's comment has the list) and returns with the stream drained. */
#define O3DMI_HULL_EPS_ULPS 256
int o3dmi_pointcloud_convex_hull(
        const void* points_dev, int64_t n, int dtype, void* positions_out_dev,
        void* point_indices_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity, int index_dtype,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream);

/* HiddenPointRemoval (Katz et al.; geometry/PointCloud.cpp:791-850): the
 * spherical flip in float64 as upstream writes it, v = p - camera, norm =
 * sqrt((v.x^2 + v.y^2) + v.z^2), f = v + ((2 (radius - norm)) v) / norm; the
 * origin is added as point n, the hull of the n + 1 points is taken by the
 * rules above, then the origin vertex and every triangle that names it are
 * dropped. Vertices are the ORIGINAL rows of the kept points in ascending
 * index and point_indices_out_dev is that index list; the triangles are
 * numbered on it. camera_location: host doubles {3}. radius <= 0 or not
 * finite, a camera location that is not finite, a point whose flip is not
 * finite (a point at the camera location gives norm = 0; upstream feeds the
 * NaN to Qhull): O3DMI_ERR_INVALID_ARG. V <= n and T <= 2 n - 4 suffice (the origin, when it
 * is a vertex, takes at least three triangles with it). */
int o3dmi_pointcloud_hidden_point_removal(
        const void* points_dev, int64_t n, int dtype,
        const double* camera_location, double radius, void* positions_out_dev,
        void* point_indices_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity, int index_dtype,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream);

/* ---- GetOrientedBoundingBox / GetOrientedBoundingEllipsoid ---------------------
 * OrientedBoundingBox::CreateFromPoints(points, robust = false, method) and
 * OrientedBoundingEllipsoid::CreateFromPoints, which is what t::geometry::
 * PointCloud / TriangleMesh / LineSet::GetOrientedBoundingBox() and
 * GetOrientedBoundingEllipsoid() return (docs/bounding_volumes.md). Both start
 * from the convex hull of o3dmi_pointcloud_convex_hull, taken on the device:
 * its vertices in ascending point index widened to float64, its triangles
 * sorted by (v0, v1, v2). All arithmetic is float64 without contraction; every
 * sum is taken in a fixed tree (runs of O3DMI_BV_TREE_RUN consecutive values in
 * index order, the run sums likewise, level by level), so a result is a pure
 * function of the input.
 *   O3DMI_OBB_MINIMAL_APPROX (t/geometry/kernel/MinimumOBB.cpp:1250-1319): for
 *     hull triangle (a, b, c): u = b - a, v = c - a, w = u x v, v = w x u,
 *     each divided by its norm sqrt((x^2 + y^2) + z^2); the coordinates of hull
 *     vertex x are ((d.x r.x + d.y r.y) + d.z r.z), d = x - a, r = u, v, w
 *     (upstream multiplies by the inverse of [u v w]; the transpose is the same
 *     matrix up to rounding). The candidate's volume is (e0 e1) e2, e = hi - lo.
 *     Candidate -1 is the axis-aligned box of the hull vertices with the
 *     identity rotation, its volume taken in float64 (upstream: from the
 *     vertices cast to Float32). The smallest volume wins under a strict <, so
 *     ties go to the lowest candidate index; a NaN volume (a degenerate frame)
 *     never wins. The box: rotation = [u v w] as columns, extent = hi - lo,
 *     center = a + R ((lo + hi) / 2).
 *   O3DMI_OBB_PCA (geometry/BoundingVolume.cpp:232-286): the frame of
 *     o3dmi_bounding_box_frame_from_moments on the nine sums of the hull
 *     vertices, the minima and maxima of R^T (x - mean) by the same three-term
 *     dot, center = R ((lo + hi) / 2) + mean, extent = hi - lo.
 *   O3DMI_OBB_MINIMAL_JYLANKI: O3DMI_ERR_UNSUPPORTED. Upstream's traversal
 *     order comes from std::random_device and its searches are seeded from one
 *     edge to the next, so its result is not a function of the input.
 *   The ellipsoid (t/geometry/kernel/MinimumOBE.cpp:108-272): Khachiyan's
 *     iteration on the hull vertices with weights p_i = 1 / V: Lambda = sum p_i
 *     [a_i; 1] [a_i; 1]^T (terms (p x) y), its inverse by an L D L^T in fixed
 *     order without pivoting (a pivot <= 0 or not finite: O3DMI_ERR_SINGULAR),
 *     M_i = [a_i; 1]^T Lambda^-1 [a_i; 1] (the diagonal only), its maximum with
 *     ties to the lowest index, step = (max - 4) / (4 (max - 1)), p <- (1 -
 *     step) p, p_j += step. The loop ends when sqrt(sum (new p_i - p_i)^2) <=
 *     O3DMI_OBE_TOLERANCE or after O3DMI_OBE_MAX_ITERATIONS iterations; the rest
 *     is o3dmi_bounding_ellipsoid_from_moments on the weighted sums.
 * Outputs are HOST doubles; the rotation is row-major, as
 * o3dmi_pointcloud_obb_mask takes it. Float32 / Float64 positions. A flat cloud
 * is the hull's O3DMI_ERR_SINGULAR. Refused with O3DMI_ERR_INVALID_ARG before
 * anything is allocated: n < 4, n >= 2^31 - 1, a NULL pointer other than
 * iterations_out, another dtype, another method value; after the finiteness
 * gate: a NaN or Inf coordinate. Every refusal leaves the outputs untouched.
 * Waits: the hull's (once per round of insertions), then one for the box
 * (MINIMAL_APPROX), two for PCA (the sums, the extents), one for the resident
 * form of the ellipsoid's loop or one per batch of iterations for the streamed
 * form (O3DMI_OBE_FORM, docs/switches.md; the resident form above its capacity
 * is O3DMI_ERR_CAPACITY). Both return with the stream drained. */
#define O3DMI_OBB_MINIMAL_APPROX 0 /* upstream's default */
#define O3DMI_OBB_PCA 1
#define O3DMI_OBB_MINIMAL_JYLANKI 2 /* O3DMI_ERR_UNSUPPORTED */
#define O3DMI_BV_TREE_RUN 8
#define O3DMI_OBE_TOLERANCE 1e-6
#define O3DMI_OBE_MAX_ITERATIONS 1000
int o3dmi_pointcloud_oriented_bounding_box(
        const void* points_dev, int64_t n, int dtype, int method,
        double center_out[3], double rotation_out[9], double extent_out[3],
        o3dmi_stream_t stream);
int o3dmi_pointcloud_oriented_bounding_ellipsoid(
        const void* points_dev, int64_t n, int dtype, double center_out[3],
        double rotation_out[9], double radii_out[3],
        int32_t* iterations_out /* may be NULL */, o3dmi_stream_t stream);

/* The host half of O3DMI_OBB_PCA, the companion of o3dmi_metrics_from_sums: no
 * device, no stream. sums = the sums of {x, y, z, xx, xy, xz, yy, yz, zz} over
 * n points. They are divided by n, mean = the first three, the covariance is
 * E[xy] - E[x] E[y] entry by entry (utility/Eigen.cpp:391-403), diagonalised
 * by this library's cyclic Jacobi iteration; the eigenvalues are put in
 * descending order by upstream's three swaps, columns 0 and 1 are normalised
 * and column 2 = column 0 x column 1. Eigen leaves the signs of columns 0 and
 * 1 undefined; here each is negated if its component of largest magnitude is
 * negative (lowest index on ties). rotation_out is row-major.
 * O3DMI_ERR_INVALID_ARG: n < 1, a NULL pointer, a sum that is not finite. */
int o3dmi_bounding_box_frame_from_moments(int64_t n, const double sums[9],
                                          double mean_out[3],
                                          double rotation_out[9]);

/* The host half of the ellipsoid: sums = {sum p x, p y, p z, p xx, p xy, p xz,
 * p yy, p yz, p zz} with weights that add up to 1. center = the first three,
 * Q = (PN - c c^T)^-1 / 3 by an L D L^T in fixed order (a pivot <= 0 or not
 * finite: O3DMI_ERR_SINGULAR), diagonalised by the same Jacobi iteration with
 * the eigenvalues in ascending order, radii = 1 / sqrt(eigenvalue), then
 * upstream's MapOBEToClosestIdentity: of the 48 signed permutations of the
 * columns the one with the largest trace, strict >, the first best wins.
 * rotation_out is row-major. O3DMI_ERR_INVALID_ARG: a NULL pointer, a sum that
 * is not finite. */
int o3dmi_bounding_ellipsoid_from_moments(const double sums[9],
                                          double center_out[3],
                                          double rotation_out[9],
                                          double radii_out[3]);

#ifdef __cplusplus
}
#endif
#endif /* O3D_MI355X_HOST_H_ */
