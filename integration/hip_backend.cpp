// The reference-side binding of libo3d_mi355x.so, COMPILED:
// the `...HIP` functions a maintainer adds next to Open3D's `...CUDA` ones --
// INTEGRATION.md sections 0-5 as one translation unit. Nothing here is
// product code and nothing here runs in the product: tests/test_integration_
// binding.py type-checks this file against
//   * the reference's OWN headers, included from where they lie under
//     /root/reference/cpp (t/geometry/kernel/VoxelBlockGrid.h,
//     t/pipelines/kernel/RegistrationImpl.h, t/geometry/kernel/Transform.h,
//     core/nns/FixedRadiusIndex.h, core/hashmap/DeviceHashBackend.h), over the
//     stand-in Tensor / TensorMap of oracle/ref_shim, and
//   * include/o3d_mi355x.h,
// and links it against the built library, so that the documented drop-in
// cannot rot: every `...HIP` function below is static_assert-ed to have the
// type of the reference's per-device function it stands beside.
//
//   g++ -std=c++17 -fsyntax-only -I integration/shim -I oracle/ref_shim \
//       -I /root/reference/cpp -I include integration/hip_backend.cpp
#include <memory>
#include <tuple>
#include <type_traits>
#include <vector>

#include "open3d/core/HIPBackend.h"
#include "open3d/core/Tensor.h"
#include "open3d/core/hashmap/DeviceHashBackend.h"
#include "open3d/core/hashmap/HashMap.h"
#include "open3d/core/nns/FixedRadiusIndex.h"
#include "open3d/core/nns/NeighborSearchCommon.h"
#include "open3d/t/geometry/kernel/PointCloud.h"
#include "open3d/t/geometry/kernel/Transform.h"
#include "open3d/t/geometry/kernel/TriangleMesh.h"
#include "open3d/t/geometry/kernel/VoxelBlockGrid.h"
#include "open3d/t/pipelines/kernel/RegistrationImpl.h"
#include "open3d/t/pipelines/registration/RobustKernel.h"
// the PointCloud smoothing drivers are whole-operator calls
#include "o3d_mi355x_host.h"

namespace open3d {

// ---------------------------------------------------------------------------
// 3. Hash map -- core/hashmap/DeviceHashBackend.cpp:18-49
//    (CreateDeviceHashBackend gains `else if (device.IsHIP()) return
//    std::make_shared<HIPHashBackend>(...)`).
// ---------------------------------------------------------------------------
namespace core {

class HIPHashBackend : public DeviceHashBackend {  // DeviceHashBackend.h:20-107
public:
    HIPHashBackend(int64_t init_capacity,
                   int64_t key_dsize,
                   const std::vector<int64_t>& value_dsizes,
                   const Device& device)
        : DeviceHashBackend(init_capacity, key_dsize, value_dsizes, device) {
        if (key_dsize != 12)
            utility::LogError("HIP backend supports Int32x3 keys");
        O3DMI_CALL(o3dmi_hash_create(init_capacity, (int)value_dsizes.size(),
                                     value_dsizes.data(), HipStream(), &h_));
    }
    ~HIPHashBackend() override { o3dmi_hash_destroy(h_); }

    void Reserve(int64_t capacity) override {
        O3DMI_CALL(o3dmi_hash_reserve(h_, capacity, HipStream()));
    }
    void Insert(const void* input_keys,
                const std::vector<const void*>& input_values_soa,
                buf_index_t* output_buf_indices,
                bool* output_masks,
                int64_t count) override {
        static_assert(sizeof(buf_index_t) == sizeof(int32_t) &&
                              sizeof(bool) == sizeof(uint8_t),
                      "the ABI's int32 indices / uint8 masks are the "
                      "reference's buf_index_t / bool");
        if (input_values_soa.empty())  // HashMap::Activate
            O3DMI_CALL(o3dmi_hash_activate(
                    h_, (const int32_t*)input_keys, count, nullptr,
                    (int32_t*)output_buf_indices, (uint8_t*)output_masks,
                    HipStream()));
        else
            O3DMI_CALL(o3dmi_hash_insert(
                    h_, (const int32_t*)input_keys, input_values_soa.data(),
                    count, (int32_t*)output_buf_indices,
                    (uint8_t*)output_masks, HipStream()));
    }
    void Find(const void* input_keys,
              buf_index_t* output_buf_indices,
              bool* output_masks,
              int64_t count) override {
        O3DMI_CALL(o3dmi_hash_find(h_, (const int32_t*)input_keys, count,
                                   nullptr, (int32_t*)output_buf_indices,
                                   (uint8_t*)output_masks, HipStream()));
    }
    void Erase(const void* input_keys,
               bool* output_masks,
               int64_t count) override {
        O3DMI_CALL(o3dmi_hash_erase(h_, (const int32_t*)input_keys, count,
                                    (uint8_t*)output_masks, HipStream()));
    }
    int64_t GetActiveIndices(buf_index_t* output_buf_indices) override {
        int64_t c = 0;
        O3DMI_CALL(o3dmi_hash_active_indices(h_, (int32_t*)output_buf_indices,
                                             HipStream(), &c));
        return c;
    }
    void Clear() override { O3DMI_CALL(o3dmi_hash_clear(h_, HipStream())); }
    int64_t Size() const override {
        int64_t s = 0;
        O3DMI_CALL(o3dmi_hash_size(h_, HipStream(), &s));
        return s;
    }
    int64_t GetBucketCount() const override {
        return o3dmi_hash_bucket_count(h_);
    }
    float LoadFactor() const override {
        return float(Size()) / float(GetBucketCount());
    }
    std::vector<int64_t> BucketSizes() const override {
        // open addressing: a "bucket" is a slot (0 or 1 entries); the
        // reference's TBB backend returns its own buckets' sizes, tests only
        // read the sum
        return std::vector<int64_t>((size_t)GetBucketCount(), 0);
    }
    // The buffers live in the o3dmi_hash_t (o3dmi_hash_key_buffer /
    // o3dmi_hash_value_buffer(i), adopted as Tensors through core::Blob with a
    // no-op deleter): nothing to allocate or free here.
    void Allocate(int64_t capacity) override { (void)capacity; }
    void Free() override {}

    o3dmi_hash_t* Handle() const { return h_; }

private:
    o3dmi_hash_t* h_ = nullptr;
};

// CreateDeviceHashBackend's HIP branch (DeviceHashBackend.cpp:18-49)
std::shared_ptr<DeviceHashBackend> CreateHIPHashBackend(
        int64_t init_capacity,
        const Dtype& key_dtype,
        const SizeVector& key_element_shape,
        const std::vector<Dtype>& value_dtypes,
        const std::vector<SizeVector>& value_element_shapes,
        const Device& device) {
    const int64_t key_dsize =
            key_dtype.ByteSize() * key_element_shape.NumElements();
    std::vector<int64_t> value_dsizes;
    for (size_t i = 0; i < value_dtypes.size(); ++i)
        value_dsizes.push_back(value_dtypes[i].ByteSize() *
                               value_element_shapes[i].NumElements());
    return std::make_shared<HIPHashBackend>(init_capacity, key_dsize,
                                            value_dsizes, device);
}

inline o3dmi_hash_t* HipHandle(const std::shared_ptr<HashMap>& hashmap) {
    auto backend = std::dynamic_pointer_cast<HIPHashBackend>(
            hashmap->GetDeviceHashBackend());
    if (!backend) utility::LogError("hash map is not on a HIP device");
    return backend->Handle();
}

}  // namespace core

// ---------------------------------------------------------------------------
// 1, 2, 4. VoxelBlockGrid kernels -- t/geometry/kernel/VoxelBlockGrid.cpp
//    dispatchers gain `else if (x.IsHIP()) { ...HIP(...); }`
// ---------------------------------------------------------------------------
namespace t {
namespace geometry {
namespace kernel {
namespace voxel_grid {

static core::Tensor HostF64(const core::Tensor& m) {
    return m.To(core::Device("CPU:0")).To(core::Float64).Contiguous();
}

// beside DepthTouchCUDA (kernel/VoxelBlockGrid.h:345-355,
// VoxelBlockGridCUDA.cu:106-227)
void DepthTouchHIP(std::shared_ptr<core::HashMap>& hashmap,
                   const core::Tensor& depth,
                   const core::Tensor& intrinsic,
                   const core::Tensor& extrinsic,
                   core::Tensor& voxel_block_coords,
                   index_t voxel_grid_resolution,
                   float voxel_size,
                   float sdf_trunc,
                   float depth_scale,
                   float depth_max,
                   index_t stride) {
    const core::Tensor K = HostF64(intrinsic), T = HostF64(extrinsic);
    const int64_t cap =
            (depth.GetShape(0) / stride) * (depth.GetShape(1) / stride) * 4;
    voxel_block_coords = core::Tensor({cap, 3}, core::Int32, depth.GetDevice());
    core::Tensor count({1}, core::Int32, depth.GetDevice());
    O3DMI_CALL(o3dmi_vbg_depth_touch(
            core::HipHandle(hashmap), depth.GetDataPtr(),
            core::ToO3dmi(depth.GetDtype()), (int)depth.GetShape(0),
            (int)depth.GetShape(1), K.GetDataPtr<double>(),
            T.GetDataPtr<double>(), voxel_block_coords.GetDataPtr<int32_t>(),
            cap, count.GetDataPtr<int32_t>(), voxel_grid_resolution, voxel_size,
            sdf_trunc, depth_scale, depth_max, stride, core::HipStream()));
    // the one synchronisation the reference also has (Item())
    const int64_t m = count.To(core::Device("CPU:0")).Item<int32_t>();
    if (m == 0)
        utility::LogError(
                "No block is touched in TSDF volume, abort integration. Please "
                "check specified parameters, especially depth_scale and "
                "voxel_size");
    voxel_block_coords = voxel_block_coords.Slice(0, 0, m);
}
static_assert(std::is_same<decltype(&DepthTouchHIP),
                           decltype(&DepthTouchCPU)>::value,
              "DepthTouchHIP has the dispatcher's per-device signature");

// beside PointCloudTouchCUDA (kernel/VoxelBlockGrid.h:338-343)
void PointCloudTouchHIP(std::shared_ptr<core::HashMap>& hashmap,
                        const core::Tensor& points,
                        core::Tensor& voxel_block_coords,
                        index_t voxel_grid_resolution,
                        float voxel_size,
                        float sdf_trunc) {
    const int64_t cap = points.GetLength() * 27;
    voxel_block_coords =
            core::Tensor({cap, 3}, core::Int32, points.GetDevice());
    core::Tensor count({1}, core::Int32, points.GetDevice());
    O3DMI_CALL(o3dmi_vbg_pointcloud_touch(
            core::HipHandle(hashmap), points.GetDataPtr<float>(),
            points.GetLength(), voxel_block_coords.GetDataPtr<int32_t>(), cap,
            count.GetDataPtr<int32_t>(), voxel_grid_resolution, voxel_size,
            sdf_trunc, core::HipStream()));
    const int64_t m = count.To(core::Device("CPU:0")).Item<int32_t>();
    voxel_block_coords = voxel_block_coords.Slice(0, 0, m);
}
static_assert(std::is_same<decltype(&PointCloudTouchHIP),
                           decltype(&PointCloudTouchCPU)>::value,
              "PointCloudTouchHIP has the dispatcher's per-device signature");

// beside IntegrateCUDA<input_depth_t, input_color_t, tsdf_t, weight_t,
// color_t> (kernel/VoxelBlockGrid.h:364-381, VoxelBlockGridImpl.h:151-308).
// Not a template: the 2 x 2 dtype dispatch (kernel/VoxelBlockGrid.cpp:107-146)
// happens inside the library.
void IntegrateHIP(const core::Tensor& depth,
                  const core::Tensor& color,
                  const core::Tensor& block_indices,
                  const core::Tensor& block_keys,
                  TensorMap& block_value_map,
                  const core::Tensor& depth_intrinsic,
                  const core::Tensor& color_intrinsic,
                  const core::Tensor& extrinsic,
                  index_t resolution,
                  float voxel_size,
                  float sdf_trunc,
                  float depth_scale,
                  float depth_max) {
    if (!block_value_map.Contains("tsdf") ||
        !block_value_map.Contains("weight"))
        utility::LogError(
                "TSDF and/or weight not allocated in blocks, please implement "
                "customized integration.");
    const bool with_color =
            block_value_map.Contains("color") && color.NumElements() > 0;
    const core::Tensor Kd = HostF64(depth_intrinsic),
                       Kc = HostF64(color_intrinsic), T = HostF64(extrinsic);
    core::Tensor w = block_value_map.at("weight");
    O3DMI_CALL(o3dmi_vbg_integrate(
            depth.GetDataPtr(), (int)depth.GetShape(0), (int)depth.GetShape(1),
            with_color ? color.GetDataPtr() : nullptr,
            with_color ? (int)color.GetShape(0) : 0,
            with_color ? (int)color.GetShape(1) : 0,
            depth.GetDtype() == core::Float32 ? O3DMI_F32 : O3DMI_U16,
            block_indices.GetDataPtr<int32_t>(), block_indices.GetLength(),
            /*n_indices_dev=*/nullptr, block_keys.GetDataPtr<int32_t>(),
            block_value_map.at("tsdf").GetDataPtr<float>(), w.GetDataPtr(),
            with_color ? block_value_map.at("color").GetDataPtr() : nullptr,
            w.GetDtype() == core::Float32 ? O3DMI_F32 : O3DMI_U16,
            Kd.GetDataPtr<double>(), Kc.GetDataPtr<double>(),
            T.GetDataPtr<double>(), resolution, voxel_size, sdf_trunc,
            depth_scale, depth_max, core::HipStream()));
}
static_assert(
        std::is_same<decltype(&IntegrateHIP),
                     decltype(&IntegrateCPU<uint16_t, uint8_t, float, uint16_t,
                                            uint16_t>)>::value,
        "IntegrateHIP takes IntegrateCPU/CUDA's arguments");

// beside EstimateRangeCUDA (kernel/VoxelBlockGrid.h:383-394)
void EstimateRangeHIP(const core::Tensor& block_keys,
                      core::Tensor& range_minmax_map,
                      const core::Tensor& intrinsics,
                      const core::Tensor& extrinsics,
                      int h,
                      int w,
                      int down_factor,
                      int64_t block_resolution,
                      float voxel_size,
                      float depth_min,
                      float depth_max,
                      core::Tensor& fragment_buffer) {
    (void)fragment_buffer;  // no fragment stage on this backend
    const core::Tensor K = HostF64(intrinsics), T = HostF64(extrinsics);
    range_minmax_map = core::Tensor({h / down_factor, w / down_factor, 2},
                                    core::Float32, block_keys.GetDevice());
    O3DMI_CALL(o3dmi_vbg_estimate_range(
            block_keys.GetDataPtr<int32_t>(), block_keys.GetLength(),
            range_minmax_map.GetDataPtr<float>(), K.GetDataPtr<double>(),
            T.GetDataPtr<double>(), h, w, down_factor, block_resolution,
            voxel_size, depth_min, depth_max, core::HipStream()));
}
static_assert(std::is_same<decltype(&EstimateRangeHIP),
                           decltype(&EstimateRangeCPU)>::value,
              "EstimateRangeHIP has the dispatcher's per-device signature");

// beside RayCastCUDA<tsdf_t, weight_t, color_t> (kernel/VoxelBlockGrid.h:
// 396-413, VoxelBlockGridImpl.h:578-1120); dtype dispatch inside the library
void RayCastHIP(std::shared_ptr<core::HashMap>& hashmap,
                const TensorMap& block_value_map,
                const core::Tensor& range_map,
                TensorMap& renderings_map,
                const core::Tensor& intrinsic,
                const core::Tensor& extrinsic,
                index_t h,
                index_t w,
                index_t block_resolution,
                float voxel_size,
                float depth_scale,
                float depth_min,
                float depth_max,
                float weight_threshold,
                float trunc_voxel_multiplier,
                int range_map_down_factor) {
    const core::Tensor K = HostF64(intrinsic), T = HostF64(extrinsic);
    auto P = [&](const char* n) -> void* {  // NULL: map not requested
        return renderings_map.Contains(n) ? renderings_map.at(n).GetDataPtr()
                                          : nullptr;
    };
    const core::Tensor& weight = block_value_map.at("weight");
    O3DMI_CALL(o3dmi_vbg_raycast(
            core::HipHandle(hashmap),
            block_value_map.at("tsdf").GetDataPtr<float>(),
            weight.GetDataPtr(),
            block_value_map.Contains("color")
                    ? block_value_map.at("color").GetDataPtr()
                    : nullptr,
            weight.GetDtype() == core::Float32 ? O3DMI_F32 : O3DMI_U16,
            range_map.GetDataPtr<float>(), (float*)P("depth"),
            (float*)P("vertex"), (float*)P("color"), (float*)P("normal"),
            (int64_t*)P("index"), (uint8_t*)P("mask"),
            (float*)P("interp_ratio"), (float*)P("interp_ratio_dx"),
            (float*)P("interp_ratio_dy"), (float*)P("interp_ratio_dz"),
            K.GetDataPtr<double>(), T.GetDataPtr<double>(), h, w,
            block_resolution, voxel_size, depth_scale, depth_min, depth_max,
            weight_threshold, trunc_voxel_multiplier, range_map_down_factor,
            core::HipStream()));
}
static_assert(
        std::is_same<decltype(&RayCastHIP),
                     decltype(&RayCastCPU<float, uint16_t, uint16_t>)>::value,
        "RayCastHIP takes RayCastCPU/CUDA's arguments");

}  // namespace voxel_grid

// 5. beside TransformPointsCUDA / TransformNormalsCUDA
//    (t/geometry/kernel/Transform.h:42-47)
namespace transform {
void TransformPointsHIP(const core::Tensor& transformation,
                        core::Tensor& points) {
    const core::Tensor T = transformation.To(core::Device("CPU:0"))
                                   .To(core::Float64)
                                   .Contiguous();
    O3DMI_CALL(o3dmi_transform_points(T.GetDataPtr<double>(),
                                      points.GetDataPtr(), points.GetLength(),
                                      core::ToO3dmi(points.GetDtype()),
                                      core::HipStream()));
}
void TransformNormalsHIP(const core::Tensor& transformation,
                         core::Tensor& normals) {
    const core::Tensor T = transformation.To(core::Device("CPU:0"))
                                   .To(core::Float64)
                                   .Contiguous();
    O3DMI_CALL(o3dmi_transform_normals(T.GetDataPtr<double>(),
                                       normals.GetDataPtr(),
                                       normals.GetLength(),
                                       core::ToO3dmi(normals.GetDtype()),
                                       core::HipStream()));
}
static_assert(std::is_same<decltype(&TransformPointsHIP),
                           decltype(&TransformPointsCPU)>::value &&
                      std::is_same<decltype(&TransformNormalsHIP),
                                   decltype(&TransformNormalsCPU)>::value,
              "Transform*HIP have the dispatcher's per-device signature");
}  // namespace transform

// 5e''. beside SmoothLaplacianCUDA ... OrientNormalsTowardsCameraLocationCUDA
//    (t/geometry/kernel/PointCloud.h:96-110, 329-357; the dispatchers in
//    t/geometry/PointCloud.cpp:762-854, 986-1050, 1074-1203 gain
//    `else if (IsHIP()) { kernel::pointcloud::...HIP(...); }`)
namespace pointcloud {
namespace {
// {3} reference vector on the host in float64 (the library converts it to
// the point dtype, as upstream's reference.To(dtype) does)
core::Tensor HostVec3(const core::Tensor& v) {
    return v.To(core::Device("CPU:0")).To(core::Float64).Contiguous();
}
}  // namespace

void SmoothLaplacianHIP(const core::Tensor& points,
                        core::Tensor& smoothed_points,
                        size_t iterations,
                        double lambda,
                        int max_nn,
                        bool use_fixed_neighborhoods) {
    smoothed_points = core::Tensor::Empty(points.GetShape(), points.GetDtype(),
                                          points.GetDevice());
    O3DMI_CALL(o3dmi_pointcloud_smooth_laplacian(
            points.GetDataPtr(), points.GetLength(),
            core::ToO3dmi(points.GetDtype()), (int64_t)iterations, lambda,
            max_nn, use_fixed_neighborhoods ? 1 : 0,
            smoothed_points.GetDataPtr(), core::HipStream()));
}
void SmoothTaubinHIP(const core::Tensor& points,
                     core::Tensor& smoothed_points,
                     size_t iterations,
                     double lambda,
                     double mu,
                     int max_nn,
                     bool use_fixed_neighborhoods) {
    smoothed_points = core::Tensor::Empty(points.GetShape(), points.GetDtype(),
                                          points.GetDevice());
    O3DMI_CALL(o3dmi_pointcloud_smooth_taubin(
            points.GetDataPtr(), points.GetLength(),
            core::ToO3dmi(points.GetDtype()), (int64_t)iterations, lambda, mu,
            max_nn, use_fixed_neighborhoods ? 1 : 0,
            smoothed_points.GetDataPtr(), core::HipStream()));
}
void SmoothMLSHIP(const core::Tensor& points,
                  core::Tensor& smoothed_points,
                  core::Tensor& normals,
                  bool update_normals,
                  double radius,
                  int max_nn) {
    smoothed_points = core::Tensor::Empty(points.GetShape(), points.GetDtype(),
                                          points.GetDevice());
    // upstream updates `normals` in place; the library reads one buffer and
    // writes another
    core::Tensor incoming;
    if (update_normals) incoming = normals.Clone();
    O3DMI_CALL(o3dmi_pointcloud_smooth_mls(
            points.GetDataPtr(),
            update_normals ? incoming.GetDataPtr() : nullptr,
            points.GetLength(), core::ToO3dmi(points.GetDtype()), radius,
            max_nn, smoothed_points.GetDataPtr(),
            update_normals ? normals.GetDataPtr() : nullptr,
            core::HipStream()));
}
void SmoothBilateralHIP(const core::Tensor& points,
                        const core::Tensor& normals,
                        core::Tensor& smoothed_points,
                        double radius,
                        int max_nn,
                        double sigma_s,
                        double sigma_r) {
    smoothed_points = core::Tensor::Empty(points.GetShape(), points.GetDtype(),
                                          points.GetDevice());
    O3DMI_CALL(o3dmi_pointcloud_smooth_bilateral(
            points.GetDataPtr(), normals.GetDataPtr(), points.GetLength(),
            core::ToO3dmi(points.GetDtype()), radius, max_nn, sigma_s, sigma_r,
            smoothed_points.GetDataPtr(), core::HipStream()));
}
void ComputeBoundaryPointsHIP(const core::Tensor& points,
                              const core::Tensor& normals,
                              const core::Tensor& indices,
                              const core::Tensor& counts,
                              core::Tensor& mask,
                              double angle_threshold) {
    O3DMI_CALL(o3dmi_pointcloud_boundary_from_neighbors(
            points.GetDataPtr(), normals.GetDataPtr(),
            (const int32_t*)indices.GetDataPtr(),
            (const int32_t*)counts.GetDataPtr(), points.GetLength(),
            (int)indices.GetShape(1), core::ToO3dmi(points.GetDtype()),
            angle_threshold, (uint8_t*)mask.GetDataPtr(), core::HipStream()));
}
void NormalizeNormalsHIP(core::Tensor& normals) {
    O3DMI_CALL(o3dmi_pointcloud_normalize_normals(
            normals.GetDataPtr(), normals.GetLength(),
            core::ToO3dmi(normals.GetDtype()), core::HipStream()));
}
void OrientNormalsToAlignWithDirectionHIP(core::Tensor& normals,
                                          const core::Tensor& direction) {
    const core::Tensor d = HostVec3(direction);
    O3DMI_CALL(o3dmi_pointcloud_orient_normals_to_align_with_direction(
            normals.GetDataPtr(), normals.GetLength(),
            core::ToO3dmi(normals.GetDtype()), d.GetDataPtr<double>(),
            core::HipStream()));
}
void OrientNormalsTowardsCameraLocationHIP(const core::Tensor& points,
                                           core::Tensor& normals,
                                           const core::Tensor& camera) {
    const core::Tensor c = HostVec3(camera);
    O3DMI_CALL(o3dmi_pointcloud_orient_normals_towards_camera_location(
            points.GetDataPtr(), normals.GetDataPtr(), normals.GetLength(),
            core::ToO3dmi(points.GetDtype()), c.GetDataPtr<double>(),
            core::HipStream()));
}
static_assert(
        std::is_same<decltype(&SmoothLaplacianHIP),
                     decltype(&SmoothLaplacianCPU)>::value &&
                std::is_same<decltype(&SmoothTaubinHIP),
                             decltype(&SmoothTaubinCPU)>::value &&
                std::is_same<decltype(&SmoothMLSHIP),
                             decltype(&SmoothMLSCPU)>::value &&
                std::is_same<decltype(&SmoothBilateralHIP),
                             decltype(&SmoothBilateralCPU)>::value &&
                std::is_same<decltype(&ComputeBoundaryPointsHIP),
                             decltype(&ComputeBoundaryPointsCPU)>::value &&
                std::is_same<decltype(&NormalizeNormalsHIP),
                             decltype(&NormalizeNormalsCPU)>::value &&
                std::is_same<
                        decltype(&OrientNormalsToAlignWithDirectionHIP),
                        decltype(&OrientNormalsToAlignWithDirectionCPU)>::
                        value &&
                std::is_same<
                        decltype(&OrientNormalsTowardsCameraLocationHIP),
                        decltype(&OrientNormalsTowardsCameraLocationCPU)>::
                        value,
        "the PointCloud smoothing / boundary / normal ...HIP functions have "
        "the dispatchers' per-device signatures");

// 5e'''''. PointCloud::ComputeMetrics (t/geometry/PointCloud.cpp:1805-1836)
//    has no per-device kernel upstream: the method copies both clouds to the
//    host and searches two k-d trees. It gains, before those copies,
//    `if (IsHIP() && pcd2.IsHIP()) return kernel::pointcloud::ComputeMetricsHIP(
//    GetPointPositions(), pcd2.GetPointPositions(), codes,
//    params.fscore_radius);` with codes[i] = static_cast<int32_t>(metrics[i])
//    (the library's codes are upstream's enum order). The result is a host
//    Float32 tensor, as upstream's.
core::Tensor ComputeMetricsHIP(const core::Tensor& points1,
                               const core::Tensor& points2,
                               const std::vector<int32_t>& metrics,
                               const std::vector<float>& fscore_radius) {
    int64_t n_values = 0;
    for (int32_t m : metrics)
        n_values += m == O3DMI_METRIC_FSCORE ? (int64_t)fscore_radius.size()
                                             : 1;
    std::vector<float> values((size_t)n_values);
    O3DMI_CALL(o3dmi_pointcloud_compute_metrics(
            points1.GetDataPtr(), points1.GetLength(), points2.GetDataPtr(),
            points2.GetLength(), core::ToO3dmi(points1.GetDtype()),
            metrics.data(), (int)metrics.size(), fscore_radius.data(),
            (int)fscore_radius.size(), values.data(), n_values, nullptr,
            core::HipStream()));
    return core::Tensor(values, {n_values}, core::Float32);
}
}  // namespace pointcloud

// 5e. beside NormalizeNormalsCUDA ... ComputeTriangleAreasCUDA
//    (t/geometry/kernel/TriangleMesh.h:60-73; the dispatchers in
//    t/geometry/TriangleMesh.cpp:198-360 gain `else if (IsHIP()) {
//    kernel::trianglemesh::...HIP(...); }`). The outputs are the tensors the
//    dispatchers allocate; ComputeVertexNormals' arrives zeroed and is
//    overwritten with the sum of upstream's CPU loop.
namespace trianglemesh {
void NormalizeNormalsHIP(core::Tensor& normals) {
    O3DMI_CALL(o3dmi_trianglemesh_normalize_normals(
            normals.GetDataPtr(), normals.GetLength(),
            core::ToO3dmi(normals.GetDtype()), core::HipStream()));
}
void ComputeTriangleNormalsHIP(const core::Tensor& vertices,
                               const core::Tensor& triangles,
                               core::Tensor& normals) {
    O3DMI_CALL(o3dmi_trianglemesh_compute_triangle_normals(
            vertices.GetDataPtr(), vertices.GetLength(),
            core::ToO3dmi(normals.GetDtype()), triangles.GetDataPtr(),
            triangles.GetLength(), core::ToO3dmi(triangles.GetDtype()),
            normals.GetDataPtr(), core::HipStream()));
}
void ComputeVertexNormalsHIP(const core::Tensor& triangles,
                             const core::Tensor& triangle_normals,
                             core::Tensor& vertex_normals) {
    O3DMI_CALL(o3dmi_trianglemesh_compute_vertex_normals(
            triangles.GetDataPtr(), triangles.GetLength(),
            core::ToO3dmi(triangles.GetDtype()), triangle_normals.GetDataPtr(),
            core::ToO3dmi(vertex_normals.GetDtype()),
            vertex_normals.GetLength(), vertex_normals.GetDataPtr(),
            core::HipStream()));
}
void ComputeTriangleAreasHIP(const core::Tensor& vertices,
                             const core::Tensor& triangles,
                             core::Tensor& triangle_areas) {
    O3DMI_CALL(o3dmi_trianglemesh_compute_triangle_areas(
            vertices.GetDataPtr(), vertices.GetLength(),
            core::ToO3dmi(triangle_areas.GetDtype()), triangles.GetDataPtr(),
            triangles.GetLength(), core::ToO3dmi(triangles.GetDtype()),
            triangle_areas.GetDataPtr(), core::HipStream()));
}
static_assert(
        std::is_same<decltype(&NormalizeNormalsHIP),
                     decltype(&NormalizeNormalsCPU)>::value &&
                std::is_same<decltype(&ComputeTriangleNormalsHIP),
                             decltype(&ComputeTriangleNormalsCPU)>::value &&
                std::is_same<decltype(&ComputeVertexNormalsHIP),
                             decltype(&ComputeVertexNormalsCPU)>::value &&
                std::is_same<decltype(&ComputeTriangleAreasHIP),
                             decltype(&ComputeTriangleAreasCPU)>::value,
        "the TriangleMesh ...HIP functions have the dispatchers' per-device "
        "signatures");

// 5e (continued). TriangleMesh::SamplePointsUniformly (t/geometry/
//    TriangleMesh.cpp:1866-1937), RaycastingScene::ComputeClosestPoints /
//    ComputeDistance for one triangle geometry (RaycastingScene.cpp:
//    1464-1517) and TriangleMesh::ComputeMetrics (:1939-1967) have no
//    per-device kernel upstream: each copies to the host first. Each gains a
//    HIP branch in front of those copies (INTEGRATION 5e''''''). `seed` is
//    drawn once per call from utility::random.
//    points / normals / colors: the tensors the method allocates ({n,3};
//    normals and colors may be empty), vertex_normals / triangle_normals /
//    vertex_colors the inputs SamplePointsUniformly selects (empty: unused).
void SamplePointsUniformlyHIP(const core::Tensor& triangles,
                              const core::Tensor& vertices,
                              const core::Tensor& vertex_normals,
                              const core::Tensor& vertex_colors,
                              const core::Tensor& triangle_normals,
                              uint64_t seed, core::Tensor& points,
                              core::Tensor& normals, core::Tensor& colors) {
    auto ptr = [](const core::Tensor& t) -> const void* {
        return t.NumElements() > 0 ? t.GetDataPtr() : nullptr;
    };
    O3DMI_CALL(o3dmi_trianglemesh_sample_points_uniformly(
            vertices.GetDataPtr(), vertices.GetLength(),
            core::ToO3dmi(vertices.GetDtype()), triangles.GetDataPtr(),
            triangles.GetLength(), core::ToO3dmi(triangles.GetDtype()),
            points.GetLength(), seed, ptr(vertex_normals),
            ptr(triangle_normals), ptr(vertex_colors),
            vertex_colors.NumElements() > 0
                    ? core::ToO3dmi(vertex_colors.GetDtype())
                    : O3DMI_F32,
            points.GetDataPtr(),
            normals.NumElements() > 0 ? normals.GetDataPtr() : nullptr,
            colors.NumElements() > 0 ? colors.GetDataPtr<float>() : nullptr,
            nullptr, core::HipStream()));
}

//    RaycastingScene::Impl keeps the handle: AddTriangles creates it,
//    the destructor destroys it.
o3dmi_mesh_bvh_t* MeshBvhCreateHIP(const core::Tensor& vertices,
                                   const core::Tensor& triangles) {
    o3dmi_mesh_bvh_t* bvh = nullptr;
    O3DMI_CALL(o3dmi_mesh_bvh_create(
            vertices.GetDataPtr(), vertices.GetLength(),
            core::ToO3dmi(vertices.GetDtype()), triangles.GetDataPtr(),
            triangles.GetLength(), core::ToO3dmi(triangles.GetDtype()), &bvh,
            core::HipStream()));
    return bvh;
}
void MeshBvhDestroyHIP(o3dmi_mesh_bvh_t* bvh) {
    O3DMI_CALL(o3dmi_mesh_bvh_destroy(bvh));
}
//    query_points {..,3} Float32, contiguous; every output has its leading
//    dimensions and may be empty (ComputeDistance passes `distance` alone).
void MeshClosestPointsHIP(const o3dmi_mesh_bvh_t* bvh,
                          const core::Tensor& query_points,
                          core::Tensor& points, core::Tensor& primitive_ids,
                          core::Tensor& primitive_uvs,
                          core::Tensor& primitive_normals,
                          core::Tensor& distance) {
    auto ptr = [](core::Tensor& t) -> void* {
        return t.NumElements() > 0 ? t.GetDataPtr() : nullptr;
    };
    O3DMI_CALL(o3dmi_mesh_bvh_closest_points(
            bvh, query_points.GetDataPtr(), query_points.NumElements() / 3,
            core::ToO3dmi(query_points.GetDtype()), ptr(points),
            (uint32_t*)ptr(primitive_ids), ptr(primitive_uvs),
            ptr(primitive_normals), ptr(distance), core::HipStream()));
}

//    codes[i] = static_cast<int32_t>(metrics[i]); the result is a host
//    Float32 tensor, as upstream's.
core::Tensor ComputeMetricsHIP(const core::Tensor& vertices1,
                               const core::Tensor& triangles1,
                               const core::Tensor& vertices2,
                               const core::Tensor& triangles2,
                               const std::vector<int32_t>& metrics,
                               const std::vector<float>& fscore_radius,
                               int64_t n_sampled_points, uint64_t seed) {
    int64_t n_values = 0;
    for (int32_t m : metrics)
        n_values += m == O3DMI_METRIC_FSCORE ? (int64_t)fscore_radius.size()
                                             : 1;
    std::vector<float> values((size_t)n_values);
    O3DMI_CALL(o3dmi_trianglemesh_compute_metrics(
            vertices1.GetDataPtr(), vertices1.GetLength(),
            triangles1.GetDataPtr(), triangles1.GetLength(),
            core::ToO3dmi(triangles1.GetDtype()), vertices2.GetDataPtr(),
            vertices2.GetLength(), triangles2.GetDataPtr(),
            triangles2.GetLength(), core::ToO3dmi(triangles2.GetDtype()),
            core::ToO3dmi(vertices1.GetDtype()), metrics.data(),
            (int)metrics.size(), fscore_radius.data(),
            (int)fscore_radius.size(), n_sampled_points, seed, values.data(),
            n_values, nullptr, core::HipStream()));
    return core::Tensor(values, {n_values}, core::Float32);
}
}  // namespace trianglemesh
}  // namespace kernel
}  // namespace geometry

// ---------------------------------------------------------------------------
// 5. ICP -- t/pipelines/kernel/Registration.cpp:35-78 (ComputePosePointToPlane
//    dispatcher) gains `else if (source_points.IsHIP())`
// ---------------------------------------------------------------------------
namespace pipelines {
namespace kernel {

// beside ComputePosePointToPlaneCUDA (RegistrationImpl.h:93-102,
// RegistrationCUDA.cu:81-117)
void ComputePosePointToPlaneHIP(const core::Tensor& source_points,
                                const core::Tensor& target_points,
                                const core::Tensor& target_normals,
                                const core::Tensor& correspondence_indices,
                                core::Tensor& pose,
                                float& residual,
                                int& inlier_count,
                                const core::Dtype& dtype,
                                const core::Device& device,
                                const registration::RobustKernel& kernel) {
    core::Tensor sums = core::Tensor::Empty({29}, core::Float64, device);
    O3DMI_CALL(o3dmi_icp_p2plane_accumulate(
            source_points.Contiguous().GetDataPtr(),
            target_points.Contiguous().GetDataPtr(),
            target_normals.Contiguous().GetDataPtr(),
            correspondence_indices.Contiguous().GetDataPtr<int64_t>(),
            source_points.GetLength(), core::ToO3dmi(dtype), (int)kernel.type_,
            kernel.scaling_parameter_, kernel.shape_parameter_,
            sums.GetDataPtr<double>(), core::HipStream()));
    // the one device-to-host copy of the iteration; DecodeAndSolve6x6
    // (TransformationConverter.cpp:189-226) on the host copy
    const core::Tensor host = sums.To(core::Device("CPU:0"));
    pose = core::Tensor::Empty({6}, core::Float64, core::Device("CPU:0"));
    O3DMI_CALL(o3dmi_decode_and_solve6x6(host.GetDataPtr<double>(),
                                         pose.GetDataPtr<double>(), &residual,
                                         &inlier_count));
}
static_assert(std::is_same<decltype(&ComputePosePointToPlaneHIP),
                           decltype(&ComputePosePointToPlaneCPU)>::value,
              "ComputePosePointToPlaneHIP has the dispatcher's per-device "
              "signature");


// beside ComputePoseDopplerICPCUDA (RegistrationImpl.h:69-90,
// RegistrationCUDA.cu): the small tensors the dispatcher prepared in the point
// dtype go over as host float64
void ComputePoseDopplerICPHIP(const core::Tensor& source_points,
                              const core::Tensor& source_dopplers,
                              const core::Tensor& source_directions,
                              const core::Tensor& target_points,
                              const core::Tensor& target_normals,
                              const core::Tensor& correspondence_indices,
                              core::Tensor& output_pose,
                              float& residual,
                              int& inlier_count,
                              const core::Dtype& dtype,
                              const core::Device& device,
                              const core::Tensor& R_S_to_V,
                              const core::Tensor& r_v_to_s_in_V,
                              const core::Tensor& w_v_in_V,
                              const core::Tensor& v_v_in_V,
                              const double period,
                              const bool reject_dynamic_outliers,
                              const double doppler_outlier_threshold,
                              const registration::RobustKernel& kernel_geometric,
                              const registration::RobustKernel& kernel_doppler,
                              const double lambda_doppler) {
    const core::Device cpu("CPU:0");
    const core::Tensor R = R_S_to_V.To(cpu, core::Float64).Contiguous();
    const core::Tensor r = r_v_to_s_in_V.To(cpu, core::Float64).Contiguous();
    const core::Tensor w = w_v_in_V.To(cpu, core::Float64).Contiguous();
    const core::Tensor v = v_v_in_V.To(cpu, core::Float64).Contiguous();
    core::Tensor sums = core::Tensor::Empty({29}, core::Float64, device);
    O3DMI_CALL(o3dmi_icp_doppler_accumulate(
            source_points.Contiguous().GetDataPtr(),
            source_dopplers.Contiguous().GetDataPtr(),
            source_directions.Contiguous().GetDataPtr(),
            target_points.Contiguous().GetDataPtr(),
            target_normals.Contiguous().GetDataPtr(),
            correspondence_indices.Contiguous().GetDataPtr<int64_t>(),
            source_points.GetLength(), target_points.GetLength(),
            core::ToO3dmi(dtype), R.GetDataPtr<double>(),
            r.GetDataPtr<double>(), w.GetDataPtr<double>(),
            v.GetDataPtr<double>(), period, reject_dynamic_outliers ? 1 : 0,
            doppler_outlier_threshold, (int)kernel_geometric.type_,
            kernel_geometric.scaling_parameter_,
            kernel_geometric.shape_parameter_, (int)kernel_doppler.type_,
            kernel_doppler.scaling_parameter_, kernel_doppler.shape_parameter_,
            lambda_doppler, sums.GetDataPtr<double>(), core::HipStream()));
    const core::Tensor host = sums.To(cpu);
    output_pose = core::Tensor::Empty({6}, core::Float64, cpu);
    O3DMI_CALL(o3dmi_decode_and_solve6x6(host.GetDataPtr<double>(),
                                         output_pose.GetDataPtr<double>(),
                                         &residual, &inlier_count));
}
static_assert(std::is_same<decltype(&ComputePoseDopplerICPHIP),
                           decltype(&ComputePoseDopplerICPCPU)>::value,
              "ComputePoseDopplerICPHIP has the dispatcher's per-device "
              "signature");

}  // namespace kernel
}  // namespace pipelines
}  // namespace t

// ---------------------------------------------------------------------------
// 5. Neighbour search -- core/nns/FixedRadiusIndex.cpp:58-136 (SetTensorData)
//    and :229-299 (SearchHybrid). The reference builds a CSR hash table
//    (BuildSpatialHashTableCUDA<T>) and hands its tensors to
//    HybridSearchCUDA<T, TIndex> (FixedRadiusIndex.h:227-233,364-377); this
//    backend's index is an opaque handle built once per SetTensorData, so the
//    HIP branches of the two members replace the pair of calls.
// ---------------------------------------------------------------------------
namespace core {
namespace nns {

struct HIPFixedRadiusIndex {
    o3dmi_nns_t* handle = nullptr;
    Tensor dataset_points;  // kept alive: the build is stream-ordered
    ~HIPFixedRadiusIndex() {
        if (handle) o3dmi_nns_destroy(handle);
    }

    // FixedRadiusIndex::SetTensorData, HIP branch
    bool SetTensorData(const Tensor& points, double radius) {
        if (handle) o3dmi_nns_destroy(handle);
        handle = nullptr;
        dataset_points = points.Contiguous();
        O3DMI_CALL(o3dmi_nns_create(dataset_points.GetDataPtr(),
                                    dataset_points.GetLength(),
                                    ToO3dmi(dataset_points.GetDtype()), radius,
                                    HipStream(), &handle));
        return true;
    }

    // FixedRadiusIndex::SearchHybrid, HIP branch: {indices {Q,max_knn},
    // distances {Q,max_knn}, counts {Q}} -- NNSIndex::SearchHybrid's tuple
    std::tuple<Tensor, Tensor, Tensor> SearchHybrid(const Tensor& query_points,
                                                    double radius,
                                                    int max_knn) const {
        (void)radius;  // fixed at SetTensorData, as FixedRadiusIndex checks
        const Tensor q = query_points.Contiguous();
        const int64_t n = q.GetLength();
        Tensor indices = Tensor::Empty({n, max_knn}, Int32, q.GetDevice());
        Tensor distances =
                Tensor::Empty({n, max_knn}, q.GetDtype(), q.GetDevice());
        Tensor counts = Tensor::Empty({n}, Int32, q.GetDevice());
        if (max_knn == 1)
            O3DMI_CALL(o3dmi_nns_hybrid_search_k1(
                    handle, q.GetDataPtr(), n, indices.GetDataPtr<int32_t>(),
                    distances.GetDataPtr(), counts.GetDataPtr<int32_t>(),
                    HipStream()));
        else
            O3DMI_CALL(o3dmi_nns_hybrid_search(
                    handle, q.GetDataPtr(), n, max_knn,
                    indices.GetDataPtr<int32_t>(), distances.GetDataPtr(),
                    counts.GetDataPtr<int32_t>(), HipStream()));
        return std::make_tuple(indices, distances, counts);
    }
};

// The seam-level form for a caller that keeps the reference's two free
// functions: the build output tensors stay empty (the handle carries the
// index), the search ignores them.
template <class T>
void BuildSpatialHashTableHIP(const Tensor& points,
                              double radius,
                              const Tensor& points_row_splits,
                              const Tensor& hash_table_splits,
                              Tensor& hash_table_index,
                              Tensor& hash_table_cell_splits,
                              HIPFixedRadiusIndex& index) {
    (void)points_row_splits;
    (void)hash_table_splits;
    (void)hash_table_index;
    (void)hash_table_cell_splits;
    index.SetTensorData(points, radius);
}

template <class T, class TIndex>
void HybridSearchHIP(const Tensor& points,
                     const Tensor& queries,
                     double radius,
                     int max_knn,
                     const Tensor& points_row_splits,
                     const Tensor& queries_row_splits,
                     const Tensor& hash_table_splits,
                     const Tensor& hash_table_index,
                     const Tensor& hash_table_cell_splits,
                     const Metric metric,
                     Tensor& neighbors_index,
                     Tensor& neighbors_count,
                     Tensor& neighbors_distance,
                     const HIPFixedRadiusIndex& index) {
    static_assert(std::is_same<TIndex, int32_t>::value,
                  "the ABI returns Int32 indices (NearestNeighborSearch's "
                  "default index dtype; the ICP driver casts to Int64)");
    (void)points;
    (void)points_row_splits;
    (void)queries_row_splits;
    (void)hash_table_splits;
    (void)hash_table_index;
    (void)hash_table_cell_splits;
    if (metric != L2) utility::LogError("HIP hybrid search: L2 metric only");
    std::tie(neighbors_index, neighbors_distance, neighbors_count) =
            index.SearchHybrid(queries, radius, max_knn);
}
template void BuildSpatialHashTableHIP<float>(const Tensor&, double,
                                              const Tensor&, const Tensor&,
                                              Tensor&, Tensor&,
                                              HIPFixedRadiusIndex&);
template void HybridSearchHIP<float, int32_t>(
        const Tensor&, const Tensor&, double, int, const Tensor&,
        const Tensor&, const Tensor&, const Tensor&, const Tensor&,
        const Metric, Tensor&, Tensor&, Tensor&, const HIPFixedRadiusIndex&);

}  // namespace nns
}  // namespace core
}  // namespace open3d
