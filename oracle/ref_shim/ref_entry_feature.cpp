// TEST INFRASTRUCTURE ONLY.
//
// C entry points over the reference's FPFH kernel file, compiled from where
// it lies (see README.md in this directory). A translation unit of its own,
// with FeatureCPU.cpp FIRST, as the reference builds it: ComputePairFeature
// calls acos / fabs / atan2 / sqrt / floor unqualified, and which overload
// that is depends on what has been declared before it. With only <cmath> in
// scope they are the C functions of double, whatever the point dtype; after a
// header that includes <math.h> (core/linalg/kernel/SVD3x3.h does) they are
// the overloads of float. ref_fpfh_float_math_is_float() reports which.

// The reference translation unit, unmodified.
#include "open3d/t/pipelines/kernel/FeatureCPU.cpp"

namespace open3d {
namespace t {
namespace pipelines {
namespace kernel {
// Evaluated where ComputePairFeature's body was parsed.
static const bool kAcosOfFloatIsFloat =
        std::is_same<decltype(acos(1.0f)), float>::value;
}  // namespace kernel
}  // namespace pipelines
}  // namespace t
}  // namespace open3d

#include <cstdint>
#include <exception>
#include <optional>
#include <vector>

using namespace open3d;
using core::Tensor;
namespace pk = open3d::t::pipelines::kernel;

extern "C" void ref_set_last_error(const char* what);

namespace {
Tensor Wrap(const void* p, core::SizeVector shape, core::Dtype dt) {
    return Tensor::FromPtr(p, shape, dt);
}
template <typename F>
int Guard(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        ref_set_last_error(e.what());
        return 1;
    }
}
}  // namespace

extern "C" {

int ref_fpfh_float_math_is_float() { return pk::kAcosOfFloatIsFloat ? 1 : 0; }

// ComputePairFeature, t/pipelines/kernel/FeatureImpl.h:24-85: feature {4}.
int ref_fpfh_pair_feature(const void* p1, const void* n1, const void* p2,
                          const void* n2, int is_f64, void* feature4) {
    return Guard([&] {
        if (is_f64)
            pk::ComputePairFeature<double>((const double*)p1, (const double*)n1,
                                           (const double*)p2, (const double*)n2,
                                           (double*)feature4);
        else
            pk::ComputePairFeature<float>((const float*)p1, (const float*)n1,
                                          (const float*)p2, (const float*)n2,
                                          (float*)feature4);
    });
}

// ComputeFPFHFeatureCPU, FeatureImpl.h:107-295. Padded lists: indices /
// distance2 {n_rows, max_nn} with counts {n_rows}; CSR lists (row_splits
// {n_rows + 1} given, counts NULL): indices / distance2 {row_splits[n_rows]},
// the splits narrowed to the Int32 prefix sums the body reads. mask (uint8
// {n_points}) and map {n_rows} are both given or both NULL. The body ADDS into
// fpfhs {n_fpfh, 33}: the caller passes what it wants added to (zeros).
int ref_fpfh_from_neighbors(const void* points, const void* normals,
                            int64_t n_points, int is_f64,
                            const int32_t* indices, const void* distance2,
                            const int32_t* counts, const int64_t* row_splits,
                            int max_nn, int64_t n_rows, const uint8_t* mask,
                            const int64_t* map_info_idx_to_point_idx,
                            void* fpfhs, int64_t n_fpfh) {
    return Guard([&] {
        const core::Dtype dt = is_f64 ? core::Float64 : core::Float32;
        Tensor pts = Wrap(points, {n_points, 3}, dt);
        Tensor nrm = Wrap(normals, {n_points, 3}, dt);
        Tensor idx, d2, cnt;
        std::vector<int32_t> prefix;
        if (row_splits) {
            prefix.assign(row_splits, row_splits + n_rows + 1);
            const int64_t total = row_splits[n_rows];
            idx = Wrap(indices, {total}, core::Int32);
            d2 = Wrap(distance2, {total}, dt);
            cnt = Wrap(prefix.data(), {n_rows + 1}, core::Int32);
        } else {
            idx = Wrap(indices, {n_rows, (int64_t)max_nn}, core::Int32);
            d2 = Wrap(distance2, {n_rows, (int64_t)max_nn}, dt);
            cnt = Wrap(counts, {n_rows}, core::Int32);
        }
        Tensor out = Wrap(fpfhs, {n_fpfh, 33}, dt);
        std::optional<Tensor> m = std::nullopt, mp = std::nullopt;
        if (mask) m = Wrap(mask, {n_points}, core::Bool);
        if (map_info_idx_to_point_idx)
            mp = Wrap(map_info_idx_to_point_idx, {n_rows}, core::Int64);
        pk::ComputeFPFHFeatureCPU(pts, nrm, idx, d2, cnt, out, m, mp);
    });
}

}  // extern "C"
