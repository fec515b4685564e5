// slac::ControlGrid (t/pipelines/slac/ControlGrid.{h,cpp}) over the kernels of
// control_grid.hip: the node map is an o3dmi_hash_t with one value buffer,
// the nodes' current positions.
//
// Touch feeds the insert from the kernel and grows the map the way the frame
// stream does (RecoverOverflow, Reserve, replay); Parameterize is flags ->
// scan -> write, so the survivors keep the input order; the image forms of
// Deform go pixel -> packed word -> pixel and never build the cloud.
#include <algorithm>
#include <array>
#include <vector>

#include "common.h"
#include "control_grid.h"
#include "o3d_mi355x_host.h"
#include "scan.h"
#include "stream_path.h"

using namespace o3dmi;

struct o3dmi_control_grid {
    float grid_size = 0;
    o3dmi_hash_t* hash = nullptr;
    int anchor_idx = -1;
};

namespace {

int NewGrid(float grid_size, int64_t capacity, o3dmi_stream_t stream,
            o3dmi_control_grid** out) {
    const int64_t dsize = 3 * sizeof(float);
    o3dmi_hash_t* h = nullptr;
    int st = o3dmi_hash_create(std::max<int64_t>(capacity, 1), 1, &dsize,
                               stream, &h);
    if (st) return st;
    auto* g = new o3dmi_control_grid;
    g->grid_size = grid_size;
    g->hash = h;
    *out = g;
    return O3DMI_OK;
}

int CheckFrame(const void* depth_dev, int depth_dtype, int rows, int cols,
               const double* intrinsic, const double* extrinsic,
               const float* depth_out_dev) {
    O3DMI_REQUIRE(depth_dev && intrinsic && extrinsic && depth_out_dev,
                  "null argument");
    O3DMI_REQUIRE(depth_dtype == O3DMI_U16 || depth_dtype == O3DMI_F32,
                  "depth dtype must be UInt16 or Float32");
    O3DMI_REQUIRE(rows > 0 && cols > 0, "empty image");
    return O3DMI_OK;
}

int Project(const float* points_dev, const float* colors_dev, int64_t n,
            int rows, int cols, const double* intrinsic,
            const double* extrinsic, float depth_scale, float depth_max,
            float* depth_out_dev, float* color_out_dev,
            o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n >= 0 && n < (1ll << 32), "point count out of range");
    O3DMI_REQUIRE((n == 0 || points_dev) && intrinsic && extrinsic &&
                          depth_out_dev,
                  "null argument");
    O3DMI_REQUIRE(rows > 0 && cols > 0, "empty image");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    unsigned long long* packed = nullptr;
    int st = sc.Alloc(&packed, sizeof(unsigned long long) * (size_t)rows *
                                       (size_t)cols);
    if (st) return st;
    const ControlGridFrame f = MakeControlGridFrame(
            intrinsic, extrinsic, rows, cols, depth_scale, depth_max);
    if ((st = ProjectPackAsync(points_dev, n, f, packed, s))) return st;
    return ProjectResolveAsync(packed, rows, cols, colors_dev, O3DMI_F32,
                               depth_out_dev, color_out_dev, s);
}

int DeformImage(o3dmi_control_grid* g, const void* depth_dev, int depth_dtype,
                const void* color_dev, int color_dtype, int rows, int cols,
                const double* intrinsic, const double* extrinsic,
                float depth_scale, float depth_max, float* depth_out_dev,
                float* color_out_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr, "control grid is null");
    int st = CheckFrame(depth_dev, depth_dtype, rows, cols, intrinsic,
                        extrinsic, depth_out_dev);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    unsigned long long* packed = nullptr;
    if ((st = sc.Alloc(&packed, sizeof(unsigned long long) * (size_t)rows *
                                        (size_t)cols)))
        return st;
    const ControlGridFrame f = MakeControlGridFrame(
            intrinsic, extrinsic, rows, cols, depth_scale, depth_max);
    if ((st = ControlGridDeformImagePackAsync(g->hash, depth_dev, depth_dtype,
                                              f, g->grid_size, packed, s)))
        return st;
    return ProjectResolveAsync(packed, rows, cols, color_dev, color_dtype,
                               depth_out_dev, color_out_dev, s);
}

}  // namespace

extern "C" int o3dmi_control_grid_create(float grid_size, int64_t grid_count,
                                         o3dmi_stream_t stream,
                                         o3dmi_control_grid_t** out) {
    O3DMI_REQUIRE(out != nullptr, "out is null");
    O3DMI_REQUIRE(grid_size > 0, "grid_size must be > 0");
    O3DMI_REQUIRE(grid_count >= 0, "grid_count < 0");
    return NewGrid(grid_size, grid_count, stream, out);
}

extern "C" int o3dmi_control_grid_create_from(float grid_size,
                                              const int32_t* keys_dev,
                                              const float* values_dev,
                                              int64_t n,
                                              o3dmi_stream_t stream,
                                              o3dmi_control_grid_t** out) {
    O3DMI_REQUIRE(out != nullptr, "out is null");
    O3DMI_REQUIRE(grid_size > 0, "grid_size must be > 0");
    O3DMI_REQUIRE(n >= 0 && (n == 0 || (keys_dev && values_dev)),
                  "null argument");
    o3dmi_control_grid* g = nullptr;
    int st = NewGrid(grid_size, 2 * n, stream, &g);
    if (st) return st;
    const void* values[1] = {values_dev};
    int64_t size = 0;
    if ((st = o3dmi_hash_insert(g->hash, keys_dev, values, n, nullptr, nullptr,
                                stream)) ||
        (st = o3dmi_hash_size(g->hash, stream, &size))) {
        o3dmi_control_grid_destroy(g);
        return st;
    }
    *out = g;
    return O3DMI_OK;
}

extern "C" int o3dmi_control_grid_destroy(o3dmi_control_grid_t* g) {
    if (!g) return O3DMI_OK;
    (void)o3dmi_hash_destroy(g->hash);
    delete g;
    return O3DMI_OK;
}

extern "C" int o3dmi_control_grid_touch(o3dmi_control_grid_t* g,
                                        const float* points_dev, int64_t n,
                                        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr, "control grid is null");
    O3DMI_REQUIRE(n >= 0 && (n == 0 || points_dev), "null argument");
    if (n == 0) return O3DMI_OK;
    hipStream_t s = (hipStream_t)stream;
    // every round at least doubles the capacity
    for (int round = 0; round < 40; ++round) {
        int st = ControlGridTouchAsync(g->hash, points_dev, n, g->grid_size, s);
        if (st) return st;
        int counters[4] = {0, 0, 0, 0};
        O3DMI_HIP_CHECK(hipMemcpyAsync(counters, g->hash->view.counters,
                                       sizeof(counters),
                                       hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        if (counters[3] == 0) {
            int64_t size = 0;  // reports the deferred error flags
            return o3dmi_hash_size(g->hash, stream, &size);
        }
        int64_t wanted = 0;
        if ((st = RecoverOverflow(g->hash, s, &wanted))) return st;
        const int64_t capacity = o3dmi_hash_capacity(g->hash);
        if ((st = o3dmi_hash_reserve(g->hash,
                                     std::max(wanted, 2 * capacity), stream)))
            return st;
    }
    SetLastError("control grid: the node map did not stop growing");
    return O3DMI_ERR_INTERNAL;
}

extern "C" int o3dmi_control_grid_compactify(o3dmi_control_grid_t* g,
                                             o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr, "control grid is null");
    hipStream_t s = (hipStream_t)stream;
    int64_t size = 0;
    int st = o3dmi_hash_size(g->hash, stream, &size);
    if (st) return st;
    if ((st = o3dmi_hash_reserve(g->hash, 2 * size, stream))) return st;
    g->anchor_idx = -1;
    if (size == 0) return O3DMI_OK;
    PoolScratch sc(s);
    int32_t* active = nullptr;
    int32_t* keys = nullptr;
    const int64_t capacity = o3dmi_hash_capacity(g->hash);
    if ((st = sc.Alloc(&active, sizeof(int32_t) * (size_t)capacity)) ||
        (st = sc.Alloc(&keys, 3 * sizeof(int32_t) * (size_t)capacity)))
        return st;
    int64_t n = 0;
    if ((st = o3dmi_hash_active_indices(g->hash, active, stream, &n)) ||
        (st = GatherRows(o3dmi_hash_key_buffer(g->hash), active, n,
                         3 * sizeof(int32_t), keys, s)))
        return st;
    std::vector<int32_t> idx((size_t)n);
    std::vector<std::array<int32_t, 3>> k((size_t)n);
    O3DMI_HIP_CHECK(hipMemcpyAsync(idx.data(), active, sizeof(int32_t) * n,
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipMemcpyAsync(k.data(), keys, 3 * sizeof(int32_t) * n,
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    if (n == 0) return O3DMI_OK;
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[i] = i;
    // ControlGrid.cpp:103-107: by (z, y, x)
    std::nth_element(order.begin(), order.begin() + n / 2, order.end(),
                     [&](int64_t a, int64_t b) {
                         const auto& p = k[a];
                         const auto& q = k[b];
                         return (p[2] < q[2]) ||
                                (p[2] == q[2] && p[1] < q[1]) ||
                                (p[2] == q[2] && p[1] == q[1] && p[0] < q[0]);
                     });
    g->anchor_idx = idx[order[n / 2]];
    return O3DMI_OK;
}

extern "C" int o3dmi_control_grid_size(o3dmi_control_grid_t* g,
                                       o3dmi_stream_t stream, int64_t* size) {
    O3DMI_REQUIRE(g != nullptr && size != nullptr, "null argument");
    return o3dmi_hash_size(g->hash, stream, size);
}

extern "C" int o3dmi_control_grid_anchor_idx(const o3dmi_control_grid_t* g) {
    return g ? g->anchor_idx : -1;
}

extern "C" float o3dmi_control_grid_grid_size(const o3dmi_control_grid_t* g) {
    return g ? g->grid_size : 0.0f;
}

extern "C" o3dmi_hash_t* o3dmi_control_grid_hashmap(o3dmi_control_grid_t* g) {
    return g ? g->hash : nullptr;
}

extern "C" int o3dmi_control_grid_init_positions(o3dmi_control_grid_t* g,
                                                 float* out_dev,
                                                 o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr && out_dev != nullptr, "null argument");
    return ControlGridInitPositionsAsync(g->hash, g->grid_size, out_dev,
                                         (hipStream_t)stream);
}

extern "C" float* o3dmi_control_grid_curr_positions(o3dmi_control_grid_t* g) {
    return g ? (float*)o3dmi_hash_value_buffer(g->hash, 0) : nullptr;
}

extern "C" int o3dmi_control_grid_neighbor_grid_map(
        o3dmi_control_grid_t* g, int32_t* active_dev, int32_t* nb_indices_dev,
        uint8_t* nb_masks_dev, int64_t* n_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && active_dev && nb_indices_dev && nb_masks_dev && n_out,
                  "null argument");
    int64_t n = 0;
    int st = o3dmi_hash_active_indices(g->hash, active_dev, stream, &n);
    if (st) return st;
    *n_out = n;
    if (n == 0) return O3DMI_OK;
    // the slot scan lists the nodes in arrival order: sorted, the map is the
    // same on every run
    if ((st = o3dmi_sort_indices(active_dev, n, stream))) return st;
    if ((st = ControlGridNeighborMapAsync(g->hash, active_dev, n,
                                          nb_indices_dev, nb_masks_dev,
                                          (hipStream_t)stream)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return O3DMI_OK;
}

extern "C" int o3dmi_control_grid_parameterize(
        o3dmi_control_grid_t* g, const float* points_dev,
        const float* normals_dev, const float* colors_dev, int64_t n,
        int64_t out_capacity, float* out_points_dev, float* out_normals_dev,
        float* out_colors_dev, int32_t* out_indices_dev,
        float* out_vertex_ratios_dev, float* out_normal_ratios_dev,
        int64_t* m_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr && m_out != nullptr, "null argument");
    O3DMI_REQUIRE(n >= 0 && out_capacity >= 0, "negative count");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && out_points_dev && out_indices_dev &&
                          out_vertex_ratios_dev,
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    int32_t* flags = nullptr;
    int64_t* position = nullptr;
    void* scan_tmp = nullptr;
    int64_t* total = nullptr;
    int st;
    if ((st = sc.Alloc(&flags, sizeof(int32_t) * (size_t)n)) ||
        (st = sc.Alloc(&position, sizeof(int64_t) * (size_t)n)) ||
        (st = sc.Alloc(&scan_tmp, ScanScratchBytes(n))) ||
        (st = sc.Alloc(&total, sizeof(int64_t))))
        return st;
    if ((st = ControlGridValidAsync(g->hash, points_dev, n, g->grid_size,
                                    flags, s)) ||
        (st = PrefixSumAsync(flags, n, false, position, total, scan_tmp, s)))
        return st;
    int64_t m = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&m, total, sizeof(m), hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    *m_out = m;
    if (m > out_capacity) {
        SetLastError("control grid: parameterize output too small");
        return O3DMI_ERR_CAPACITY;
    }
    if ((st = ControlGridParameterizeAsync(
                 g->hash, points_dev, normals_dev, colors_dev, n, g->grid_size,
                 flags, position, out_points_dev, out_normals_dev,
                 out_colors_dev, out_indices_dev, out_vertex_ratios_dev,
                 out_normal_ratios_dev, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

extern "C" int o3dmi_control_grid_deform(o3dmi_control_grid_t* g,
                                         const int32_t* indices_dev,
                                         const float* vertex_ratios_dev,
                                         const float* normal_ratios_dev,
                                         int64_t n, float* out_points_dev,
                                         float* out_normals_dev,
                                         o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr, "control grid is null");
    O3DMI_REQUIRE(n >= 0, "negative count");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(indices_dev && vertex_ratios_dev && out_points_dev,
                  "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    int* bad = nullptr;
    int st = sc.Alloc(&bad, sizeof(int));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    if ((st = ControlGridDeformAsync(g->hash, indices_dev, vertex_ratios_dev,
                                     normal_ratios_dev, n, out_points_dev,
                                     out_normals_dev, bad, s)))
        return st;
    int h = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(h == 0, "control grid: node index out of range");
    return O3DMI_OK;
}

extern "C" int o3dmi_project_to_depth_image(
        const float* points_dev, int64_t n, int rows, int cols,
        const double* intrinsic, const double* extrinsic, float depth_scale,
        float depth_max, float* depth_out_dev, o3dmi_stream_t stream) {
    return Project(points_dev, nullptr, n, rows, cols, intrinsic, extrinsic,
                   depth_scale, depth_max, depth_out_dev, nullptr, stream);
}

extern "C" int o3dmi_project_to_rgbd_image(
        const float* points_dev, const float* colors_dev, int64_t n, int rows,
        int cols, const double* intrinsic, const double* extrinsic,
        float depth_scale, float depth_max, float* depth_out_dev,
        float* color_out_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE((n == 0 || colors_dev) && color_out_dev, "null argument");
    return Project(points_dev, colors_dev, n, rows, cols, intrinsic, extrinsic,
                   depth_scale, depth_max, depth_out_dev, color_out_dev,
                   stream);
}

extern "C" int o3dmi_control_grid_deform_depth_image(
        o3dmi_control_grid_t* g, const void* depth_dev, int depth_dtype,
        int rows, int cols, const double* intrinsic, const double* extrinsic,
        float depth_scale, float depth_max, float* depth_out_dev,
        o3dmi_stream_t stream) {
    return DeformImage(g, depth_dev, depth_dtype, nullptr, O3DMI_F32, rows,
                       cols, intrinsic, extrinsic, depth_scale, depth_max,
                       depth_out_dev, nullptr, stream);
}

extern "C" int o3dmi_control_grid_deform_rgbd_image(
        o3dmi_control_grid_t* g, const void* depth_dev, int depth_dtype,
        const void* color_dev, int color_dtype, int rows, int cols,
        const double* intrinsic, const double* extrinsic, float depth_scale,
        float depth_max, float* depth_out_dev, float* color_out_dev,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(color_dev && color_out_dev, "null argument");
    O3DMI_REQUIRE(color_dtype == O3DMI_U8 || color_dtype == O3DMI_F32,
                  "colour dtype must be UInt8 or Float32");
    return DeformImage(g, depth_dev, depth_dtype, color_dev, color_dtype, rows,
                       cols, intrinsic, extrinsic, depth_scale, depth_max,
                       depth_out_dev, color_out_dev, stream);
}
