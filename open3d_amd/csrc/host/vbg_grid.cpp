// Host-side VoxelBlockGrid for the MI355X backend: the orchestration of
// t::geometry::VoxelBlockGrid (cpp/open3d/t/geometry/VoxelBlockGrid.cpp:65-117
// ctor, :212-245 GetUniqueBlockCoordinates, :292-326 Integrate, :328-402
// RayCast) and of core::HashMap::Activate's capacity policy
// (cpp/open3d/core/hashmap/HashMap.cpp:166-181) on top of the kernel C ABI.
//
// What differs from the reference is where counts live: the reference reads
// Size() and the candidate count back to the host every frame; here the
// host keeps an upper bound of the map size and only synchronises when that
// bound says a Reserve() might be needed, so the steady-state frame stream
// (o3dmi_vbg_integrate_frame) issues kernels back to back.

#include <cstdlib>
#include <cstring>

#include "vbg.h"

using namespace o3dmi;

namespace {

// HashMap::Activate's pre-amble (HashMap.cpp:166-176): if Size()+length would
// exceed the capacity, Reserve(max(new_size, 2*capacity)). `size_bound` avoids
// the Size() read-back while it proves no growth is needed.
int EnsureCapacity(o3dmi_vbg* g, int64_t length, o3dmi_stream_t stream) {
    if (g->size_event_pending) {
        O3DMI_HIP_CHECK(hipEventSynchronize(g->size_event));
        g->size_event_pending = false;
        g->size_bound = g->size_host[0];
    }
    int64_t capacity = o3dmi_hash_capacity(g->block_hashmap);
    if (g->size_bound + length <= capacity) {
        g->size_bound += length;
        return O3DMI_OK;
    }
    int64_t size = 0;
    int st = o3dmi_hash_size(g->block_hashmap, stream, &size);
    if (st) return st;
    int64_t new_size = size + length;
    if (new_size > capacity) {
        int64_t target = new_size > capacity * 2 ? new_size : capacity * 2;
        st = o3dmi_hash_reserve(g->block_hashmap, target, stream);
        if (st) return st;
    }
    g->size_bound = new_size;
    return O3DMI_OK;
}

int EnsureScratch(o3dmi_vbg* g, int64_t m) {
    if (m <= g->scratch_capacity) return O3DMI_OK;
    (void)hipFree(g->scratch_buf_indices);
    g->scratch_buf_indices = nullptr;
    O3DMI_HIP_CHECK(hipMalloc((void**)&g->scratch_buf_indices,
                              sizeof(int32_t) * (size_t)m));
    g->scratch_capacity = m;
    return O3DMI_OK;
}

// ExtractPointCloud / ExtractTriangleMesh (VoxelBlockGrid.cpp:404-471): the
// seam `extract` over the active blocks, sorted (the mesh seam finds a
// neighbour's position by bisection). The seams synchronise the stream.
template <typename F>
int ExtractSurface(o3dmi_vbg* g, o3dmi_stream_t stream, F&& extract) {
    TsdfAttrs at;
    int st = ResolveTsdf(g, &at);
    if (st) return st;
    PoolScratch scratch((hipStream_t)stream);
    ActiveList active;
    if ((st = active.Fill(g, true, scratch, stream))) return st;
    return extract(at, active);
}

int RunIntegrate(o3dmi_vbg* g, const int32_t* indices, int64_t n,
                 const int32_t* n_dev, const void* depth, int drows, int dcols,
                 const void* color, int crows, int ccols, int input_dtype,
                 const double* Kd, const double* Kc, const double* T,
                 float depth_scale, float depth_max, float trunc_mult,
                 o3dmi_stream_t stream) {
    TsdfAttrs at;
    const int st = ResolveTsdf(g, &at);
    if (st) return st;
    O3DMI_REQUIRE(g->attr_dtypes[(size_t)at.ti] == O3DMI_F32,
                  "tsdf must be Float32");
    bool integrate_color = color != nullptr && (int64_t)crows * ccols > 0;
    return o3dmi_vbg_integrate(
            depth, drows, dcols, integrate_color ? color : nullptr, crows,
            ccols, input_dtype, indices, n, n_dev,
            o3dmi_hash_key_buffer(g->block_hashmap), at.tsdf, at.weight,
            integrate_color ? at.color : nullptr, at.grid_dtype, Kd,
            Kc ? Kc : Kd, T, (int)g->block_resolution, g->voxel_size,
            g->voxel_size * trunc_mult, depth_scale, depth_max, stream);
}


// Folds foreign blocks into the grid (o3dmi_vbg_merge_blocks): one thread per
// voxel, block b of the foreign set lands in buffer row indices[b]. Streaming:
// reads both sides once, writes the grid side once.
template <typename W>
__global__ void MergeBlocksKernel(const int32_t* __restrict__ indices,
                                  int64_t n_voxels_total, int voxels_per_block,
                                  float* __restrict__ tsdf,
                                  W* __restrict__ weight, W* __restrict__ color,
                                  const float* __restrict__ src_tsdf,
                                  const W* __restrict__ src_weight,
                                  const W* __restrict__ src_color) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n_voxels_total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / voxels_per_block;
        const int64_t v = i - b * voxels_per_block;
        const int64_t d = (int64_t)indices[b] * voxels_per_block + v;
        const float w2 = (float)src_weight[i];
        if (w2 == 0) continue;
        const float w1 = (float)weight[d];
        if (w1 == 0) {
            tsdf[d] = src_tsdf[i];
            weight[d] = src_weight[i];
            if (color)
                for (int c = 0; c < 3; ++c) color[3 * d + c] = src_color[3 * i + c];
            continue;
        }
        const float inv = 1.0f / (w1 + w2);
        tsdf[d] = (w1 * tsdf[d] + w2 * src_tsdf[i]) * inv;
        if (color)
            for (int c = 0; c < 3; ++c)
                color[3 * d + c] = (W)((w1 * (float)color[3 * d + c] +
                                        w2 * (float)src_color[3 * i + c]) *
                                       inv);
        // a uint16 weight saturates (long per-rank streams can pass 65535;
        // float -> uint16 of a larger value is undefined)
        const float wsum = w1 + w2;
        if constexpr (sizeof(W) == 2)
            weight[d] = (W)(wsum < 65535.0f ? wsum : 65535.0f);
        else
            weight[d] = (W)wsum;
    }
}

// The generic per-frame path (touch + activate, then integrate): every grid
// the frame stream does not apply to.
int IntegrateFrameGeneric(o3dmi_vbg_t* g, const void* depth_dev, int depth_rows,
                          int depth_cols, const void* color_dev, int color_rows,
                          int color_cols, int input_dtype,
                          const double* depth_intrinsic,
                          const double* color_intrinsic,
                          const double* extrinsic, float depth_scale,
                          float depth_max, float trunc_voxel_multiplier,
                          o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_dev && depth_intrinsic && extrinsic,
                  "null argument");
    const int stride = 4;
    int64_t max_new = (int64_t)(depth_cols / stride) * (depth_rows / stride) * 4;
    O3DMI_REQUIRE(max_new > 0, "depth image too small");
    if (g->frame_indices_capacity < max_new) {
        (void)hipFree(g->frame_indices);
        g->frame_indices = nullptr;
        O3DMI_HIP_CHECK(hipMalloc((void**)&g->frame_indices,
                                  sizeof(int32_t) * (size_t)max_new));
        g->frame_indices_capacity = max_new;
    }
    // Capacity policy (HashMap::Activate, HashMap.cpp:166-176, with `length`
    // = the most blocks one frame can create). The exact map size after the
    // previous frame's activation was copied to pinned memory right behind
    // that frame's touch kernel; waiting for it does not drain the GPU (the
    // previous frame's integrate kernel is still running) and keeps the
    // Reserve decision exact instead of heuristic.
    hipStream_t s = (hipStream_t)stream;
    if (g->size_event_pending) {
        O3DMI_HIP_CHECK(hipEventSynchronize(g->size_event));
        g->size_event_pending = false;
        if (g->size_host[1] & kErrKeyRange) {
            SetLastError("block coordinate outside +-2^20");
            return O3DMI_ERR_KEY_RANGE;
        }
        if (g->size_host[1] & kErrCapacity) {
            SetLastError("hash map capacity exceeded");
            return O3DMI_ERR_CAPACITY;
        }
        g->size_bound = g->size_host[0];
    }
    int64_t capacity = o3dmi_hash_capacity(g->block_hashmap);
    if (g->size_bound + max_new > capacity) {
        int64_t size = 0;
        int st = o3dmi_hash_size(g->block_hashmap, stream, &size);
        if (st) return st;
        g->size_bound = size;
        if (size + max_new > capacity) {
            int64_t need = size + max_new;
            int64_t target = need > capacity * 2 ? need : capacity * 2;
            st = o3dmi_hash_reserve(g->block_hashmap, target, stream);
            if (st) return st;
        }
    }

    int dt = input_dtype == O3DMI_F32 ? O3DMI_F32 : O3DMI_U16;
    g->known_valid = false;
    g->frame_stamp += 1;
    const bool prof = g->profiling && g->prof_frames < g->prof_max &&
                      g->prof_stride > 0 &&
                      (g->prof_seen++ % g->prof_stride) == 0;
    int st = o3dmi_vbg_touch_activate(
            g->block_hashmap, depth_dev, dt, depth_rows, depth_cols,
            depth_intrinsic, extrinsic, g->frame_indices, max_new,
            g->frame_count, (int)g->block_resolution, g->voxel_size,
            g->voxel_size * trunc_voxel_multiplier, depth_scale, depth_max,
            stride, g->frame_stamp, stream);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(g->size_host, g->block_hashmap->view.counters,
                                   sizeof(int) * 2, hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipEventRecord(g->size_event, s));
    g->size_event_pending = true;
    g->size_bound += max_new;  // until the read-back lands
    if (prof) {
        O3DMI_HIP_CHECK(hipMemcpyAsync(g->prof_counts + g->prof_frames,
                                       g->frame_count, sizeof(int32_t),
                                       hipMemcpyDeviceToDevice, s));
        O3DMI_HIP_CHECK(hipEventRecord(
                g->prof_events[(size_t)g->prof_frames * 2 + 0], s));
    }
    g->last_path = 2;
    st = RunIntegrate(g, g->frame_indices, max_new, g->frame_count, depth_dev,
                      depth_rows, depth_cols, color_dev, color_rows,
                      color_cols, input_dtype, depth_intrinsic,
                      color_intrinsic, extrinsic, depth_scale, depth_max,
                      trunc_voxel_multiplier, stream);
    if (prof) {
        O3DMI_HIP_CHECK(hipEventRecord(
                g->prof_events[(size_t)g->prof_frames * 2 + 1], s));
        g->prof_launch_frames += 1;
        g->prof_frames += 1;
    }
    return st;
}

}  // namespace

namespace o3dmi {

int DtypeSize(int dt) {
    switch (dt) {
        case O3DMI_F32: return 4;
        case O3DMI_F64: return 8;
        case O3DMI_U16: return 2;
        case O3DMI_U8: return 1;
        case O3DMI_I32: return 4;
        case O3DMI_I64: return 8;
        default: return 0;
    }
}

int ResolveTsdf(o3dmi_vbg* g, TsdfAttrs* a) {
    a->ti = g->AttrIndex("tsdf");
    a->wi = g->AttrIndex("weight");
    a->ci = g->AttrIndex("color");
    if (a->ti < 0 || a->wi < 0) {
        SetLastError(
                "TSDF and/or weight not allocated in blocks, please implement "
                "customized integration.");
        return O3DMI_ERR_INVALID_ARG;
    }
    const int wdt = g->attr_dtypes[(size_t)a->wi];
    const int cdt = a->ci >= 0 ? g->attr_dtypes[(size_t)a->ci] : wdt;
    if (wdt == O3DMI_F32 && cdt == O3DMI_F32) a->grid_dtype = O3DMI_F32;
    else if (wdt == O3DMI_U16 && cdt == O3DMI_U16) a->grid_dtype = O3DMI_U16;
    else {
        SetLastError(
                "Unsupported value data type combination. Expected (float, "
                "float) or (uint16, uint16)");
        return O3DMI_ERR_INVALID_ARG;
    }
    a->tsdf = (float*)o3dmi_hash_value_buffer(g->block_hashmap, a->ti);
    a->weight = o3dmi_hash_value_buffer(g->block_hashmap, a->wi);
    a->color = a->ci >= 0 ? o3dmi_hash_value_buffer(g->block_hashmap, a->ci)
                          : nullptr;
    return O3DMI_OK;
}

}  // namespace o3dmi

extern "C" {

int o3dmi_vbg_create(int n_attrs, const char* const* attr_names,
                     const int* attr_dtypes, const int* attr_channels,
                     float voxel_size, int64_t block_resolution,
                     int64_t block_count, o3dmi_stream_t stream,
                     o3dmi_vbg_t** out) {
    O3DMI_REQUIRE(out != nullptr, "out is null");
    O3DMI_REQUIRE(voxel_size > 0, "voxel size must be positive");
    O3DMI_REQUIRE(block_resolution > 0, "block resolution must be positive");
    O3DMI_REQUIRE(n_attrs > 0 && n_attrs <= 8 && attr_names && attr_dtypes &&
                          attr_channels,
                  "Number of attribute dtypes/channels mismatch with names.");
    auto* g = new o3dmi_vbg();
    g->voxel_size = voxel_size;
    g->block_resolution = block_resolution;
    int64_t dsizes[8];
    int64_t res3 = block_resolution * block_resolution * block_resolution;
    for (int i = 0; i < n_attrs; ++i) {
        int sz = DtypeSize(attr_dtypes[i]);
        if (sz == 0 || attr_channels[i] <= 0) {
            delete g;
            SetLastError("bad attribute dtype / channels");
            return O3DMI_ERR_INVALID_ARG;
        }
        g->attr_names.emplace_back(attr_names[i]);
        g->attr_dtypes.push_back(attr_dtypes[i]);
        g->attr_channels.push_back(attr_channels[i]);
        dsizes[i] = res3 * attr_channels[i] * sz;
    }
    int st = o3dmi_hash_create(block_count, n_attrs, dsizes, stream,
                               &g->block_hashmap);
    if (st == O3DMI_OK) {
        hipError_t e = hipMalloc((void**)&g->frame_count, sizeof(int32_t) * 4);
        if (e == hipSuccess)
            e = hipHostMalloc((void**)&g->size_host, sizeof(int) * 4);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&g->size_event, hipEventDisableTiming);
        if (e != hipSuccess) st = O3DMI_ERR_HIP;
    }
    if (st != O3DMI_OK) {
        o3dmi_vbg_destroy(g);
        return st;
    }
    // The frame stream's short division forms are proven per truncation
    // distance on the device, asynchronously (vbg_stream.hip): start the proof
    // for the API's default multiplier now, so that it is over before frames
    // arrive.
    if (block_resolution % 4 == 0)
        (void)PrefetchFastDivision(voxel_size * 8.0f, false);
    *out = g;
    return O3DMI_OK;
}

int o3dmi_vbg_division_forms(float voxel_size, float trunc_voxel_multiplier,
                             int wait) {
    return PrefetchFastDivision(voxel_size * trunc_voxel_multiplier, wait != 0);
}

int64_t o3dmi_vbg_step_form_launches(int form) {
    return (int64_t)StepFormLaunches(form);
}

int32_t o3dmi_vbg_front_tile_key_limit(void) { return FrontTileKeyLimit(); }

// VoxelBlockGrid::To(device, copy) (VoxelBlockGrid.cpp, via
// HashMap::To, core/hashmap/HashMap.cpp:230-255): the same grid on another
// (or the same) device -- attribute layout and voxel size carried over, the
// block hash map cloned with its value rows, scratch state fresh.
int o3dmi_vbg_to_device(o3dmi_vbg_t* g, int device, o3dmi_vbg_t** out) {
    O3DMI_REQUIRE(g != nullptr && out != nullptr, "null argument");
    int cur = 0;
    O3DMI_HIP_CHECK(hipGetDevice(&cur));
    o3dmi_hash_t* hm = nullptr;
    int st = o3dmi_hash_to_device(g->block_hashmap, device, &hm);
    if (st) return st;
    auto* n = new o3dmi_vbg();
    n->voxel_size = g->voxel_size;
    n->block_resolution = g->block_resolution;
    n->attr_names = g->attr_names;
    n->attr_dtypes = g->attr_dtypes;
    n->attr_channels = g->attr_channels;
    n->owner_rank = g->owner_rank;
    n->owner_world = g->owner_world;
    n->block_hashmap = hm;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = hipMalloc((void**)&n->frame_count, sizeof(int32_t) * 4);
    if (e == hipSuccess)
        e = hipHostMalloc((void**)&n->size_host, sizeof(int) * 4);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&n->size_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        o3dmi_vbg_destroy(n);
        (void)hipSetDevice(cur);
        SetLastError(std::string("o3dmi_vbg_to_device: ") +
                     hipGetErrorString(e));
        return O3DMI_ERR_HIP;
    }
    (void)hipSetDevice(cur);
    *out = n;
    return O3DMI_OK;
}

int o3dmi_vbg_destroy(o3dmi_vbg_t* g) {
    if (!g) return O3DMI_OK;
    o3dmi_hash_destroy(g->block_hashmap);
    o3dmi_hash_destroy(g->frustum_hashmap);
    (void)hipFree(g->frame_indices);
    (void)hipFree(g->frame_count);
    (void)hipFree(g->scratch_buf_indices);
    if (g->size_host) (void)hipHostFree(g->size_host);
    if (g->size_event) (void)hipEventDestroy(g->size_event);
    for (int i = 0; i < 2; ++i) {
        for (int f = 0; f < kMaxGroup; ++f) (void)hipFree(g->recs[i][f]);
        (void)hipFree(g->lists[i]);
        (void)hipFree(g->ready[i]);
        if (i == 0) (void)hipFree(g->prep_col);
    }
    (void)hipFree(g->front_tickets);
    (void)hipFree(g->ring_counters);
    (void)hipFree(g->own_range);
    (void)hipFree(g->rc_cost);
    (void)hipFree(g->rc_order);
    if (g->stream_status) (void)hipHostFree((void*)g->stream_status);
    for (hipEvent_t e : g->prof_events) (void)hipEventDestroy(e);
    (void)hipFree(g->prof_counts);
    FreeSliced(g);
    delete g;
    return O3DMI_OK;
}

int o3dmi_vbg_set_block_ownership(o3dmi_vbg_t* g, int rank, int world) {
    O3DMI_REQUIRE(g != nullptr, "grid is null");
    int st = o3dmi_hash_set_ownership(g->block_hashmap, rank, world);
    if (st) return st;
    if (g->frustum_hashmap &&
        (st = o3dmi_hash_set_ownership(g->frustum_hashmap, rank, world)))
        return st;
    g->owner_rank = rank;
    g->owner_world = world;
    return O3DMI_OK;
}

o3dmi_hash_t* o3dmi_vbg_hashmap(o3dmi_vbg_t* g) {
    return g ? g->block_hashmap : nullptr;
}

void* o3dmi_vbg_attribute(o3dmi_vbg_t* g, const char* name, int* dtype,
                          int* channels) {
    if (!g || !name) return nullptr;
    int i = g->AttrIndex(name);
    if (i < 0) return nullptr;  // "Attribute {} not found, return empty tensor."
    if (dtype) *dtype = g->attr_dtypes[(size_t)i];
    if (channels) *channels = g->attr_channels[(size_t)i];
    return o3dmi_hash_value_buffer(g->block_hashmap, i);
}

int o3dmi_vbg_get_unique_block_coordinates(
        o3dmi_vbg_t* g, const void* depth_dev, int depth_dtype, int rows,
        int cols, const double* intrinsic, const double* extrinsic,
        float depth_scale, float depth_max, float trunc_voxel_multiplier,
        int32_t* out_coords_dev, int64_t* m_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_dev && out_coords_dev && m_out, "null argument");
    const int64_t down_factor = 4;
    const int64_t est_sample_multiplier = 4;
    int64_t capacity = (cols / down_factor) * (rows / down_factor) *
                       est_sample_multiplier;
    O3DMI_REQUIRE(capacity > 0, "depth image too small");
    if (g->frustum_hashmap == nullptr || g->frustum_capacity < capacity) {
        o3dmi_hash_destroy(g->frustum_hashmap);
        g->frustum_hashmap = nullptr;
        int st = o3dmi_hash_create(capacity, 0, nullptr, stream,
                                   &g->frustum_hashmap);
        if (st) return st;
        g->frustum_capacity = capacity;
        if ((st = o3dmi_hash_set_ownership(g->frustum_hashmap, g->owner_rank,
                                           g->owner_world)))
            return st;
    }
    int st = o3dmi_vbg_depth_touch(
            g->frustum_hashmap, depth_dev, depth_dtype, rows, cols, intrinsic,
            extrinsic, out_coords_dev, capacity, g->frame_count,
            (int)g->block_resolution, g->voxel_size,
            g->voxel_size * trunc_voxel_multiplier, depth_scale, depth_max,
            (int)down_factor, stream);
    if (st) return st;
    // The count rides to pinned memory in front of the size query's own copy
    // and wait: one round trip to the host per call (as upstream: the size of
    // the returned tensor), not one per word.
    g->size_host[2] = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&g->size_host[2], g->frame_count,
                                   sizeof(int32_t), hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
    int64_t dummy = 0;
    st = o3dmi_hash_size(g->frustum_hashmap, stream, &dummy);  // syncs + errors
    if (st) return st;
    const int32_t count = g->size_host[2];
    *m_out = count;
    if (count == 0) {
        SetLastError(o3dmi_status_string(O3DMI_ERR_NO_BLOCKS));
        return O3DMI_ERR_NO_BLOCKS;
    }
    return O3DMI_OK;
}

int o3dmi_vbg_get_unique_block_coordinates_pcd(
        o3dmi_vbg_t* g, const float* points_dev, int64_t n,
        float trunc_voxel_multiplier, int32_t* out_coords_dev,
        int64_t out_capacity, int64_t* m_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && m_out && n >= 0 && out_capacity >= 0, "null argument");
    *m_out = 0;
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(points_dev && out_coords_dev, "null argument");
    const int64_t est_neighbor_multiplier = 8;  // VoxelBlockGrid.cpp:251
    const int64_t capacity = n * est_neighbor_multiplier;
    if (g->frustum_hashmap == nullptr || g->frustum_capacity < capacity) {
        o3dmi_hash_destroy(g->frustum_hashmap);
        g->frustum_hashmap = nullptr;
        g->frustum_capacity = 0;
        int st = o3dmi_hash_create(capacity, 0, nullptr, stream,
                                   &g->frustum_hashmap);
        if (st) return st;
        g->frustum_capacity = capacity;
        if ((st = o3dmi_hash_set_ownership(g->frustum_hashmap, g->owner_rank,
                                           g->owner_world)))
            return st;
    }
    int st = o3dmi_vbg_pointcloud_touch(
            g->frustum_hashmap, points_dev, n, out_coords_dev, out_capacity,
            g->frame_count, (int)g->block_resolution, g->voxel_size,
            g->voxel_size * trunc_voxel_multiplier, stream);
    if (st) return st;
    g->size_host[2] = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&g->size_host[2], g->frame_count,
                                   sizeof(int32_t), hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
    int64_t dummy = 0;
    st = o3dmi_hash_size(g->frustum_hashmap, stream, &dummy);  // syncs + errors
    if (st) return st;
    const int64_t count = g->size_host[2];
    if (count > out_capacity) {
        *m_out = out_capacity;
        SetLastError("GetUniqueBlockCoordinates: more blocks than "
                     "out_capacity rows");
        return O3DMI_ERR_CAPACITY;
    }
    *m_out = count;
    return O3DMI_OK;
}

int o3dmi_vbg_get_voxel_indices(o3dmi_vbg_t* g, const int32_t* buf_indices_dev,
                                int64_t n_blocks, int64_t* voxel_indices_dev,
                                o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g, "null argument");
    return o3dmi_vbg_voxel_indices(buf_indices_dev, n_blocks,
                                   (int)g->block_resolution, voxel_indices_dev,
                                   stream);
}

int o3dmi_vbg_get_voxel_coordinates(o3dmi_vbg_t* g,
                                    const int64_t* voxel_indices_dev,
                                    int64_t n_voxels, int64_t* voxel_coords_dev,
                                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && n_voxels >= 0, "null argument");
    if (n_voxels == 0) return O3DMI_OK;
    // the word the kernel flags a bad buffer index in: the frame counter's
    // neighbour of the grid's device scratch, read back with the result
    int32_t* err = g->frame_count + 1;
    O3DMI_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int32_t),
                                   (hipStream_t)stream));
    int st = o3dmi_vbg_voxel_coordinates(
            voxel_indices_dev, n_voxels,
            o3dmi_hash_key_buffer(g->block_hashmap),
            o3dmi_hash_capacity(g->block_hashmap), (int)g->block_resolution,
            voxel_coords_dev, err, stream);
    if (st) return st;
    g->size_host[2] = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&g->size_host[2], err, sizeof(int32_t),
                                   hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
    O3DMI_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    O3DMI_REQUIRE(g->size_host[2] == 0,
                  "GetVoxelCoordinates: buffer index out of range");
    return O3DMI_OK;
}

int o3dmi_vbg_get_voxel_coordinates_and_flattened_indices(
        o3dmi_vbg_t* g, const int32_t* buf_indices_dev, int64_t n_blocks,
        float* voxel_coords_dev, int64_t* flattened_indices_dev,
        o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g, "null argument");
    return o3dmi_vbg_voxel_coordinates_and_flattened_indices(
            buf_indices_dev, n_blocks, o3dmi_hash_key_buffer(g->block_hashmap),
            (int)g->block_resolution, g->voxel_size, voxel_coords_dev,
            flattened_indices_dev, stream);
}

int o3dmi_vbg_integrate_blocks(o3dmi_vbg_t* g, const int32_t* block_coords_dev,
                               int64_t m, const void* depth_dev,
                               int depth_rows, int depth_cols,
                               const void* color_dev, int color_rows,
                               int color_cols, int input_dtype,
                               const double* depth_intrinsic,
                               const double* color_intrinsic,
                               const double* extrinsic, float depth_scale,
                               float depth_max, float trunc_voxel_multiplier,
                               o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && block_coords_dev && depth_dev && depth_intrinsic &&
                          extrinsic,
                  "null argument");
    O3DMI_REQUIRE(m >= 0, "m < 0");
    if (m == 0) return O3DMI_OK;
    g->known_valid = false;
    int st = EnsureCapacity(g, m, stream);
    if (st) return st;
    if ((st = EnsureScratch(g, m))) return st;
    // block_hashmap_->Activate(block_coords, ...); ->Find(block_coords, ...)
    st = o3dmi_hash_activate(g->block_hashmap, block_coords_dev, m, nullptr,
                             nullptr, nullptr, stream);
    if (st) return st;
    st = o3dmi_hash_find(g->block_hashmap, block_coords_dev, m, nullptr,
                         g->scratch_buf_indices, nullptr, stream);
    if (st) return st;
    return RunIntegrate(g, g->scratch_buf_indices, m, nullptr, depth_dev,
                        depth_rows, depth_cols, color_dev, color_rows,
                        color_cols, input_dtype, depth_intrinsic,
                        color_intrinsic, extrinsic, depth_scale, depth_max,
                        trunc_voxel_multiplier, stream);
}

int o3dmi_vbg_integrate_frame(o3dmi_vbg_t* g, const void* depth_dev,
                              int depth_rows, int depth_cols,
                              const void* color_dev, int color_rows,
                              int color_cols, int input_dtype,
                              const double* depth_intrinsic,
                              const double* color_intrinsic,
                              const double* extrinsic, float depth_scale,
                              float depth_max, float trunc_voxel_multiplier,
                              o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_dev && depth_intrinsic && extrinsic,
                  "null argument");
    if (!StreamPathApplies(g, input_dtype))
        return IntegrateFrameGeneric(g, depth_dev, depth_rows, depth_cols,
                                     color_dev, color_rows, color_cols,
                                     input_dtype, depth_intrinsic,
                                     color_intrinsic, extrinsic, depth_scale,
                                     depth_max, trunc_voxel_multiplier, stream);
    StreamCommon c = MakeCommon(depth_rows, depth_cols, color_rows, color_cols,
                                depth_intrinsic, color_intrinsic, depth_scale,
                                depth_max, trunc_voxel_multiplier);
    StreamFrame fr = {depth_dev, color_dev, extrinsic};
    return StreamIntegrate(g, c, &fr, 1, 1, (hipStream_t)stream);
}

int o3dmi_vbg_integrate_frames(o3dmi_vbg_t* g, int n_frames,
                               const void* const* depth_devs, int depth_rows,
                               int depth_cols, const void* const* color_devs,
                               int color_rows, int color_cols, int input_dtype,
                               const double* depth_intrinsic,
                               const double* color_intrinsic,
                               const double* extrinsics, float depth_scale,
                               float depth_max, float trunc_voxel_multiplier,
                               int frames_per_launch, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_devs && depth_intrinsic && extrinsics &&
                          n_frames >= 0,
                  "null argument");
    if (!StreamPathApplies(g, input_dtype)) {
        for (int f = 0; f < n_frames; ++f) {
            int st = IntegrateFrameGeneric(
                    g, depth_devs[f], depth_rows, depth_cols,
                    color_devs ? color_devs[f] : nullptr, color_rows,
                    color_cols, input_dtype, depth_intrinsic, color_intrinsic,
                    extrinsics + 16 * (size_t)f, depth_scale, depth_max,
                    trunc_voxel_multiplier, stream);
            if (st) return st;
        }
        return O3DMI_OK;
    }
    StreamCommon c = MakeCommon(depth_rows, depth_cols, color_rows, color_cols,
                                depth_intrinsic, color_intrinsic, depth_scale,
                                depth_max, trunc_voxel_multiplier);
    const std::vector<StreamFrame> frames =
            MakeFrames(depth_devs, color_devs, extrinsics, n_frames);
    const int group = ClampGroup(frames_per_launch);
    // Block ownership with a communicator on this thread: the touch is split
    // over the ranks and the candidate keys all-gathered (sliced_path.h)
    // instead of every rank touching every ray -- when the images allow the
    // raw-image integrate role (else the replicated touch below: same grids).
    if (g->owner_world > 1 && n_frames > 1) {
        o3dmi_comm* comm = ThreadComm();
        static const bool no_slice = std::getenv("O3DMI_NO_SLICED_TOUCH") != nullptr;
        if (comm && !no_slice && comm->world == g->owner_world &&
            comm->rank == g->owner_rank && color_rows == depth_rows &&
            color_cols == depth_cols && (depth_cols % 4) == 0 &&
            (!color_intrinsic ||
             std::memcmp(color_intrinsic, depth_intrinsic,
                         sizeof(double) * 9) == 0 || !color_devs)) {
            // The chunk launch needs the proven short division forms. The
            // proof is a property of the part and the truncation distance,
            // but whether THIS rank has it is rank-local (a failed allocation
            // of the proof's scratch, O3DMI_EXACT_DIV in one rank's
            // environment): the ranks agree once per truncation distance and
            // communicator -- a rank that silently took the
            // non-collective path below would leave its peers in chunk 0's
            // all-gather.
            o3dmi_vbg::Sliced& z = g->sliced;
            const float trunc = g->voxel_size * trunc_voxel_multiplier;
            if (z.agreed_fast_div == 0 || z.agreed_trunc != trunc ||
                z.agreed_comm != (const void*)comm) {
                const int mine = PrefetchFastDivision(trunc, true) == 2
                                         ? O3DMI_OK
                                         : O3DMI_ERR_INTERNAL;
                const int all = comm->AgreeStatus(mine, (hipStream_t)stream);
                z.agreed_fast_div = all == O3DMI_OK ? 1 : -1;
                z.agreed_trunc = trunc;
                z.agreed_comm = (const void*)comm;
            }
            if (z.agreed_fast_div == 1)
                return StreamIntegrateSliced(g, c, frames.data(), n_frames,
                                             group, (hipStream_t)stream, comm,
                                             nullptr);
        }
    }
    return StreamIntegrate(g, c, frames.data(), n_frames, group,
                           (hipStream_t)stream);
}

int o3dmi_vbg_extract_point_cloud(o3dmi_vbg_t* g, float weight_threshold,
                                  int64_t capacity, float* points_dev,
                                  float* normals_dev, float* colors_dev,
                                  int64_t* total_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && total_out, "null argument");
    return ExtractSurface(g, stream, [&](const TsdfAttrs& at,
                                         const ActiveList& active) {
        return o3dmi_vbg_extract_points(
                g->block_hashmap, active.idx, active.n, at.tsdf, at.weight,
                at.color, at.grid_dtype, (int)g->block_resolution,
                g->voxel_size, weight_threshold, points_dev, normals_dev,
                at.ci >= 0 ? colors_dev : nullptr, capacity, total_out,
                stream);
    });
}

int o3dmi_vbg_extract_triangle_mesh(o3dmi_vbg_t* g, float weight_threshold,
                                    int64_t vertex_capacity,
                                    float* vertices_dev, float* normals_dev,
                                    float* colors_dev, int32_t* triangles_dev,
                                    int64_t* n_vertices_out,
                                    int64_t* n_triangles_out,
                                    o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && n_vertices_out && n_triangles_out, "null argument");
    return ExtractSurface(g, stream, [&](const TsdfAttrs& at,
                                         const ActiveList& active) {
        return o3dmi_vbg_extract_mesh(
                g->block_hashmap, active.idx, active.n, at.tsdf, at.weight,
                at.color, at.grid_dtype, (int)g->block_resolution,
                g->voxel_size, weight_threshold, vertices_dev, normals_dev,
                at.ci >= 0 ? colors_dev : nullptr, triangles_dev,
                vertex_capacity, n_vertices_out, n_triangles_out, stream);
    });
}

int o3dmi_vbg_attribute_count(const o3dmi_vbg_t* g) {
    return g ? (int)g->attr_names.size() : 0;
}
const char* o3dmi_vbg_attribute_name(const o3dmi_vbg_t* g, int i) {
    if (!g || i < 0 || i >= (int)g->attr_names.size()) return nullptr;
    return g->attr_names[(size_t)i].c_str();
}
float o3dmi_vbg_voxel_size(const o3dmi_vbg_t* g) {
    return g ? g->voxel_size : 0.f;
}
int64_t o3dmi_vbg_block_resolution(const o3dmi_vbg_t* g) {
    return g ? g->block_resolution : 0;
}

int o3dmi_vbg_export_blocks(o3dmi_vbg_t* g, int64_t capacity,
                            int32_t* keys_dev, void* const* values_dev,
                            int64_t* n_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && n_out, "null argument");
    O3DMI_REQUIRE(keys_dev == nullptr || values_dev != nullptr,
                  "values_dev is null");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch scratch(s);
    ActiveList active;
    int st = active.Fill(g, keys_dev != nullptr, scratch, stream);
    if (st) return st;
    const int64_t n = active.n;
    *n_out = n;
    if (!keys_dev || n == 0) return O3DMI_OK;
    if (n > capacity) {
        SetLastError("export_blocks: more active blocks than `capacity`");
        return O3DMI_ERR_CAPACITY;
    }
    if ((st = GatherRows(o3dmi_hash_key_buffer(g->block_hashmap), active.idx,
                         n, 12, keys_dev, s)))
        return st;
    const int64_t res = g->block_resolution;
    for (size_t i = 0; i < g->attr_names.size(); ++i) {
        O3DMI_REQUIRE(values_dev[i] != nullptr, "values_dev[i] is null");
        const int64_t row = res * res * res * g->attr_channels[i] *
                            DtypeSize(g->attr_dtypes[i]);
        if ((st = GatherRows(o3dmi_hash_value_buffer(g->block_hashmap, (int)i),
                             active.idx, n, row, values_dev[i], s)))
            return st;
    }
    return O3DMI_OK;
}

int o3dmi_vbg_merge_blocks(o3dmi_vbg_t* g, const int32_t* keys_dev,
                           const void* const* values_dev, int64_t n,
                           o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g != nullptr, "grid is null");
    O3DMI_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return O3DMI_OK;
    O3DMI_REQUIRE(keys_dev && values_dev, "null argument");
    TsdfAttrs at;
    int st = ResolveTsdf(g, &at);
    if (st) return st;
    const int ti = at.ti, wi = at.wi, ci = at.ci;
    O3DMI_REQUIRE(g->attr_dtypes[(size_t)ti] == O3DMI_F32,
                  "tsdf must be Float32");
    O3DMI_REQUIRE((int)g->attr_names.size() ==
                          2 + (ci >= 0 ? 1 : 0),
                  "merge_blocks handles the tsdf / weight / color attributes");
    O3DMI_REQUIRE(ci < 0 || g->attr_channels[(size_t)ci] == 3,
                  "color must have 3 channels");
    O3DMI_REQUIRE(values_dev[ti] && values_dev[wi] &&
                          (ci < 0 || values_dev[ci]),
                  "values_dev[i] is null");
    g->known_valid = false;
    if ((st = EnsureCapacity(g, n, stream))) return st;
    if ((st = EnsureScratch(g, n))) return st;
    if ((st = o3dmi_hash_activate(g->block_hashmap, keys_dev, n, nullptr,
                                  nullptr, nullptr, stream)))
        return st;
    if ((st = o3dmi_hash_find(g->block_hashmap, keys_dev, n, nullptr,
                              g->scratch_buf_indices, nullptr, stream)))
        return st;
    (void)ResolveTsdf(g, &at);  // again: a Reserve above moves the buffers
    const int64_t res = g->block_resolution;
    const int vpb = (int)(res * res * res);
    const int64_t total = n * vpb;
    const int block = 256;
    const int64_t want = (total + block - 1) / block;
    const int grid = (int)(want < 65536 ? want : 65536);
    hipStream_t s = (hipStream_t)stream;
    if (at.grid_dtype == O3DMI_F32)
        MergeBlocksKernel<float><<<grid, block, 0, s>>>(
                g->scratch_buf_indices, total, vpb, at.tsdf, (float*)at.weight,
                (float*)at.color, (const float*)values_dev[ti],
                (const float*)values_dev[wi],
                ci >= 0 ? (const float*)values_dev[ci] : nullptr);
    else
        MergeBlocksKernel<uint16_t><<<grid, block, 0, s>>>(
                g->scratch_buf_indices, total, vpb, at.tsdf,
                (uint16_t*)at.weight, (uint16_t*)at.color,
                (const float*)values_dev[ti],
                (const uint16_t*)values_dev[wi],
                ci >= 0 ? (const uint16_t*)values_dev[ci] : nullptr);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // extern "C"
