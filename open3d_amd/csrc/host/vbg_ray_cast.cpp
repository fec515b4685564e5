// VoxelBlockGrid::RayCast (VoxelBlockGrid.cpp:328-402) on the host-side grid:
// the range map, then the ray cast proper; with a communicator, a band of
// tile rows per rank.

#include "vbg.h"
#include "../raycast.h"

using namespace o3dmi;

extern "C" {

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
                       o3dmi_stream_t stream) {
    return o3dmi_vbg_ray_cast_dev(
            g, block_coords_dev, m, nullptr, intrinsic, extrinsic, width,
            height, range_map_dev, out_depth, out_vertex, out_color, out_normal,
            out_index, out_mask, out_ratio, out_ratio_dx, out_ratio_dy,
            out_ratio_dz, depth_scale, depth_min, depth_max, weight_threshold,
            trunc_voxel_multiplier, range_map_down_factor, stream);
}

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
                           int range_map_down_factor, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && intrinsic && extrinsic, "null argument");
    TsdfAttrs at;
    int st = ResolveTsdf(g, &at);
    if (st) return st;
    O3DMI_REQUIRE(range_map_down_factor > 0 && height >= range_map_down_factor &&
                          width >= range_map_down_factor,
                  "bad image size / down factor");
    // block_coords_dev == NULL: the blocks the last frame-stream integration
    // touched, read straight from the grid's own list (no export launch, no
    // caller-side copy) -- what o3dmi_vbg_last_frame_block_coordinates would
    // hand over.
    int key_stride = 3;
    if (!block_coords_dev) {
        O3DMI_REQUIRE(g->last_path == 1 && g->lists[0] != nullptr,
                      "ray cast without block coordinates: no frame-stream "
                      "integration to take them from "
                      "(o3dmi_vbg_integrate_frame first, or pass the "
                      "coordinates)");
        block_coords_dev = (const int32_t*)g->lists[g->last_seq & 1] + 1;
        m_dev = g->ring_counters + (g->last_seq & 3);
        max_m = g->lists_capacity;
        key_stride = 4;
    }
    // range_map_dev == NULL: the range map is the grid's own scratch (as in
    // the reference, where RayCast allocates it), and the ray cast that
    // consumes it leaves it clean for the next call: no clearing launch per
    // frame.
    int map_is_clean = 0;
    RayCastOptions options = {};
    if (!range_map_dev) {
        const int64_t cells = (int64_t)(height / range_map_down_factor) *
                              (width / range_map_down_factor);
        if (g->own_range_cells != cells) {
            if (g->own_range) {
                O3DMI_HIP_CHECK(hipDeviceSynchronize());
                (void)hipFree(g->own_range);
                g->own_range = nullptr;
            }
            // (+ one cell: the clean state's {lo, hi} for the resetting cast)
            O3DMI_HIP_CHECK(hipMalloc((void**)&g->own_range,
                                      sizeof(float) * 2 * (size_t)(cells + 1)));
            g->own_range_cells = cells;
            g->own_range_clean = false;
        }
        range_map_dev = g->own_range;
        map_is_clean = g->own_range_clean && g->own_range_lo == depth_max &&
                       g->own_range_hi == depth_min;
        // the cast below re-cleans what it reads (8-pixel cells only)
        g->own_range_clean = range_map_down_factor == 8 && (height % 8) == 0 &&
                             (width % 8) == 0;
        g->own_range_lo = depth_max;
        g->own_range_hi = depth_min;
        if (g->own_range_clean) {
            if (!map_is_clean) {
                const float lohi[2] = {depth_max, depth_min};
                O3DMI_HIP_CHECK(hipMemcpyAsync(
                        g->own_range + 2 * cells, lohi, sizeof(lohi),
                        hipMemcpyHostToDevice, (hipStream_t)stream));
            }
            options.reset_range = 1;
        }
        // An image of more tiles than the chip holds workgroups (1280 x 720:
        // 3600 against 1280) is rendered longest tile first, by the last
        // cast's measured tile times (vbg_raycast.hip TileOrder).
        const int64_t n_tiles =
                (int64_t)((width + 31) / 32) * ((height + 7) / 8);
        if (n_tiles > kCUs * 5 && n_tiles <= kCUs * 16 && max_m > 0) {
            if (g->rc_tiles != n_tiles) {
                if (g->rc_cost) {
                    O3DMI_HIP_CHECK(hipDeviceSynchronize());
                    (void)hipFree(g->rc_cost);
                    (void)hipFree(g->rc_order);
                    g->rc_cost = nullptr;
                    g->rc_order = nullptr;
                    g->rc_tiles = 0;
                }
                O3DMI_HIP_CHECK(hipMalloc((void**)&g->rc_cost,
                                          sizeof(unsigned long long) *
                                                  (size_t)n_tiles));
                O3DMI_HIP_CHECK(hipMalloc((void**)&g->rc_order,
                                          sizeof(int) * (size_t)n_tiles));
                O3DMI_HIP_CHECK(hipMemsetAsync(
                        g->rc_cost, 0,
                        sizeof(unsigned long long) * (size_t)n_tiles,
                        (hipStream_t)stream));
                g->rc_tiles = n_tiles;
                g->rc_seq = 0;
            }
            const unsigned last = g->rc_seq;
            g->rc_seq = last + 1 == 0 ? 1 : last + 1;
            options.cost = g->rc_cost;
            options.order = g->rc_order;
            options.n_tiles = (int)n_tiles;
            options.want_seq = last;
            options.seq = g->rc_seq;
        }
    }
    st = o3dmi_internal_estimate_range(
            block_coords_dev, key_stride, max_m, m_dev, range_map_dev,
            map_is_clean, intrinsic, extrinsic, height, width,
            range_map_down_factor, g->block_resolution, g->voxel_size,
            depth_min, depth_max, options, stream);
    if (st) {
        g->own_range_clean = false;
        return st;
    }
    st = o3dmi_internal_raycast_rows(
            g->block_hashmap, at.tsdf, at.weight,
            out_color ? at.color : nullptr, at.grid_dtype, range_map_dev,
            out_depth, out_vertex, out_color, out_normal,
            out_index, out_mask, out_ratio, out_ratio_dx, out_ratio_dy,
            out_ratio_dz, intrinsic, extrinsic, height, width, 0, height,
            (int)g->block_resolution, g->voxel_size, depth_scale, depth_min,
            depth_max, weight_threshold, trunc_voxel_multiplier,
            range_map_down_factor, options, stream);
    if (st) g->own_range_clean = false;
    return st;
}

int o3dmi_vbg_ray_cast_sharded(
        o3dmi_vbg_t* g, const int32_t* block_coords_dev, int64_t m,
        const double* intrinsic, const double* extrinsic, int width, int height,
        float* range_map_dev, float* out_depth, float* out_vertex,
        float* out_color, float* out_normal, float depth_scale, float depth_min,
        float depth_max, float weight_threshold, float trunc_voxel_multiplier,
        int range_map_down_factor, o3dmi_stream_t stream) {
    o3dmi_comm* comm = ThreadComm();
    if (!comm || comm->world <= 1)
        return o3dmi_vbg_ray_cast(
                g, block_coords_dev, m, intrinsic, extrinsic, width, height,
                range_map_dev, out_depth, out_vertex, out_color, out_normal,
                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                depth_scale, depth_min, depth_max, weight_threshold,
                trunc_voxel_multiplier, range_map_down_factor, stream);
    // A collective call: what can fail on one rank alone (arguments, the
    // pool, a launch) is the rank-local stage below, whose status the ranks
    // AGREE on before the first all-gather -- a rank whose stage failed does
    // not leave its peers waiting in a collective it never enters; they
    // return O3DMI_ERR_PEER.
    hipStream_t s = (hipStream_t)stream;
    const int world = comm->world, rank = comm->rank;
    struct Map {
        float* out;
        int channels;
        float* staged;
    } maps[4] = {{out_depth, 1, nullptr},
                 {out_vertex, 3, nullptr},
                 {out_color, 3, nullptr},
                 {out_normal, 3, nullptr}};
    struct Staging {
        hipStream_t s;
        void* p = nullptr;
        ~Staging() {
            if (!p) return;
            (void)hipStreamSynchronize(s);
            PoolFree(p);
        }
    } staging{s};
    int band_rows = 0;
    // ---- rank-local stage: the range map and this rank's band of tile rows,
    // rendered into rows [r0, r1) of maps of `band_rows * world` rows (the
    // kernel addresses pixels of the whole image)
    const auto render_band = [&]() -> int {
        O3DMI_REQUIRE(g && range_map_dev && intrinsic && extrinsic &&
                              width > 0 && height > 0,
                      "bad argument");
        TsdfAttrs at;
        int st = ResolveTsdf(g, &at);
        if (st) return st;
        // the range map is cheap (one pass over the frustum's block keys)
        // and replicated: every rank needs the cells of its band only, but
        // all of it is an output of the call
        if ((st = o3dmi_vbg_estimate_range_dev(
                     block_coords_dev, m, nullptr, range_map_dev, intrinsic,
                     extrinsic, height, width, range_map_down_factor,
                     g->block_resolution, g->voxel_size, depth_min, depth_max,
                     stream)))
            return st;
        const int tiles = (height + 7) / 8;
        const int band_tiles = (tiles + world - 1) / world;
        band_rows = band_tiles * 8;
        const int padded = band_rows * world;  // rows of the gathered maps
        int r0 = rank * band_rows, r1 = r0 + band_rows;
        if (r1 > height) r1 = height;
        // a rank past the last tile row has no band (rows 0..0: the clipped
        // start `height` is no tile boundary when height % 8 != 0)
        if (r0 >= height) r0 = r1 = 0;
        size_t floats = 0;
        for (Map& mp : maps)
            if (mp.out) floats += (size_t)padded * width * mp.channels;
        if (floats == 0) return O3DMI_OK;
        if ((st = PoolAlloc(&staging.p, floats * sizeof(float)))) return st;
        float* q = (float*)staging.p;
        for (Map& mp : maps)
            if (mp.out) {
                mp.staged = q;
                q += (size_t)padded * width * mp.channels;
            }
        return o3dmi_vbg_raycast_rows(
                g->block_hashmap, at.tsdf, at.weight,
                out_color ? at.color : nullptr, at.grid_dtype, range_map_dev, maps[0].staged, maps[1].staged,
                maps[2].staged, maps[3].staged, nullptr, nullptr, nullptr,
                nullptr, nullptr, nullptr, intrinsic, extrinsic, height, width,
                r0, r1, (int)g->block_resolution, g->voxel_size, depth_scale,
                depth_min, depth_max, weight_threshold, trunc_voxel_multiplier,
                range_map_down_factor, stream);
    };
    int st = comm->AgreeStatus(render_band(), s);
    if (st) return st;
    // ---- collective stage: a rank's band is a contiguous run of rows, so
    // the maps are gathered in place; the caller's {height, width, C} maps
    // are their first rows
    for (Map& mp : maps) {
        if (!mp.out) continue;
        const int64_t seg = (int64_t)band_rows * width * mp.channels *
                            (int64_t)sizeof(float);
        if ((st = comm->Allgather((char*)mp.staged + (size_t)seg * rank,
                                  mp.staged, seg, s)))
            return st;
        O3DMI_HIP_CHECK(hipMemcpyAsync(
                mp.out, mp.staged,
                (size_t)height * width * mp.channels * sizeof(float),
                hipMemcpyDeviceToDevice, s));
    }
    return O3DMI_OK;
}

}  // extern "C"
