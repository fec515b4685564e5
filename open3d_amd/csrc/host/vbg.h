// Private header of the host-side VoxelBlockGrid (host/vbg_*.cpp): the grid
// object and what more than one of its translation units needs.
//   vbg_grid.cpp          the grid object, block / voxel queries, the integrate
//                         entry points and their generic path, surface
//                         extraction, block export / merge
//   vbg_frame_stream.cpp  the frame-stream driver (StreamIntegrate)
//   vbg_sliced.cpp        the sliced multi-rank driver (sliced_path.h)
//   vbg_ray_cast.cpp      the ray-cast drivers
//   vbg_exchange.cpp      the multi-rank block exchanges
//   vbg_io.cpp            NPZ save / load
#pragma once

#include "../common.h"
#include "../stream_path.h"
#include "../sliced_path.h"
#include "../collectives.h"
#include "vbg_last_frame.h"

struct o3dmi_vbg {
    float voxel_size = 0;
    int64_t block_resolution = 0;
    std::vector<std::string> attr_names;
    std::vector<int> attr_dtypes;
    std::vector<int> attr_channels;
    o3dmi_hash_t* block_hashmap = nullptr;
    o3dmi_hash_t* frustum_hashmap = nullptr;  // lazily created (cpp:224-235)
    int64_t frustum_capacity = 0;
    int owner_rank = 0, owner_world = 1;      // block-ownership sharding
    // Host-side upper bound of block_hashmap's Size().
    int64_t size_bound = 0;
    // Device scratch for the frame-stream path.
    int32_t* frame_indices = nullptr;
    int64_t frame_indices_capacity = 0;
    int32_t* frame_count = nullptr;
    int32_t* scratch_buf_indices = nullptr;
    int64_t scratch_capacity = 0;
    int32_t frame_stamp = 0;
    // Pinned read-back of {heap_top, error flags} behind each frame's touch.
    int* size_host = nullptr;
    hipEvent_t size_event = nullptr;
    bool size_event_pending = false;
    // Frame-stream fast path (stream_path.h): double-buffered prepared pixel
    // records and block lists, a ring of 4 device counters and a host-mapped
    // status word written by the integrate role.
    o3dmi::PixelRec* recs[2][o3dmi::kMaxGroup] = {};
    int64_t recs_pixels = 0;
    o3dmi::FrameBlock* lists[2] = {nullptr, nullptr};
    o3dmi::ReadyEntry* ready[2] = {nullptr, nullptr};  // same capacity as the lists
    int* front_tickets = nullptr;               // device int[2][16]
    int64_t lists_capacity = 0;
    int* ring_counters = nullptr;        // device int[4]
    // o3dmi_vbg_ray_cast_dev without a caller's range map: the grid's own,
    // left clean ({lo, hi} in every cell) by the ray cast that consumed it
    float* own_range = nullptr;
    int64_t own_range_cells = 0;
    bool own_range_clean = false;
    float own_range_lo = 0, own_range_hi = 0;
    // ... and, for images whose ray cast runs in rounds, the last cast's
    // per-tile durations and this cast's tile order (longest first)
    unsigned long long* rc_cost = nullptr;
    int* rc_order = nullptr;
    int64_t rc_tiles = 0;
    unsigned rc_seq = 0;
    volatile int* stream_status = nullptr;  // host-mapped int[8]: [0..3]
                                         // published by the integrate roles,
                                         // [4..7] by the groups' last touch
                                         // workgroup (stream_path.h)
    int touch_seen_stamp = 0;            // newest touch status taken in
    int touch_seen_size = 0;
    int stream_overflow = 0;             // stamp of the first group that ran
                                         // out of buffer indices (sticky until
                                         // StreamIntegrate has recovered)
    // What recent groups really added to the map (for the run-ahead policy).
    int recent_new[4] = {0, 0, 0, 0};
    int recent_n = 0;
    int64_t stream_seq = 0;              // groups issued on the fast path
    int known_size = 0;                  // map size after frame `known_stamp`
    int known_stamp = 0;
    bool known_valid = false;            // false after any non-stream activation
    // Prepare-pass tables (stream_path.h PrepTables) and what they were
    // built for.
    int* prep_col = nullptr;
    int* prep_row = nullptr;
    std::vector<int> prep_host;
    double prep_key[24] = {0};
    bool prep_valid = false, prep_div_short = false, prep_identity = false;
    int last_count = 1024;
    // Which path integrated the most recent frame (for
    // o3dmi_vbg_export_last_frame_blocks): 0 none, 1 frame-stream, 2 generic.
    int last_path = 0;
    int64_t last_seq = 0;                // frame-stream group sequence number
    // bench.py measurement hook (o3dmi_vbg_profile_begin/end).
    bool profiling = false;
    std::vector<hipEvent_t> prof_events;  // 2 per frame, around the launch carrying the integrate work
    int prof_frames = 0, prof_max = 0, prof_stride = 1, prof_seen = 0;
    int64_t prof_launch_frames = 0;  // frames carried by the bracketed launches
    int32_t* prof_counts = nullptr;  // device: [prof_max] block-frames, then
                                     // [prof_max] distinct blocks, then
                                     // [prof_max] map size, per launch
    int64_t prof_distinct_blocks = 0;  // of the last profile_end
    // per bracketed launch of the last profile_end (o3dmi_vbg_profile_launches)
    std::vector<float> prof_launch_ms;
    std::vector<int32_t> prof_launch_counts;  // 3 x launches, as prof_counts

    // Sliced block touch (sliced_path.h): block-ownership sharding with the
    // touch split over the ranks. Buffers are per grid; the side stream runs
    // chunk c + 1's touch / exchange / apply while the caller's stream runs
    // chunk c's integrate launches.
    struct Sliced {
        hipStream_t side = nullptr;
        hipEvent_t ev_side[2] = {nullptr, nullptr};  // chunk set ready
        hipEvent_t ev_main[2] = {nullptr, nullptr};  // chunk set consumed
        hipEvent_t ev_enter = nullptr;
        o3dmi::ChunkTable send_table = {}, recv_table = {};
        int table_slots = 0;  // sender table (doubles on every rank alike)
        int recv_slots = 0;   // receiver table (may grow on one rank alone)
        int capacity = 0;  // records of a wire segment
        int world = 0;
        // the ranks' agreed verdict on the proven short divisions for one
        // truncation distance (0 = not asked yet, 1 = all have them, -1 = no)
        float agreed_trunc = 0.0f;
        int agreed_fast_div = 0;
        const void* agreed_comm = nullptr;
        void* send_seg[2] = {nullptr, nullptr};
        void* gathered[2] = {nullptr, nullptr};
        o3dmi::ChunkEntry* entries[2] = {nullptr, nullptr};  // [entries_cap]
        int* entries_count[2] = {nullptr, nullptr};   // device int
        int entries_cap = 0;
        o3dmi::SliceFrame* frames_dev = nullptr;   // touch: pose (inverse extrinsic)
        o3dmi::IntegFrame* iframes_dev = nullptr;  // integrate: extrinsic + images
        int64_t frames_cap = 0;
        std::vector<o3dmi::SliceFrame> frames_host;
        std::vector<o3dmi::IntegFrame> iframes_host;
        // records form: the prepared records of a chunk's frames, two sets of
        // kChunkFrames images of (pixels + 1) records
        o3dmi::PixelRec* chunk_recs[2] = {nullptr, nullptr};
        int64_t chunk_recs_pixels = 0;
        int chunk_recs_frames = 0;  // frames each set holds
        int64_t chunks_done = 0;  // statistics (o3dmi_vbg_sliced_stats)
        int64_t reapplied = 0;
    } sliced;
    int sliced_slots_wanted = 8192;
    // o3dmi_vbg_allgather_owned_blocks has replicated the other ranks' blocks
    // here: a further owner-partitioned merge would send them back to their
    // owners and count their weights again
    bool replicated = false;

    int AttrIndex(const char* name) const {
        for (size_t i = 0; i < attr_names.size(); ++i)
            if (attr_names[i] == name) return (int)i;
        return -1;
    }
};

namespace o3dmi {

// ---- vbg_grid.cpp ------------------------------------------------------------

int DtypeSize(int dt);

// The attributes the TSDF operators read: tsdf, weight and (ci >= 0) colour,
// with the grid dtype of the (weight, colour) pair.
struct TsdfAttrs {
    int ti = -1, wi = -1, ci = -1;
    int grid_dtype = O3DMI_F32;
    float* tsdf = nullptr;
    void* weight = nullptr;
    void* color = nullptr;
};

int ResolveTsdf(o3dmi_vbg* g, TsdfAttrs* a);

// block_hashmap_->GetActiveIndices into the call's pooled scratch; ascending
// when `sorted`, so that what is built from them is a function of the grid
// state only.
struct ActiveList {
    int32_t* idx = nullptr;
    int64_t n = 0;
    int Fill(o3dmi_vbg* g, bool sorted, PoolScratch& scratch,
             o3dmi_stream_t stream) {
        const int64_t cap = o3dmi_hash_capacity(g->block_hashmap);
        int st = scratch.Alloc(&idx, sizeof(int32_t) * (size_t)cap);
        if (st) return st;
        n = 0;
        if ((st = o3dmi_hash_active_indices(g->block_hashmap, idx, stream, &n)))
            return st;
        return sorted ? o3dmi_sort_indices(idx, n, stream) : O3DMI_OK;
    }
};

// ---- vbg_frame_stream.cpp ----------------------------------------------------

// Per-frame inputs of the fast path.
struct StreamFrame {
    const void* depth;
    const void* color;
    const double* extrinsic;
};
struct StreamCommon {
    int depth_rows, depth_cols, color_rows, color_cols;
    const double* depth_intrinsic;
    const double* color_intrinsic;
    float depth_scale, depth_max, trunc;
    int64_t frame_new;  // strict bound on blocks one frame can touch
    int grid_dtype;
    int ti, wi, ci;
    bool with_color;
};

inline StreamCommon MakeCommon(int depth_rows, int depth_cols, int color_rows,
                               int color_cols, const double* depth_intrinsic,
                               const double* color_intrinsic, float depth_scale,
                               float depth_max, float trunc) {
    return {depth_rows,      depth_cols,      color_rows,  color_cols,
            depth_intrinsic, color_intrinsic, depth_scale, depth_max,
            trunc};  // the rest: zero
}

// Frame f of a batch call's arrays (color_devs may be null).
inline std::vector<StreamFrame> MakeFrames(const void* const* depth_devs,
                                           const void* const* color_devs,
                                           const double* extrinsics, int n) {
    std::vector<StreamFrame> frames((size_t)n);
    for (int f = 0; f < n; ++f)
        frames[(size_t)f] = {depth_devs[f], color_devs ? color_devs[f] : nullptr,
                             extrinsics + 16 * (size_t)f};
    return frames;
}

// frames_per_launch of the batch entry points -> frames per integrate launch.
inline int ClampGroup(int frames_per_launch) {
    if (frames_per_launch <= 0) return kDefaultGroup;
    return frames_per_launch > kMaxGroup ? kMaxGroup : frames_per_launch;
}

// Fills c's ti / wi / ci / with_color / grid_dtype for frames[0..n).
inline int ResolveCommon(o3dmi_vbg* g, const StreamFrame* frames, int n,
                         StreamCommon* c) {
    TsdfAttrs at;
    const int st = ResolveTsdf(g, &at);
    if (st) return st;
    c->ti = at.ti;
    c->wi = at.wi;
    c->ci = at.ci;
    c->grid_dtype = at.grid_dtype;
    c->with_color = c->ci >= 0 && (int64_t)c->color_rows * c->color_cols > 0 &&
                    n > 0 && frames[0].color != nullptr;
    return O3DMI_OK;
}

bool StreamPathApplies(const o3dmi_vbg* g, int input_dtype);
int EnsureStreamBuffers(o3dmi_vbg* g, int rows, int cols, int64_t list_cap);
int EnsurePrepTables(o3dmi_vbg* g, const double* dk, const double* ck, int rows,
                     int cols, int crows, int ccols, float depth_scale,
                     hipStream_t s);
int PollStreamStatus(o3dmi_vbg* g, int* overflow = nullptr);
// frames[0..n) strictly in order on stream `s`, `group` (ClampGroup) frames
// per integrate launch.
int StreamIntegrate(o3dmi_vbg* g, const StreamCommon& c0,
                    const StreamFrame* frames, int n, int group, hipStream_t s);

// ---- vbg_sliced.cpp ----------------------------------------------------------

void FreeSliced(o3dmi_vbg* g);
int StreamIntegrateSliced(o3dmi_vbg* g, const StreamCommon& c0,
                          const StreamFrame* frames, int n, int group,
                          hipStream_t s, o3dmi_comm* comm,
                          const void* const* gathered_in);

}  // namespace o3dmi
