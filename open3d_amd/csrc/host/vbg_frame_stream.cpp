// The frame-stream driver of the host-side VoxelBlockGrid (StreamIntegrate,
// behind o3dmi_vbg_integrate_frame[s]): groups of frames issued back to back
// on the fast path of stream_path.h, the run-ahead capacity policy, and what
// reads the driver's state (the last frame's block list, bench.py's profiling
// hook).

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "vbg.h"
#include "../preload.h"

using namespace o3dmi;

namespace {

// Block keys of a frame-stream group list -> {n,3} int32, count copied.
__global__ void ExportListKeysKernel(const FrameBlock* __restrict__ list,
                                     const int* __restrict__ count,
                                     int64_t capacity,
                                     int32_t* __restrict__ out_keys,
                                     int32_t* __restrict__ out_count) {
    int64_t n = *count;
    if (n > capacity) n = capacity;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const FrameBlock b = list[i];
        out_keys[3 * i + 0] = b.x;
        out_keys[3 * i + 1] = b.y;
        out_keys[3 * i + 2] = b.z;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = (int32_t)n;
}

// Same from a list of buffer indices (generic path).
__global__ void ExportIndexKeysKernel(const int32_t* __restrict__ indices,
                                      const int* __restrict__ count,
                                      int64_t capacity,
                                      const int32_t* __restrict__ key_buffer,
                                      int32_t* __restrict__ out_keys,
                                      int32_t* __restrict__ out_count) {
    int64_t n = *count;
    if (n > capacity) n = capacity;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* k = key_buffer + 3 * (int64_t)indices[i];
        out_keys[3 * i + 0] = k[0];
        out_keys[3 * i + 1] = k[1];
        out_keys[3 * i + 2] = k[2];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = (int32_t)n;
}

}  // namespace

// ---- run-ahead capacity policy ------------------------------------------------
// HashMap::Activate reserves when Size() + M would pass the capacity
// (HashMap.cpp:166-176), M being the frame's block count, which the reference
// has on the host because it synchronises every frame. The frame stream
// issues groups ahead of the GPU, so neither Size() nor M is known when a
// group is issued. Two bounds:
//   strict   known size + (groups not yet reported + 1) x the frustum bound of
//            a group (FrustumBlockBound per frame): cannot overflow, needs no
//            confirmation. A map with a few hundred thousand blocks of
//            head-room is issued this way, as in rounds 1-3.
//   estimate the same with what recent groups REALLY added (twice the largest
//            of the last four + a margin) in place of the frustum bound. A
//            group issued on the estimate may run out of buffer indices: the
//            device then drops that group and every later one as a whole
//            (InsertKey / the last touch workgroup, vbg_stream.hip), reports
//            the stamp, and StreamIntegrate reserves and replays from the
//            dropped group's first frame. Such groups are CONFIRMED before the
//            call that issued them returns (their frames are only known to be
//            alive until then).
// A Reserve therefore happens when the map really is too small (or, drained,
// when even the estimate does not fit), not because of the frustum bound.
static int64_t EstimatedGroupNew(const o3dmi_vbg* g, int64_t strict) {
    if (g->recent_n == 0) {
        // nothing observed yet (a cold start): an eighth of the free map per
        // group in flight, so that the first groups of a stream pipeline too
        const int64_t room = o3dmi_hash_capacity(g->block_hashmap) -
                             (int64_t)g->known_size;
        const int64_t guess = room / 8 > 1024 ? room / 8 : 1024;
        return guess < strict ? guess : strict;
    }
    int m = 0;
    for (int i = 0; i < 4 && i < g->recent_n; ++i)
        if (g->recent_new[i] > m) m = g->recent_new[i];
    const int64_t est = 2 * (int64_t)m + 64;
    return est < strict ? est : strict;
}

enum class Issue { kStrict, kEstimate, kNo };

// The map size is exact again (stream drained, size read from the map).
static void SetExactSize(o3dmi_vbg* g, int64_t size) {
    g->known_size = (int)size;
    g->known_stamp = g->frame_stamp;
    g->touch_seen_stamp = g->frame_stamp;
    g->touch_seen_size = (int)size;
    g->known_valid = true;
}

// Non-blocking: may one more group be issued behind those in flight?
static Issue StreamMayIssue(o3dmi_vbg* g, int64_t strict_new, bool allow_est,
                            bool may_spin = true) {
    if (!g->known_valid) return Issue::kNo;
    const int64_t capacity = o3dmi_hash_capacity(g->block_hashmap);
    // The host runs ahead of the GPU; when a bound fails only because too
    // many issued groups have not reported their map size yet, give the
    // status words a moment to catch up instead of draining the pipeline.
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        if (PollStreamStatus(g) != O3DMI_OK) return Issue::kNo;  // surfaced later
        if (g->stream_overflow != 0) return Issue::kNo;  // recovery first
        const int64_t unknown = (int64_t)g->frame_stamp - g->known_stamp;
        if ((int64_t)g->known_size + (unknown + 1) * strict_new <= capacity)
            return Issue::kStrict;
        const int64_t est = EstimatedGroupNew(g, strict_new);
        if (allow_est && est < strict_new &&
            (int64_t)g->known_size + (unknown + 1) * est <= capacity)
            return Issue::kEstimate;
        // Even a fully reported pipeline would not fit: the blocking path
        // decides (drained go-ahead or Reserve).
        if ((int64_t)g->known_size + 2 * (allow_est ? est : strict_new) >
            capacity)
            return Issue::kNo;
        if (unknown <= 1 || !may_spin) return Issue::kNo;
        if (std::chrono::steady_clock::now() - t0 >
            std::chrono::microseconds(500))
            return Issue::kNo;
    }
}

// Blocking form, for a group issued with nothing overlapping it: waits until
// every issued group has reported (they complete without the host), then
// applies the policy to the exact size. With `allow_est` a drained map that is
// not full issues the group whatever the bounds say -- the device reports an
// overflow and the caller recovers (Reserve to max(wanted, 2 x capacity), the
// reference's growth rule, then replay).
static int StreamEnsureCapacity(o3dmi_vbg* g, int64_t strict_new,
                                bool allow_est, hipStream_t s, Issue* how,
                                int* overflow) {
    *how = Issue::kStrict;
    int st = PollStreamStatus(g, overflow);
    if (st || *overflow) return st;
    if (!g->known_valid) {
        // Something else activated blocks since the last fast-path group (or
        // this is the first one): take the exact size from the map itself.
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        int64_t size = 0;
        st = o3dmi_hash_size(g->block_hashmap, (o3dmi_stream_t)s, &size);
        if (st) return st;
        SetExactSize(g, size);
        g->recent_n = 0;
    }
    const Issue quick = StreamMayIssue(g, strict_new, allow_est, false);
    if (quick != Issue::kNo) {
        *how = quick;
        return O3DMI_OK;
    }
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    // a group issued on the estimate may have overflowed the map meanwhile:
    // the caller recovers (the map must not be sized or reserved before)
    if ((st = PollStreamStatus(g, overflow)) || *overflow) return st;
    int64_t size = 0;
    st = o3dmi_hash_size(g->block_hashmap, (o3dmi_stream_t)s, &size);
    if (st) return st;
    SetExactSize(g, size);
    const int64_t capacity = o3dmi_hash_capacity(g->block_hashmap);
    // Drained, on the estimate: go unless the map is outright full -- an
    // overflow is recoverable (drop + replay), a Reserve the stream did not
    // need is not. The estimate only decides how far AHEAD groups are issued.
    const int64_t need_new = allow_est ? 1 : strict_new;
    if (size + need_new > capacity) {
        const int64_t need = size + need_new;
        const int64_t target = need > capacity * 2 ? need : capacity * 2;
        st = o3dmi_hash_reserve(g->block_hashmap, target, (o3dmi_stream_t)s);
        if (st) return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    }
    *how = size + strict_new <= o3dmi_hash_capacity(g->block_hashmap)
                   ? Issue::kStrict
                   : Issue::kEstimate;
    return O3DMI_OK;
}

// A group of up to kMaxGroup consecutive frames whose front roles have been
// (or are being) issued.
struct StreamGroup {
    int n = 0;
    int64_t seq = 0;  // group sequence number (selects the scratch buffers)
    int stamp = 0;    // touch / status stamp
    const StreamFrame* frames = nullptr;
};

// Front-role arguments of the frames of a new group; advances the stamp.
static StreamGroup MakeGroup(o3dmi_vbg* g, const StreamCommon& c,
                             const StreamFrame* frames, int n,
                             FrameFrontArgs* fa) {
    StreamGroup grp;
    grp.n = n;
    grp.seq = g->stream_seq;
    g->frame_stamp += 1;
    grp.stamp = g->frame_stamp;
    grp.frames = frames;
    const int par = (int)(grp.seq & 1);
    for (int f = 0; f < n; ++f) {
        FrameFrontArgs& a = fa[f];
        a.depth = (const uint16_t*)frames[f].depth;
        a.color = c.with_color ? (const uint8_t*)frames[f].color : nullptr;
        a.rows = c.depth_rows;
        a.cols = c.depth_cols;
        a.color_rows = c.color_rows;
        a.color_cols = c.color_cols;
        a.depth_intrinsic = c.depth_intrinsic;
        a.color_intrinsic = c.color_intrinsic ? c.color_intrinsic
                                              : c.depth_intrinsic;
        a.extrinsic = frames[f].extrinsic;
        a.resolution = (int)g->block_resolution;
        a.voxel_size = g->voxel_size;
        a.sdf_trunc = g->voxel_size * c.trunc;
        a.depth_scale = c.depth_scale;
        a.depth_max = c.depth_max;
        a.stride = 4;
        a.group_stamp = (unsigned long long)grp.stamp;
        a.group_bit = f;
        a.touch_plane = par;
        a.col_lut = g->prep_valid ? g->prep_col : nullptr;
        a.row_lut = g->prep_valid ? g->prep_row : nullptr;
        a.depth_div_short = g->prep_valid && g->prep_div_short;
        a.prep_identity = g->prep_valid && g->prep_identity;
        a.recs = g->recs[par][f];
        a.list = g->lists[par];
        a.list_capacity = g->lists_capacity;
        a.count = g->ring_counters + (grp.seq & 3);
        a.ready = g->ready[par];
        a.tickets = g->front_tickets + 16 * par;
        a.touch_status = (int*)g->stream_status + 4;
        a.prepare_only = false;
    }
    g->stream_seq += 1;
    g->size_bound = o3dmi_hash_capacity(g->block_hashmap);  // generic path: re-read
    return grp;
}

static void MakeIntegArgs(o3dmi_vbg* g, const StreamCommon& c,
                          const StreamGroup& grp, bool prof,
                          IntegrateStreamArgs* ia) {
    const int par = (int)(grp.seq & 1);
    ia->n_frames = grp.n;
    ia->group_stamp = (unsigned long long)grp.stamp;
    ia->touch_plane = par;
    for (int f = 0; f < grp.n; ++f) {
        ia->recs[f] = g->recs[par][f];
        ia->extrinsic[f] = grp.frames[f].extrinsic;
    }
    ia->rows = c.depth_rows;
    ia->cols = c.depth_cols;
    ia->with_color = c.with_color;
    ia->list = g->lists[par];
    ia->ready = g->ready[par];
    ia->count = g->ring_counters + (grp.seq & 3);
    ia->list_capacity = g->lists_capacity;
    ia->grid_hint = g->last_count;
    ia->tsdf = (float*)o3dmi_hash_value_buffer(g->block_hashmap, c.ti);
    ia->weight = o3dmi_hash_value_buffer(g->block_hashmap, c.wi);
    ia->color = c.with_color ? o3dmi_hash_value_buffer(g->block_hashmap, c.ci)
                             : nullptr;
    ia->grid_dtype = c.grid_dtype;
    ia->depth_intrinsic = c.depth_intrinsic;
    ia->resolution = (int)g->block_resolution;
    ia->voxel_size = g->voxel_size;
    ia->sdf_trunc = g->voxel_size * c.trunc;
    ia->depth_max = c.depth_max;
    ia->depth_scale = c.depth_scale;
    ia->zero_counter = g->ring_counters + ((grp.seq + 2) & 3);
    ia->size_host = (int*)g->stream_status;
    ia->status_stamp = grp.stamp;
    ia->prof_count = prof ? g->prof_counts + g->prof_max + g->prof_frames
                          : nullptr;
    ia->prof_frame_blocks = prof ? g->prof_counts + g->prof_frames : nullptr;
    ia->prof_map_size =
            prof ? g->prof_counts + 2 * g->prof_max + g->prof_frames : nullptr;
}

// Waits (spinning on the host-mapped words; no runtime call) until the touch
// of group `stamp` has reported or `overflow` is set.
static int WaitTouchReported(o3dmi_vbg* g, int stamp, hipStream_t s,
                             int* overflow) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        int st = PollStreamStatus(g, overflow);
        if (st) return st;
        if (*overflow != 0 || g->touch_seen_stamp - stamp >= 0) return O3DMI_OK;
        if (std::chrono::steady_clock::now() - t0 >
            std::chrono::milliseconds(20)) {
            // not a spin any more: let the runtime wait, then read once more
            O3DMI_HIP_CHECK(hipStreamSynchronize(s));
            if ((st = PollStreamStatus(g, overflow))) return st;
            return O3DMI_OK;
        }
    }
}

namespace o3dmi {

int EnsureStreamBuffers(o3dmi_vbg* g, int rows, int cols, int64_t list_cap) {
    const int64_t px = (int64_t)rows * cols;
    if (g->recs_pixels < px) {
        for (int i = 0; i < 2; ++i)
            for (int f = 0; f < kMaxGroup; ++f) {
                (void)hipFree(g->recs[i][f]);
                g->recs[i][f] = nullptr;
                // + 1: the sentinel record behind the image
                O3DMI_HIP_CHECK(hipMalloc((void**)&g->recs[i][f],
                                          sizeof(PixelRec) * (size_t)(px + 1)));
            }
        g->recs_pixels = px;
    }
    if (g->lists_capacity < list_cap) {
        for (int i = 0; i < 2; ++i) {
            (void)hipFree(g->lists[i]);
            g->lists[i] = nullptr;
            O3DMI_HIP_CHECK(hipMalloc((void**)&g->lists[i],
                                      sizeof(FrameBlock) * (size_t)list_cap));
            (void)hipFree(g->ready[i]);
            g->ready[i] = nullptr;
            O3DMI_HIP_CHECK(hipMalloc((void**)&g->ready[i],
                                      sizeof(ReadyEntry) * (size_t)list_cap));
        }
        g->lists_capacity = list_cap;
    }
    if (!g->front_tickets) {
        O3DMI_HIP_CHECK(hipMalloc((void**)&g->front_tickets, sizeof(int) * 32));
        O3DMI_HIP_CHECK(hipMemset(g->front_tickets, 0, sizeof(int) * 32));
    }
    if (!g->ring_counters) {
        O3DMI_HIP_CHECK(hipMalloc((void**)&g->ring_counters, sizeof(int) * 4));
        O3DMI_HIP_CHECK(hipMemset(g->ring_counters, 0, sizeof(int) * 4));
        int* st = nullptr;
        O3DMI_HIP_CHECK(hipHostMalloc((void**)&st, sizeof(int) * 8,
                                      hipHostMallocMapped |
                                              hipHostMallocCoherent));
        for (int i = 0; i < 8; ++i) st[i] = 0;
        g->stream_status = st;
    }
    return O3DMI_OK;
}

// Builds / re-uses the prepare-pass tables for this image geometry.
int EnsurePrepTables(o3dmi_vbg* g, const double* dk, const double* ck, int rows,
                     int cols, int crows, int ccols, float depth_scale,
                     hipStream_t s) {
    double key[24] = {0};
    for (int i = 0; i < 9; ++i) key[i] = dk[i];
    for (int i = 0; i < 9; ++i) key[9 + i] = (ck ? ck : dk)[i];
    key[18] = rows; key[19] = cols; key[20] = crows; key[21] = ccols;
    key[22] = depth_scale;
    if (g->prep_valid && std::memcmp(key, g->prep_key, sizeof(key)) == 0)
        return O3DMI_OK;
    // the previous tables may still be read by launches in flight
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    (void)hipFree(g->prep_col);
    g->prep_col = g->prep_row = nullptr;
    g->prep_valid = false;
    O3DMI_HIP_CHECK(hipMalloc((void**)&g->prep_col,
                              sizeof(int) * (size_t)(rows + cols)));
    g->prep_row = g->prep_col + cols;
    g->prep_host.assign((size_t)(rows + cols), -1);
    g->prep_div_short =
            PrepTables(dk, ck, rows, cols, crows, ccols, depth_scale,
                       g->prep_host.data(), g->prep_host.data() + cols);
    g->prep_identity = crows == rows && ccols == cols;
    for (int u = 0; u < cols && g->prep_identity; ++u)
        g->prep_identity = g->prep_host[(size_t)u] == u;
    for (int v = 0; v < rows && g->prep_identity; ++v)
        g->prep_identity = g->prep_host[(size_t)cols + (size_t)v] == v;
    O3DMI_HIP_CHECK(hipMemcpyAsync(g->prep_col, g->prep_host.data(),
                                   sizeof(int) * (size_t)(rows + cols),
                                   hipMemcpyHostToDevice, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(g->prep_key, key, sizeof(key));
    g->prep_valid = true;
    return O3DMI_OK;
}

// Reads the status words the device publishes -- by every integrate role as
// its first action ({map size, error flags, group block count, stamp}) and by
// the last touch workgroup of every group ({map size after the group's touch,
// overflow stamp, group block count, stamp}); never blocks. `overflow` (may be
// null) receives the stamp of the first group that ran out of buffer indices,
// 0 when none did.
int PollStreamStatus(o3dmi_vbg* g, int* overflow) {
    const volatile int* ts = g->stream_status + 4;
    const int tstamp = __atomic_load_n((const int*)&ts[3], __ATOMIC_ACQUIRE);
    if (tstamp - g->touch_seen_stamp > 0) {
        const int size = ts[0], ovf = ts[1];
        const int tstamp2 =
                __atomic_load_n((const int*)&ts[3], __ATOMIC_ACQUIRE);
        if (tstamp2 == tstamp) {
            // what the groups since the last word seen added, per group
            const int groups = tstamp - g->touch_seen_stamp;
            if (size >= g->touch_seen_size && g->known_valid) {
                const int per = (size - g->touch_seen_size + groups - 1) / groups;
                g->recent_new[g->recent_n++ & 3] = per;
            }
            g->touch_seen_stamp = tstamp;
            g->touch_seen_size = size;
            if (tstamp - g->known_stamp > 0) {
                g->known_size = size;
                g->known_stamp = tstamp;
            }
            if (ovf != 0 && g->stream_overflow == 0) g->stream_overflow = ovf;
        }
    }
    if (overflow) *overflow = g->stream_overflow;
    const int stamp = __atomic_load_n((const int*)&g->stream_status[3],
                                      __ATOMIC_ACQUIRE);
    if (stamp != g->known_stamp && stamp != 0) {
        const int size = g->stream_status[0];
        const int err = g->stream_status[1];
        const int count = g->stream_status[2];
        // Re-check the stamp: a newer group may have overwritten the words.
        const int stamp2 = __atomic_load_n((const int*)&g->stream_status[3],
                                           __ATOMIC_ACQUIRE);
        if (stamp2 == stamp) {
            if (stamp - g->known_stamp > 0) {
                g->known_size = size < o3dmi_hash_capacity(g->block_hashmap)
                                        ? size
                                        : (int)o3dmi_hash_capacity(
                                                  g->block_hashmap);
                g->known_stamp = stamp;
            }
            g->last_count = count;
        }
        if (err & kErrKeyRange) {
            SetLastError("block coordinate outside +-2^20");
            return O3DMI_ERR_KEY_RANGE;
        }
        if (err & kErrCapacity) {
            SetLastError("hash map capacity exceeded");
            return O3DMI_ERR_CAPACITY;
        }
        if (err & (kErrTouchStamp | kErrProbe)) {
            SetLastError(err & kErrProbe
                                 ? "hash map probe sequence wrapped"
                                 : "frame-stream touch word of another group");
            return O3DMI_ERR_INTERNAL;
        }
    }
    return O3DMI_OK;
}

bool StreamPathApplies(const o3dmi_vbg* g, int input_dtype) {
    int ti = g->AttrIndex("tsdf"), wi = g->AttrIndex("weight");
    return input_dtype == O3DMI_U16 && (g->block_resolution % 4) == 0 &&
           ti >= 0 && wi >= 0 && g->attr_dtypes[(size_t)ti] == O3DMI_F32;
}

// Integrates frames[0..n) strictly in order on stream `s`, `group` frames per
// integrate launch (in [1, kMaxGroup]: ClampGroup). The front roles of group
// k+1 share the launch of group k's integrate role whenever the capacity
// policy allows it without waiting.
int StreamIntegrate(o3dmi_vbg* g, const StreamCommon& c0,
                    const StreamFrame* frames, int n, int group,
                    hipStream_t s) {
    StreamCommon c = c0;
    c.frame_new = FrustumBlockBound(
            c.depth_intrinsic, c.depth_rows, c.depth_cols, c.depth_max,
            g->voxel_size * (float)g->block_resolution, 4);
    O3DMI_REQUIRE(c.frame_new > 0, "depth image too small");
    const int64_t group_new = c.frame_new * group;
    int st = ResolveCommon(g, frames, n, &c);
    if (st) return st;
    if ((st = EnsureStreamBuffers(g, c.depth_rows, c.depth_cols,
                                  c.frame_new * kMaxGroup)))
        return st;

    if ((st = EnsurePrepTables(g, c.depth_intrinsic, c.color_intrinsic,
                                      c.depth_rows, c.depth_cols,
                                      c.color_rows, c.color_cols,
                                      c.depth_scale, s))) {
        return st;
    }
    // The short division forms are proven asynchronously (vbg_stream.hip); a
    // batch call never waits for the proof (its launches take the IEEE forms
    // until it is over). A ONE-frame call is the interactive API -- a loop of
    // them is latency-bound and would run beside the proof's kernels for its
    // first ~10 ms: there the (one-time) wait is taken up front, as rounds 1-3
    // did for every caller.
    (void)PrefetchFastDivision(g->voxel_size * c.trunc, n == 1);
    // O3DMI_STRICT_CAPACITY=1 (A / B): rounds 1-3's policy, the frustum bound
    // only. Groups on the estimate need more than one frame per call to pay
    // (the confirmation is a wait).
    static const bool strict_only =
            std::getenv("O3DMI_STRICT_CAPACITY") != nullptr;
    const bool allow_est = !strict_only && n > 1;

    // Groups issued on the estimate and not yet confirmed: {stamp, first
    // frame}. All of them belong to this call.
    struct Pending {
        int stamp, f0;
    };
    std::vector<Pending> pending;
    bool issued = false;  // front roles of `cur` already in flight
    StreamGroup cur;
    FrameFrontArgs fa[kMaxGroup];
    int f = 0;
    for (;;) {
        int overflow = 0;
        while (f < n && overflow == 0) {
            if (!issued) {
                Issue how;
                if ((st = StreamEnsureCapacity(g, group_new, allow_est, s,
                                               &how, &overflow)))
                    return st;
                if (overflow != 0) break;
                const int m = n - f < group ? n - f : group;
                cur = MakeGroup(g, c, frames + f, m, fa);
                if (how == Issue::kEstimate)
                    pending.push_back({cur.stamp, f});
                if ((st = LaunchFrameStep(g->block_hashmap, fa, m, nullptr, s)))
                    return st;
            }
            g->last_path = 1;
            g->last_seq = cur.seq;
            const int next_f = f + cur.n;
            const bool prof = g->profiling && g->prof_frames < g->prof_max &&
                              g->prof_stride > 0 &&
                              (g->prof_seen++ % g->prof_stride) == 0;
            hipEvent_t* pe = prof ? &g->prof_events[(size_t)g->prof_frames * 2]
                                  : nullptr;
            IntegrateStreamArgs ia;
            MakeIntegArgs(g, c, cur, prof, &ia);
            StreamGroup nxt;
            // O3DMI_NO_FUSE=1 (diagnostics): front roles in their own launches
            // so that a kernel trace shows the two roles separately.
            static const bool no_fuse = std::getenv("O3DMI_NO_FUSE") != nullptr;
            Issue how = Issue::kNo;
            if (!no_fuse && next_f < n)
                how = StreamMayIssue(g, group_new, allow_est);
            const bool fuse = how != Issue::kNo;
            int m = 0;
            if (fuse) {
                m = n - next_f < group ? n - next_f : group;
                nxt = MakeGroup(g, c, frames + next_f, m, fa);
                if (how == Issue::kEstimate)
                    pending.push_back({nxt.stamp, next_f});
            }
            if (pe) O3DMI_HIP_CHECK(hipEventRecord(pe[0], s));
            if ((st = LaunchFrameStep(g->block_hashmap, fuse ? fa : nullptr, m,
                                      &ia, s)))
                return st;
            if (pe) {
                O3DMI_HIP_CHECK(hipEventRecord(pe[1], s));
                g->prof_launch_frames += cur.n;
                g->prof_frames += 1;
            }
            issued = fuse;
            if (fuse) cur = nxt;
            f = next_f;
            // confirmations that have arrived (never waits)
            if (!pending.empty()) {
                if ((st = PollStreamStatus(g, &overflow))) return st;
                while (!pending.empty() && overflow == 0 &&
                       g->touch_seen_stamp - pending.front().stamp >= 0)
                    pending.erase(pending.begin());
            }
        }
        // Every group issued on the estimate is confirmed before the call
        // returns: its touch reports from inside the launch BEFORE the one
        // that integrates it, so this wait ends while that launch is still
        // queued or running -- the GPU does not go idle over it.
        if (overflow == 0 && !pending.empty())
            if ((st = WaitTouchReported(g, pending.back().stamp, s, &overflow)))
                return st;
        if (overflow == 0) break;
        // A group ran out of buffer indices: it and every later group were
        // dropped on the device. Drain, make the map consistent, reserve,
        // replay from the dropped group's first frame.
        int replay_from = -1;
        for (const Pending& pg : pending)
            if (pg.stamp == overflow) replay_from = pg.f0;
        if (replay_from < 0) {
            // An overflow stamp of a group this call issued on the STRICT
            // bound (or a one-frame call): a probe wrap recorded as an
            // overflow (touch_device.h). Nothing to replay from -- but the map
            // must not stay in the "overflow not recovered" state, in which
            // every later size / export / reserve call is refused: recover
            // the slots, rebuild the crowded table, then report.
            (void)hipStreamSynchronize(s);
            int64_t w = 0;
            (void)RecoverOverflow(g->block_hashmap, s, &w);
            (void)hipMemsetAsync(g->ring_counters, 0, sizeof(int) * 4, s);
            (void)hipMemsetAsync(g->front_tickets, 0, sizeof(int) * 32, s);
            const int64_t cap = o3dmi_hash_capacity(g->block_hashmap);
            (void)o3dmi_hash_reserve(g->block_hashmap, w > cap ? w : cap,
                                     (o3dmi_stream_t)s);
            (void)hipStreamSynchronize(s);
            g->stream_overflow = 0;
            g->known_valid = false;
            SetLastError("frame stream: overflow reported for a group this "
                         "call did not issue on an estimate (hash table probe "
                         "sequence wrapped); the map was recovered, the "
                         "call's remaining frames were not integrated");
            return O3DMI_ERR_INTERNAL;
        }
        int64_t wanted = 0;
        if ((st = RecoverOverflow(g->block_hashmap, s, &wanted))) return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(g->ring_counters, 0, sizeof(int) * 4, s));
        O3DMI_HIP_CHECK(hipMemsetAsync(g->front_tickets, 0, sizeof(int) * 32, s));
        const int64_t capacity = o3dmi_hash_capacity(g->block_hashmap);
        const int64_t target = wanted > capacity * 2 ? wanted : capacity * 2;
        if ((st = o3dmi_hash_reserve(g->block_hashmap, target,
                                     (o3dmi_stream_t)s)))
            return st;
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        int64_t size = 0;
        if ((st = o3dmi_hash_size(g->block_hashmap, (o3dmi_stream_t)s, &size)))
            return st;
        SetExactSize(g, size);
        g->stream_overflow = 0;
        pending.clear();
        issued = false;
        f = replay_from;
    }
    return O3DMI_OK;
}

// o3dmi_preload: this translation unit's code object (the export kernels run
// in a tracked frame).
int PreloadStreamDriver() {
    return LoadCodeObjectOf(
            reinterpret_cast<const void*>(&ExportListKeysKernel));
}

}  // namespace o3dmi

extern "C" {

int o3dmi_vbg_export_last_frame_blocks(o3dmi_vbg_t* g, int32_t* out_keys_dev,
                                       int64_t out_capacity,
                                       int32_t* out_count_dev,
                                       o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && out_keys_dev && out_count_dev, "null argument");
    O3DMI_REQUIRE(g->last_path != 0, "no frame has been integrated");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(64), block(kBlock);
    if (g->last_path == 1) {
        const int64_t cap = out_capacity < g->lists_capacity ? out_capacity
                                                            : g->lists_capacity;
        hipLaunchKernelGGL(ExportListKeysKernel, grid, block, 0, s,
                           g->lists[g->last_seq & 1],
                           g->ring_counters + (g->last_seq & 3), cap,
                           out_keys_dev, out_count_dev);
    } else {
        const int64_t cap = out_capacity < g->frame_indices_capacity
                                    ? out_capacity
                                    : g->frame_indices_capacity;
        hipLaunchKernelGGL(ExportIndexKeysKernel, grid, block, 0, s,
                           g->frame_indices, g->frame_count, cap,
                           o3dmi_hash_key_buffer(g->block_hashmap),
                           out_keys_dev, out_count_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int o3dmi_vbg_last_frame_block_coordinates(o3dmi_vbg_t* g,
                                           int32_t* out_coords_dev,
                                           int64_t capacity,
                                           int32_t* out_count_dev,
                                           o3dmi_stream_t stream) {
    O3DMI_REQUIRE(capacity > 0, "capacity must be positive");
    return o3dmi_vbg_export_last_frame_blocks(g, out_coords_dev, capacity,
                                              out_count_dev, stream);
}

int o3dmi_vbg_profile_begin(o3dmi_vbg_t* g, int max_frames, int stride) {
    O3DMI_REQUIRE(g && max_frames > 0 && stride >= 0, "bad argument");
    g->prof_stride = stride;
    g->prof_seen = 0;
    while ((int)g->prof_events.size() < max_frames * 2) {
        hipEvent_t e;
        O3DMI_HIP_CHECK(hipEventCreate(&e));
        g->prof_events.push_back(e);
    }
    if (g->prof_max < max_frames || !g->prof_counts) {
        (void)hipFree(g->prof_counts);
        g->prof_counts = nullptr;
        O3DMI_HIP_CHECK(hipMalloc((void**)&g->prof_counts,
                                  sizeof(int32_t) * 3 * (size_t)max_frames));
    }
    O3DMI_HIP_CHECK(hipMemset(g->prof_counts, 0,
                              sizeof(int32_t) * 3 * (size_t)max_frames));
    g->prof_max = max_frames;
    g->prof_frames = 0;
    g->prof_launch_frames = 0;
    g->profiling = true;
    return O3DMI_OK;
}

int o3dmi_vbg_profile_end(o3dmi_vbg_t* g, o3dmi_stream_t stream,
                          double* integrate_ms, int64_t* launches,
                          int64_t* block_frames, int64_t* frames) {
    O3DMI_REQUIRE(g && integrate_ms && launches && block_frames && frames,
                  "null argument");
    g->profiling = false;
    O3DMI_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    double ti = 0;
    g->prof_launch_ms.assign((size_t)g->prof_frames, 0.0f);
    for (int f = 0; f < g->prof_frames; ++f) {
        float ms = 0;
        O3DMI_HIP_CHECK(hipEventElapsedTime(
                &ms, g->prof_events[(size_t)f * 2 + 0],
                g->prof_events[(size_t)f * 2 + 1]));
        ti += ms;
        g->prof_launch_ms[(size_t)f] = ms;
    }
    g->prof_launch_counts.assign(3 * (size_t)g->prof_frames, 0);
    for (int k = 0; k < 3 && g->prof_frames > 0; ++k)
        O3DMI_HIP_CHECK(hipMemcpy(
                g->prof_launch_counts.data() + (size_t)k * g->prof_frames,
                g->prof_counts + (size_t)k * g->prof_max,
                sizeof(int32_t) * (size_t)g->prof_frames,
                hipMemcpyDeviceToHost));
    std::vector<int32_t> counts((size_t)g->prof_frames);
    if (g->prof_frames > 0)
        O3DMI_HIP_CHECK(hipMemcpy(counts.data(), g->prof_counts,
                                  sizeof(int32_t) * (size_t)g->prof_frames,
                                  hipMemcpyDeviceToHost));
    int64_t bf = 0;
    for (int32_t c : counts) bf += c;
    if (g->prof_frames > 0)
        O3DMI_HIP_CHECK(hipMemcpy(counts.data(), g->prof_counts + g->prof_max,
                                  sizeof(int32_t) * (size_t)g->prof_frames,
                                  hipMemcpyDeviceToHost));
    g->prof_distinct_blocks = 0;
    for (int32_t c : counts) g->prof_distinct_blocks += c;
    *integrate_ms = ti;
    *launches = g->prof_frames;
    *block_frames = bf;
    *frames = g->prof_launch_frames;
    return O3DMI_OK;
}

int64_t o3dmi_vbg_profile_distinct_blocks(const o3dmi_vbg_t* g) {
    return g ? g->prof_distinct_blocks : 0;
}

int64_t o3dmi_vbg_profile_launches(const o3dmi_vbg_t* g, int64_t capacity,
                                   float* ms, int32_t* block_frames,
                                   int32_t* distinct_blocks,
                                   int32_t* map_size) {
    if (!g) return 0;
    const int64_t n = (int64_t)g->prof_launch_ms.size();
    const int64_t m = n < capacity ? n : capacity;
    for (int64_t i = 0; i < m; ++i) {
        if (ms) ms[i] = g->prof_launch_ms[(size_t)i];
        if (block_frames) block_frames[i] = g->prof_launch_counts[(size_t)i];
        if (distinct_blocks)
            distinct_blocks[i] = g->prof_launch_counts[(size_t)(n + i)];
        if (map_size) map_size[i] = g->prof_launch_counts[(size_t)(2 * n + i)];
    }
    return n;
}

}  // extern "C"
