// The sliced multi-rank driver of the host-side VoxelBlockGrid (block-ownership
// sharding, sliced_path.h): the touch split over the ranks, the candidate keys
// all-gathered per chunk of frames, a chunk integrate launch per rank.

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "vbg.h"

using namespace o3dmi;

// Buffers for `world` ranks, `capacity` records per wire segment and chunk
// tables of `slots` slots. Growing frees and re-creates everything (the
// streams are drained first).
static int EnsureSliced(o3dmi_vbg* g, int world, int capacity, int slots,
                        hipStream_t s) {
    o3dmi_vbg::Sliced& z = g->sliced;
    if (z.side && z.world >= world && z.capacity >= capacity &&
        z.table_slots >= slots)
        return O3DMI_OK;
    if (z.side) O3DMI_HIP_CHECK(hipDeviceSynchronize());
    if (world < z.world) world = z.world;
    if (capacity < z.capacity) capacity = z.capacity;
    if (slots < z.table_slots) slots = z.table_slots;
    SliceFrame* keep_frames = z.frames_dev;
    IntegFrame* keep_iframes = z.iframes_dev;
    const int64_t keep_cap = z.frames_cap;
    const int64_t keep_chunks = z.chunks_done, keep_re = z.reapplied;
    const int keep_recv_slots = z.recv_slots;
    PixelRec* keep_recs[2] = {z.chunk_recs[0], z.chunk_recs[1]};
    const int64_t keep_px = z.chunk_recs_pixels;
    const int keep_recs_frames = z.chunk_recs_frames;
    z.frames_dev = nullptr;
    z.iframes_dev = nullptr;
    z.chunk_recs[0] = z.chunk_recs[1] = nullptr;
    FreeSliced(g);
    z.frames_dev = keep_frames;
    z.iframes_dev = keep_iframes;
    z.frames_cap = keep_cap;
    z.chunk_recs[0] = keep_recs[0];
    z.chunk_recs[1] = keep_recs[1];
    z.chunk_recs_pixels = keep_px;
    z.chunk_recs_frames = keep_recs_frames;
    z.chunks_done = keep_chunks;
    z.reapplied = keep_re;
    O3DMI_HIP_CHECK(hipStreamCreateWithFlags(&z.side, hipStreamNonBlocking));
    const int64_t seg = SliceSegmentBytes(capacity);
    for (int i = 0; i < 2; ++i) {
        O3DMI_HIP_CHECK(hipEventCreateWithFlags(&z.ev_side[i],
                                                hipEventDisableTiming));
        O3DMI_HIP_CHECK(hipEventCreateWithFlags(&z.ev_main[i],
                                                hipEventDisableTiming));
        O3DMI_HIP_CHECK(hipMalloc(&z.send_seg[i], (size_t)seg));
        O3DMI_HIP_CHECK(hipMalloc(&z.gathered[i], (size_t)seg * world));
        O3DMI_HIP_CHECK(hipMalloc(
                (void**)&z.entries[i],
                sizeof(ChunkEntry) *
                        (size_t)((keep_recv_slots > slots ? keep_recv_slots
                                                          : slots) / 2)));
        O3DMI_HIP_CHECK(hipMalloc((void**)&z.entries_count[i], sizeof(int)));
        O3DMI_HIP_CHECK(hipMemsetAsync(z.entries_count[i], 0, sizeof(int),
                                       z.side));
    }
    O3DMI_HIP_CHECK(hipEventCreateWithFlags(&z.ev_enter, hipEventDisableTiming));
    int st;
    const int recv_slots = keep_recv_slots > slots ? keep_recv_slots : slots;
    if ((st = AllocChunkTable(&z.send_table, slots, false, z.side))) return st;
    if ((st = AllocChunkTable(&z.recv_table, recv_slots, true, z.side)))
        return st;
    z.table_slots = slots;
    z.recv_slots = recv_slots;
    z.entries_cap = recv_slots / 2;
    z.capacity = capacity;
    z.world = world;
    O3DMI_HIP_CHECK(hipStreamSynchronize(z.side));
    return O3DMI_OK;
}

// Per-frame tables of the side-stream touch (pose as TouchParams keeps it) and
// of the chunk integrate launch (extrinsic as Camera::Make keeps it, images).
static int UploadSliceFrames(o3dmi_vbg* g, const StreamCommon& c,
                             const StreamFrame* frames, int n,
                             TouchParams* shared, int chunk_frames = 0) {
    o3dmi_vbg::Sliced& z = g->sliced;
    if (z.frames_cap < n) {
        if (z.frames_dev) O3DMI_HIP_CHECK(hipDeviceSynchronize());
        (void)hipFree(z.frames_dev);
        (void)hipFree(z.iframes_dev);
        z.frames_dev = nullptr;
        z.iframes_dev = nullptr;
        int64_t cap = 256;
        while (cap < n) cap <<= 1;
        O3DMI_HIP_CHECK(hipMalloc((void**)&z.frames_dev,
                                  sizeof(SliceFrame) * (size_t)cap));
        O3DMI_HIP_CHECK(hipMalloc((void**)&z.iframes_dev,
                                  sizeof(IntegFrame) * (size_t)cap));
        z.frames_cap = cap;
    }
    z.frames_host.resize((size_t)n);
    z.iframes_host.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
        const TouchParams tp = MakeTouchParams(
                c.depth_intrinsic, frames[f].extrinsic, c.depth_rows,
                c.depth_cols, 4, (int)g->block_resolution, g->voxel_size,
                g->voxel_size * c.trunc, c.depth_scale, c.depth_max);
        std::memcpy(z.frames_host[(size_t)f].pose, tp.cam.e,
                    sizeof(z.frames_host[(size_t)f].pose));
        z.frames_host[(size_t)f].depth = (const uint16_t*)frames[f].depth;
        if (f == 0) *shared = tp;
        const Camera cf = Camera::Make(c.depth_intrinsic, frames[f].extrinsic,
                                       g->voxel_size);
        std::memcpy(z.iframes_host[(size_t)f].ext, cf.e,
                    sizeof(z.iframes_host[(size_t)f].ext));
        z.iframes_host[(size_t)f].depth = (const uint16_t*)frames[f].depth;
        z.iframes_host[(size_t)f].color =
                c.with_color ? (const uint8_t*)frames[f].color : nullptr;
        // records form: frame f = slot f % chunk of chunk set (f / chunk) & 1
        z.iframes_host[(size_t)f].recs =
                (chunk_frames > 0 && z.chunk_recs[0])
                        ? z.chunk_recs[(f / chunk_frames) & 1] +
                                  (size_t)(f % chunk_frames) *
                                          (size_t)(z.chunk_recs_pixels + 1)
                        : nullptr;
        z.iframes_host[(size_t)f].pad = nullptr;
    }
    // Synchronous copies: the tables are free (every launch of the previous
    // call that reads them has completed: the touch launches were waited for
    // through their chunk status, the integrate launches by the wait below)
    // and complete before the first launch of this call is issued.
    O3DMI_HIP_CHECK(hipMemcpy(z.frames_dev, z.frames_host.data(),
                              sizeof(SliceFrame) * (size_t)n,
                              hipMemcpyHostToDevice));
    O3DMI_HIP_CHECK(hipMemcpy(z.iframes_dev, z.iframes_host.data(),
                              sizeof(IntegFrame) * (size_t)n,
                              hipMemcpyHostToDevice));
    return O3DMI_OK;
}

// What a chunk's apply reported (host-mapped words 4..7 of stream_status).
struct ChunkStatus {
    int map_size, overflow, blocks;
};
static int WaitChunkStatus(o3dmi_vbg* g, int stamp, hipStream_t side,
                           ChunkStatus* out) {
    const volatile int* ts = g->stream_status + 4;
    const auto t0 = std::chrono::steady_clock::now();
    bool synced = false;
    for (;;) {
        if (__atomic_load_n((const int*)&ts[3], __ATOMIC_ACQUIRE) == stamp) {
            out->map_size = ts[0];
            out->overflow = ts[1];
            out->blocks = ts[2];
            return O3DMI_OK;
        }
        if (synced) {
            SetLastError("sliced touch: the chunk's apply never reported");
            return O3DMI_ERR_INTERNAL;
        }
        if (std::chrono::steady_clock::now() - t0 >
            std::chrono::milliseconds(50)) {
            O3DMI_HIP_CHECK(hipStreamSynchronize(side));
            synced = true;
        }
    }
}

// How far a call of the sliced path got with its collectives: what an error
// exit needs to leave the other ranks in step (StreamIntegrateSliced).
struct SlicedProgress {
    int n_chunks = 0;
    int first_gathers = 0;  // chunks whose FIRST all-gather was issued (the
                            // redo of a chunk is collective by construction:
                            // every rank reads the same gathered headers)
    bool left_in_step = false;  // the error exit was agreed on by all ranks
                                // (o3dmi_comm::AgreeStatus): nobody waits in
                                // an all-gather, no abort segment to send
};

// The frames of one call through the sliced path, `group` (in [1, kMaxGroup]:
// ClampGroup) per integrate launch. `gathered_in`: per chunk the
// `world` wire segments of all ranks (emulation / tests: the stand-in for the
// all-gather; the own segment is replaced by the one computed here), or null:
// all-gather over `comm`.
static int StreamIntegrateSlicedBody(o3dmi_vbg* g, const StreamCommon& c0,
                                     const StreamFrame* frames, int n,
                                     int group, hipStream_t s, o3dmi_comm* comm,
                                     const void* const* gathered_in,
                                     SlicedProgress* progress) {
    StreamCommon c = c0;
    const int world = g->owner_world, rank = g->owner_rank;
    O3DMI_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad ownership");
    O3DMI_REQUIRE(!comm || (comm->world == world && comm->rank == rank),
                  "sliced touch: the communicator's rank / world differ from "
                  "the grid's block ownership");
    // Everything rank-local in front of the first all-gather -- argument
    // checks that depend on this rank's grid, buffers, tables, the frame-table
    // upload -- runs as ONE stage whose status the ranks agree on (ADVICE r5:
    // a rank whose hipMalloc failed here used to return with no all-gather
    // issued, and its peers waited in chunk 0's for ever).
    int st;
    o3dmi_vbg::Sliced& z = g->sliced;
    bool raw_form = false;
    int chunk_frames = 0;
    TouchParams shared;
    auto setup = [&]() -> int {
    int st = ResolveCommon(g, frames, n, &c);
    if (st) return st;
    O3DMI_REQUIRE((c.depth_cols % 4) == 0 &&
                          (!c.with_color || (c.color_rows == c.depth_rows &&
                                             c.color_cols == c.depth_cols)),
                  "sliced touch needs depth and colour images of one size "
                  "(width % 4 == 0)");
    // status words, depth-division verdict (PrepTables) for this depth scale
    if ((st = EnsureStreamBuffers(g, c.depth_rows, c.depth_cols, 1024)))
        return st;
    if ((st = EnsurePrepTables(g, c.depth_intrinsic, c.color_intrinsic,
                               c.depth_rows, c.depth_cols, c.color_rows,
                               c.color_cols, c.depth_scale, s)))
        return st;
    O3DMI_REQUIRE(!c.with_color || g->prep_identity ||
                          !(std::getenv("O3DMI_SLICED_RAW") &&
                            std::getenv("O3DMI_SLICED_RAW")[0] == '1'),
                  "sliced touch, raw form, needs the same intrinsics for depth "
                  "and colour");
    // Sizes: a rank's band sees about 1 / world of a chunk's blocks plus the
    // band's rim; start from a generous guess and double on overflow (every
    // rank reads the same headers, so every rank doubles together).
    if ((st = EnsureSliced(g, world, z.capacity ? z.capacity : 4096,
                           z.table_slots ? z.table_slots
                                         : g->sliced_slots_wanted,
                           s)))
        return st;

    // Two forms of the chunk's integrate launch (same results):
    //   records  the per-pixel prepare pass of the chunk's frames runs on the
    //           side stream (every rank prepares every pixel: 4.3 MB of
    //           traffic per frame, replicated); the launch gathers one 8-byte
    //           record per voxel and frame, as the single-GPU stream does
    //   raw     no prepare pass and no record buffers (2 x 256 images of
    //           8 B / pixel); the launch gathers depth and colour separately
    //           and divides per voxel: 1 088 instead of 877 VALU instructions
    //           per 4 frames
    // Emulated shares (profiles/r4zb_emu_*, r4zg_emu_*; work list longest
    // first, compact lane map): records is ahead at 2 ranks (207 k frames/s
    // against 175 k), raw from 4 on, where the replicated prepare pass weighs
    // as much as a rank's share of the voxel work (328 k against 296 k at 4,
    // 527 k against 413 k at 8). O3DMI_SLICED_RAW=0 / 1 picks one (read per
    // call: tests switch it).
    const char* raw_env = std::getenv("O3DMI_SLICED_RAW");
    raw_form = raw_env ? raw_env[0] == '1'
                       : (world >= 4 && (!c.with_color || g->prep_identity));
    // (A software-pipelined form of the chunk launch -- next round's gathers
    // in flight during this round's arithmetic -- made no difference at 4 and
    // 8 emulated ranks, profiles/r4p, r4zc: dropped.)
    chunk_frames = kChunkGroups * group;
    const int64_t px = (int64_t)c.depth_rows * c.depth_cols;
    // The records form keeps two sets of prepared records, sized by what the
    // call needs (a chunk of this call's frames -- not the 256-frame maximum:
    // 0.6 GB per set at VGA); a call that takes the raw form gives them back.
    const int recs_frames = n < chunk_frames ? n : chunk_frames;
    if (raw_form && z.chunk_recs[0]) {
        O3DMI_HIP_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < 2; ++i) {
            (void)hipFree(z.chunk_recs[i]);
            z.chunk_recs[i] = nullptr;
        }
        z.chunk_recs_pixels = 0;
        z.chunk_recs_frames = 0;
    }
    if (!raw_form &&
        (z.chunk_recs_pixels < px || z.chunk_recs_frames < recs_frames)) {
        O3DMI_HIP_CHECK(hipDeviceSynchronize());
        const int64_t new_px = z.chunk_recs_pixels > px ? z.chunk_recs_pixels
                                                        : px;
        const int new_fr = z.chunk_recs_frames > recs_frames
                                   ? z.chunk_recs_frames
                                   : recs_frames;
        for (int i = 0; i < 2; ++i) {
            (void)hipFree(z.chunk_recs[i]);
            z.chunk_recs[i] = nullptr;
            O3DMI_HIP_CHECK(hipMalloc((void**)&z.chunk_recs[i],
                                      sizeof(PixelRec) * (size_t)(new_px + 1) *
                                              (size_t)new_fr));
        }
        z.chunk_recs_pixels = new_px;
        z.chunk_recs_frames = new_fr;
    }
    // every launch of the previous call that reads the frame tables is over
    // once its last integrate launch is (the side stream waited for it)
    O3DMI_HIP_CHECK(hipStreamSynchronize(z.side));
    if ((st = UploadSliceFrames(g, c, frames, n, &shared,
                                raw_form ? 0 : chunk_frames)))
        return st;
    // the caller's images may still be in flight on its stream
    O3DMI_HIP_CHECK(hipEventRecord(z.ev_enter, s));
    O3DMI_HIP_CHECK(hipStreamWaitEvent(z.side, z.ev_enter, 0));
    return O3DMI_OK;
    };
    st = setup();
    if (comm && world > 1) {
        const int agreed = comm->AgreeStatus(st, s);
        if (agreed) {
            progress->left_in_step = true;
            return agreed;
        }
    } else if (st) {
        return st;
    }

    const int n_chunks = (n + chunk_frames - 1) / chunk_frames;
    std::vector<int> chunk_stamp((size_t)n_chunks, 0);
    progress->n_chunks = n_chunks;

    // The prepare pass of a chunk's frames (front roles without the block
    // touch), kMaxGroup frames per launch, into the chunk set's records.
    auto issue_prepare = [&](int ci) -> int {
        const int set = ci & 1;
        const int f0 = ci * chunk_frames;
        const int nc = n - f0 < chunk_frames ? n - f0 : chunk_frames;
        FrameFrontArgs fa[kMaxGroup];
        for (int b0 = 0; b0 < nc; b0 += kMaxGroup) {
            const int m = nc - b0 < kMaxGroup ? nc - b0 : kMaxGroup;
            for (int k = 0; k < m; ++k) {
                FrameFrontArgs& a = fa[k];
                a = FrameFrontArgs{};
                const StreamFrame& fr = frames[f0 + b0 + k];
                a.depth = (const uint16_t*)fr.depth;
                a.color = c.with_color ? (const uint8_t*)fr.color : nullptr;
                a.rows = c.depth_rows;
                a.cols = c.depth_cols;
                a.color_rows = c.color_rows;
                a.color_cols = c.color_cols;
                a.depth_intrinsic = c.depth_intrinsic;
                a.color_intrinsic = c.color_intrinsic ? c.color_intrinsic
                                                      : c.depth_intrinsic;
                a.extrinsic = fr.extrinsic;
                a.resolution = (int)g->block_resolution;
                a.voxel_size = g->voxel_size;
                a.sdf_trunc = g->voxel_size * c.trunc;
                a.depth_scale = c.depth_scale;
                a.depth_max = c.depth_max;
                a.stride = 4;
                a.group_stamp = 0;
                a.group_bit = k;
                a.touch_plane = 0;
                a.col_lut = g->prep_valid ? g->prep_col : nullptr;
                a.row_lut = g->prep_valid ? g->prep_row : nullptr;
                a.depth_div_short = g->prep_valid && g->prep_div_short;
                a.prep_identity = g->prep_valid && g->prep_identity;
                a.recs = z.chunk_recs[set] +
                         (size_t)(b0 + k) * (size_t)(z.chunk_recs_pixels + 1);
                a.prepare_only = true;
            }
            int st2 = LaunchFrameStep(g->block_hashmap, fa, m, nullptr, z.side);
            if (st2) return st2;
        }
        return O3DMI_OK;
    };

    auto issue_side = [&](int ci, bool touch) -> int {
        const int set = ci & 1;
        const int f0 = ci * chunk_frames;
        const int nc = n - f0 < chunk_frames ? n - f0 : chunk_frames;
        int st2;
        if (touch) {
            // the set's work list was read by chunk ci - 2's launch
            if (ci >= 2)
                O3DMI_HIP_CHECK(hipStreamWaitEvent(z.side, z.ev_main[set], 0));
            if ((st2 = LaunchTouchSlice(shared, z.frames_dev, f0, nc, rank,
                                        world, z.send_table, z.side)))
                return st2;
            if (!raw_form && (st2 = issue_prepare(ci))) return st2;
            if ((st2 = LaunchPackSlice(z.send_table, z.send_seg[set],
                                       z.capacity, z.side)))
                return st2;
            const int64_t seg = SliceSegmentBytes(z.capacity);
            if (comm) {
                if ((st2 = comm->Allgather(z.send_seg[set], z.gathered[set],
                                           seg, z.side)))
                    return st2;
                if (ci >= progress->first_gathers)
                    progress->first_gathers = ci + 1;
            } else {
                if (gathered_in && world > 1)
                    O3DMI_HIP_CHECK(hipMemcpyAsync(
                            z.gathered[set], gathered_in[ci],
                            (size_t)seg * world, hipMemcpyDeviceToDevice,
                            z.side));
                O3DMI_HIP_CHECK(hipMemcpyAsync(
                        (char*)z.gathered[set] + (size_t)seg * rank,
                        z.send_seg[set], (size_t)seg, hipMemcpyDeviceToDevice,
                        z.side));
            }
        }
        g->frame_stamp += 1;
        chunk_stamp[(size_t)ci] = g->frame_stamp;
        if ((st2 = LaunchApplySlice(g->block_hashmap, z.gathered[set], world,
                                    z.capacity, z.recv_table, g->frame_stamp,
                                    z.side)))
            return st2;
        if ((st2 = LaunchBuildChunk(g->block_hashmap, z.recv_table,
                                    z.entries[set], z.entries_cap,
                                    z.entries_count[set],
                                    (int*)g->stream_status + 4, g->frame_stamp,
                                    z.side)))
            return st2;
        O3DMI_HIP_CHECK(hipEventRecord(z.ev_side[set], z.side));
        return O3DMI_OK;
    };

    if ((st = issue_side(0, true))) return st;
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int set = ci & 1;
        const int f0 = ci * chunk_frames;
        const int nc = n - f0 < chunk_frames ? n - f0 : chunk_frames;
        // What the chunk's apply found: normally long there (it was issued a
        // chunk ago).
        ChunkStatus cs = {};
        for (int attempt = 0;; ++attempt) {
            if ((st = WaitChunkStatus(g, chunk_stamp[(size_t)ci], z.side, &cs)))
                return st;
            if (cs.overflow == 0) break;
            if (cs.overflow == -3) {
                // a rank left the call with an error and said so in its wire
                // segment: every rank leaves at this chunk, in step (none has
                // a collective outstanding)
                O3DMI_HIP_CHECK(hipDeviceSynchronize());
                SetLastError("sliced touch: another rank left the call with an "
                             "error");
                return O3DMI_ERR_PEER;
            }
            O3DMI_REQUIRE(attempt < 24, "sliced touch: cannot make room");
            O3DMI_HIP_CHECK(hipDeviceSynchronize());
            z.reapplied += 1;
            g->stream_overflow = 0;  // (PollStreamStatus reads the same words)
            if (cs.overflow > 0) {
                // the block hash ran out of buffer indices: the chunk was
                // dropped; reserve, apply the same records again
                int64_t wanted = 0;
                if ((st = RecoverOverflow(g->block_hashmap, s, &wanted)))
                    return st;
                const int64_t cap = o3dmi_hash_capacity(g->block_hashmap);
                if ((st = o3dmi_hash_reserve(g->block_hashmap,
                                             wanted > 2 * cap ? wanted : 2 * cap,
                                             (o3dmi_stream_t)s)))
                    return st;
                O3DMI_HIP_CHECK(hipStreamSynchronize(s));
                if ((st = issue_side(ci, false))) return st;
            } else if (cs.overflow == -2) {
                // THIS rank's receiver table was too small for the blocks it
                // owns in the chunk: a local matter (the other ranks are not
                // waiting for anything) -- a larger table and work lists, the
                // same gathered records applied again
                FreeChunkTable(&z.recv_table);
                for (int i = 0; i < 2; ++i) {
                    (void)hipFree(z.entries[i]);
                    z.entries[i] = nullptr;
                }
                z.recv_slots *= 2;
                if ((st = AllocChunkTable(&z.recv_table, z.recv_slots, true,
                                          z.side)))
                    return st;
                for (int i = 0; i < 2; ++i)
                    O3DMI_HIP_CHECK(hipMalloc(
                            (void**)&z.entries[i],
                            sizeof(ChunkEntry) * (size_t)(z.recv_slots / 2)));
                z.entries_cap = z.recv_slots / 2;
                O3DMI_HIP_CHECK(hipStreamSynchronize(z.side));
                if ((st = issue_side(ci, false))) return st;
            } else {
                // a SENDER's wire segment or table was too small (the flags
                // travel in the all-gathered headers: every rank takes this
                // branch for the same chunk): double both, touch again
                if (gathered_in) {
                    SetLastError("sliced touch: the given wire segments are "
                                 "too small for this stream "
                                 "(o3dmi_vbg_set_slice_capacity)");
                    return O3DMI_ERR_CAPACITY;
                }
                // (every rank is here for the same chunk with nothing in
                // flight: a rank that cannot grow its buffers says so before
                // the others enter the redone all-gather -- its own send
                // segment is gone by then, no abort segment could be sent)
                st = EnsureSliced(g, world, z.capacity * 2, z.table_slots * 2,
                                  s);
                if (comm && world > 1) {
                    const int agreed = comm->AgreeStatus(st, s);
                    if (agreed) {
                        progress->left_in_step = true;
                        return agreed;
                    }
                } else if (st) {
                    return st;
                }
                if ((st = issue_side(ci, true))) return st;
            }
        }
        if (ci + 1 < n_chunks)
            if ((st = issue_side(ci + 1, true))) return st;
        // the chunk's integrate launch
        O3DMI_HIP_CHECK(hipStreamWaitEvent(s, z.ev_side[set], 0));
        g->frame_stamp += 1;
        const bool prof = g->profiling && g->prof_frames < g->prof_max &&
                          g->prof_stride > 0 &&
                          (g->prof_seen++ % g->prof_stride) == 0;
        hipEvent_t* pe = prof ? &g->prof_events[(size_t)g->prof_frames * 2]
                              : nullptr;
        ChunkIntegrateArgs ia = {};
        ia.n_frames = nc;
        ia.frames = z.iframes_dev + f0;
        ia.entries = z.entries[set];
        ia.count = z.entries_count[set];
        ia.entries_cap = z.entries_cap;
        ia.grid_hint = cs.blocks;
        ia.rows = c.depth_rows;
        ia.cols = c.depth_cols;
        ia.with_color = c.with_color;
        ia.tsdf = (float*)o3dmi_hash_value_buffer(g->block_hashmap, c.ti);
        ia.weight = o3dmi_hash_value_buffer(g->block_hashmap, c.wi);
        ia.color = c.with_color
                           ? o3dmi_hash_value_buffer(g->block_hashmap, c.ci)
                           : nullptr;
        ia.grid_dtype = c.grid_dtype;
        ia.depth_intrinsic = c.depth_intrinsic;
        ia.resolution = (int)g->block_resolution;
        ia.voxel_size = g->voxel_size;
        ia.sdf_trunc = g->voxel_size * c.trunc;
        ia.depth_max = c.depth_max;
        ia.depth_scale = c.depth_scale;
        ia.depth_div_short = g->prep_div_short;
        ia.raw = raw_form;
        ia.size_host = (int*)g->stream_status;
        ia.status_stamp = g->frame_stamp;
        ia.prof_count = prof ? g->prof_counts + g->prof_max + g->prof_frames
                             : nullptr;
        ia.prof_frame_blocks = prof ? g->prof_counts + g->prof_frames : nullptr;
        ia.prof_map_size =
                prof ? g->prof_counts + 2 * g->prof_max + g->prof_frames
                     : nullptr;
        if (pe) O3DMI_HIP_CHECK(hipEventRecord(pe[0], s));
        if ((st = LaunchChunkIntegrate(g->block_hashmap, ia, s))) return st;
        if (pe) {
            O3DMI_HIP_CHECK(hipEventRecord(pe[1], s));
            g->prof_launch_frames += nc;
            g->prof_frames += 1;
        }
        O3DMI_HIP_CHECK(hipEventRecord(z.ev_main[set], s));
        if ((st = PollStreamStatus(g))) return st;  // deferred error flags
        z.chunks_done += 1;
    }
    // the next call's side-stream work must not pass this call's launches
    // (the frame tables, the work lists)
    O3DMI_HIP_CHECK(hipStreamWaitEvent(z.side, z.ev_main[(n_chunks - 1) & 1], 0));
    g->known_valid = false;  // the other paths take the size from the map
    g->stream_overflow = 0;
    g->last_path = 0;
    return O3DMI_OK;
}

namespace o3dmi {

void FreeSliced(o3dmi_vbg* g) {
    o3dmi_vbg::Sliced& z = g->sliced;
    if (z.side) (void)hipStreamDestroy(z.side);
    for (int i = 0; i < 2; ++i) {
        if (z.ev_side[i]) (void)hipEventDestroy(z.ev_side[i]);
        if (z.ev_main[i]) (void)hipEventDestroy(z.ev_main[i]);
        (void)hipFree(z.send_seg[i]);
        (void)hipFree(z.gathered[i]);
        (void)hipFree(z.entries[i]);
        (void)hipFree(z.entries_count[i]);
    }
    if (z.ev_enter) (void)hipEventDestroy(z.ev_enter);
    if (z.table_slots) {
        FreeChunkTable(&z.send_table);
        FreeChunkTable(&z.recv_table);
    }
    (void)hipFree(z.frames_dev);
    (void)hipFree(z.iframes_dev);
    (void)hipFree(z.chunk_recs[0]);
    (void)hipFree(z.chunk_recs[1]);
    // (what the ranks agreed on is not a buffer: it outlives a re-allocation
    // that one rank may do on its own)
    const float agreed_trunc = z.agreed_trunc;
    const int agreed_fast_div = z.agreed_fast_div;
    const void* agreed_comm = z.agreed_comm;
    z = o3dmi_vbg::Sliced();
    z.agreed_trunc = agreed_trunc;
    z.agreed_fast_div = agreed_fast_div;
    z.agreed_comm = agreed_comm;
}

// o3dmi_vbg_integrate_frames on a grid with block ownership and a communicator
// is a COLLECTIVE call (one all-gather per chunk of frames). A rank that has to
// leave it with an error of its own (no room after 24 attempts, an allocation
// that failed, a deferred device-side flag) would leave the others waiting in
// the next all-gather: it delivers that one all-gather with an empty segment
// flagged kSliceFlagAbort first, and every rank returns O3DMI_ERR_PEER at the
// same chunk. The map is left usable (a dropped chunk's slots are recovered,
// the stream's overflow state cleared). Best effort after a HIP runtime error:
// the abort segment is then issued on a device that may not execute it.
int StreamIntegrateSliced(o3dmi_vbg* g, const StreamCommon& c0,
                          const StreamFrame* frames, int n, int group,
                          hipStream_t s, o3dmi_comm* comm,
                          const void* const* gathered_in) {
    SlicedProgress pr;
    const int st = StreamIntegrateSlicedBody(g, c0, frames, n, group, s, comm,
                                             gathered_in, &pr);
    if (st == O3DMI_OK) return st;
    const std::string why = o3dmi_last_error();
    o3dmi_vbg::Sliced& z = g->sliced;
    if (st != O3DMI_ERR_PEER && !pr.left_in_step && comm && z.side &&
        pr.n_chunks > 0 && pr.first_gathers > 0 &&
        pr.first_gathers < pr.n_chunks) {
        // the all-gather the other ranks will wait in next
        const int set = pr.first_gathers & 1;
        SliceHeader hd = {};
        hd.count = 0;
        hd.flags = kSliceFlagAbort;
        hd.capacity = z.capacity;
        if (hipMemcpyAsync(z.send_seg[set], &hd, sizeof(hd),
                           hipMemcpyHostToDevice, z.side) == hipSuccess &&
            hipStreamSynchronize(z.side) == hipSuccess)
            (void)comm->Allgather(z.send_seg[set], z.gathered[set],
                                  SliceSegmentBytes(z.capacity), z.side);
    }
    (void)hipDeviceSynchronize();
    // leave the map usable: a chunk dropped for lack of buffer indices left
    // keys without a block behind (CheckDeferred would refuse every later
    // size / export call)
    int64_t wanted = 0;
    (void)RecoverOverflow(g->block_hashmap, s, &wanted);
    (void)hipStreamSynchronize(s);
    g->stream_overflow = 0;
    g->known_valid = false;
    g->last_path = 0;
    SetLastError(why.c_str());
    return st;
}

}  // namespace o3dmi

extern "C" {

int o3dmi_vbg_set_slice_capacity(o3dmi_vbg_t* g, int records_per_group,
                                 int table_slots) {
    O3DMI_REQUIRE(g != nullptr, "grid is null");
    O3DMI_REQUIRE(records_per_group >= 16 && table_slots >= 64 &&
                          (table_slots & (table_slots - 1)) == 0,
                  "slice capacity: records >= 16, table slots a power of two "
                  ">= 64");
    o3dmi_vbg::Sliced& z = g->sliced;
    if (z.side) {
        O3DMI_HIP_CHECK(hipDeviceSynchronize());
        FreeSliced(g);
    }
    z.capacity = records_per_group;
    z.table_slots = 0;
    g->sliced_slots_wanted = table_slots;
    return O3DMI_OK;
}

int64_t o3dmi_vbg_slice_segment_bytes(const o3dmi_vbg_t* g) {
    if (!g) return 0;
    return SliceSegmentBytes(g->sliced.capacity ? g->sliced.capacity : 4096);
}

int o3dmi_vbg_slice_chunk_frames(int frames_per_launch) {
    return kChunkGroups * ClampGroup(frames_per_launch);
}

int o3dmi_vbg_touch_slice(o3dmi_vbg_t* g, int n_frames,
                          const void* const* depth_devs, int depth_rows,
                          int depth_cols, const double* depth_intrinsic,
                          const double* extrinsics, float depth_scale,
                          float depth_max, float trunc_voxel_multiplier,
                          int frames_per_launch, int slice_rank,
                          int slice_world, void* segment_out_dev,
                          o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_devs && depth_intrinsic && extrinsics &&
                          segment_out_dev,
                  "null argument");
    O3DMI_REQUIRE(n_frames >= 1 &&
                          n_frames <= kChunkGroups * ClampGroup(frames_per_launch),
                  "touch slice: at most one chunk of frames per call");
    hipStream_t s = (hipStream_t)stream;
    o3dmi_vbg::Sliced& z = g->sliced;
    int st = EnsureSliced(g, slice_world > z.world ? slice_world : z.world,
                          z.capacity ? z.capacity : 4096,
                          z.table_slots ? z.table_slots
                                        : g->sliced_slots_wanted,
                          s);
    if (st) return st;
    const StreamCommon c =
            MakeCommon(depth_rows, depth_cols, 0, 0, depth_intrinsic, nullptr,
                       depth_scale, depth_max, trunc_voxel_multiplier);
    const std::vector<StreamFrame> frames =
            MakeFrames(depth_devs, nullptr, extrinsics, n_frames);
    // everything on the side stream, behind the caller's stream and in front
    // of whatever the caller does next on it
    O3DMI_HIP_CHECK(hipEventRecord(z.ev_enter, s));
    O3DMI_HIP_CHECK(hipStreamWaitEvent(z.side, z.ev_enter, 0));
    TouchParams shared;
    O3DMI_HIP_CHECK(hipStreamSynchronize(z.side));
    if ((st = UploadSliceFrames(g, c, frames.data(), n_frames, &shared)))
        return st;
    if ((st = LaunchTouchSlice(shared, z.frames_dev, 0, n_frames, slice_rank,
                               slice_world, z.send_table, z.side)))
        return st;
    if ((st = LaunchPackSlice(z.send_table, segment_out_dev, z.capacity,
                              z.side)))
        return st;
    O3DMI_HIP_CHECK(hipEventRecord(z.ev_enter, z.side));
    O3DMI_HIP_CHECK(hipStreamWaitEvent(s, z.ev_enter, 0));
    return O3DMI_OK;
}

int o3dmi_vbg_integrate_frames_sliced(
        o3dmi_vbg_t* g, int n_frames, const void* const* depth_devs,
        int depth_rows, int depth_cols, const void* const* color_devs,
        int color_rows, int color_cols, int input_dtype,
        const double* depth_intrinsic, const double* color_intrinsic,
        const double* extrinsics, float depth_scale, float depth_max,
        float trunc_voxel_multiplier, int frames_per_launch,
        const void* const* gathered_devs, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(g && depth_devs && depth_intrinsic && extrinsics &&
                          n_frames >= 0,
                  "null argument");
    O3DMI_REQUIRE(StreamPathApplies(g, input_dtype),
                  "sliced touch: uint16 depth, float32 tsdf and a block "
                  "resolution divisible by 4 are required");
    o3dmi_comm* comm = gathered_devs ? nullptr : ThreadComm();
    O3DMI_REQUIRE(gathered_devs || comm || g->owner_world == 1,
                  "sliced touch: neither wire segments nor a communicator "
                  "(o3dmi_set_comm)");
    if (n_frames == 0) return O3DMI_OK;
    StreamCommon c = MakeCommon(depth_rows, depth_cols, color_rows, color_cols,
                                depth_intrinsic, color_intrinsic, depth_scale,
                                depth_max, trunc_voxel_multiplier);
    const std::vector<StreamFrame> frames =
            MakeFrames(depth_devs, color_devs, extrinsics, n_frames);
    return StreamIntegrateSliced(g, c, frames.data(), n_frames,
                                 ClampGroup(frames_per_launch),
                                 (hipStream_t)stream, comm, gathered_devs);
}

int o3dmi_vbg_sliced_stats(const o3dmi_vbg_t* g, int64_t* chunks,
                           int64_t* reapplied, int* capacity,
                           int* table_slots) {
    O3DMI_REQUIRE(g != nullptr, "grid is null");
    if (chunks) *chunks = g->sliced.chunks_done;
    if (reapplied) *reapplied = g->sliced.reapplied;
    if (capacity) *capacity = g->sliced.capacity;
    if (table_slots) *table_slots = g->sliced.table_slots;
    return O3DMI_OK;
}

}  // extern "C"
