// The pyramids of the MultiScaleICP driver (registration.cpp):
// InitializePointCloudPyramidForMultiScaleICP, Registration.cpp:221-273, for
// the source and the target cloud, and the coarsest scale's index.
//
// The source pyramid and the target pyramid are independent chains of
// VoxelDownSample levels, each a string of small launches whose sizes stay
// on the device (the voxel count of one level is the point count of the
// next; level buffers are sized by the input cloud) -- latency, not
// throughput. One host thread issues both, level by level, so the GPU works
// on the two chains at once; the counts of both are read back once, at the
// end. (Round 2 first ran the target chain from a helper thread: the thread
// start and its first HIP call cost more than issuing the second chain's
// launches from here.)

#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../common.h"
#include "../mailbox.h"
#include "../nns.h"
#include "../vds.h"
#include "icp_driver.h"
#include "o3d_mi355x_host.h"

namespace o3dmi {

namespace {

// One pyramid level without a host wait (vds.h). PointCloud::VoxelDownSample
// averages every attribute; the kernel takes positions + one attribute, so
// further attributes go through it again (the voxel order, first occurrence,
// is the same every time, and so are the positions and the count).
// next_voxel > 0: the chain's next call down-samples out_pos by that size;
// from_previous: pos is the out_pos of the chain's previous call (vds.h: a
// level with a single pass then carries the next level's hash insert).
int DownSampleAttrsAsync(const void* pos, int64_t n_max, const int* n_dev,
                         int dtype, double voxel, void* out_pos, int* m_dev,
                         int* err_dev, hipStream_t cs, int chain,
                         std::initializer_list<std::pair<const void*, void*>>
                                 attrs,
                         double next_voxel = 0, bool from_previous = false,
                         VdsLevelJob* defer = nullptr) {
    if (voxel <= 0) {
        SetLastError("voxel_size must be positive.");
        return O3DMI_ERR_INVALID_ARG;
    }
    VdsLevelJob job;
    job.pos = pos;
    job.n_max = n_max;
    job.n_dev = n_dev;
    job.voxel_size = voxel;
    job.out_pos = out_pos;
    job.m_dev = m_dev;
    job.err_dev = err_dev;
    job.chain = chain;
    int passes = 0;
    for (const auto& a : attrs) passes += a.first ? 1 : 0;
    if (passes <= 1) {
        job.next_voxel_size = next_voxel;
        job.from_previous = from_previous;
        for (const auto& a : attrs)
            if (a.first) {
                job.attr = a.first;
                job.out_attr = a.second;
            }
        // one pass: with `defer` the caller launches it together with the
        // other cloud's level (VdsPairAsync)
        if (defer) {
            *defer = job;
            return O3DMI_OK;
        }
        return VdsPairAsync(&job, 1, dtype, cs);
    }
    for (const auto& a : attrs) {
        if (!a.first) continue;
        job.attr = a.first;
        job.out_attr = a.second;
        int st = VdsPairAsync(&job, 1, dtype, cs);
        if (st) return st;
    }
    return O3DMI_OK;
}

// Device-side level counts of one cloud's pyramid: [level] voxel counts, then
// one word of error flags, in the chain's persistent buffer (vds.h VdsChain:
// zero at Init; the posting launch re-zeroes what it delivers). Read once, at
// the end of the chain, through the chain's host mailbox: no clearing fill, no
// copy, no stream synchronisation per call.
constexpr int kMaxScales = 30;
static_assert(kMaxScales + 1 <= kCountsErr && kMaxScales + 1 <= 32,
              "level counts below the error word; a post carries <= 32 values");
struct ChainCounts {
    int* dev = nullptr;
    int levels = 0;
    int chain = 0;
    VdsChain* state = nullptr;
    int Init(int n_levels, int chain_id, hipStream_t cs) {
        O3DMI_REQUIRE(n_levels >= 1 && n_levels <= kMaxScales,
                      "too many scales");
        int st = VdsChainBegin(chain_id, cs, &state, &dev);
        if (st) return st;
        levels = n_levels;
        chain = chain_id;
        return O3DMI_OK;
    }
    int* Count(int level) { return dev + level; }
    // (valid behind the chain's post)
    const int* KeptCount(int level) const { return dev + kCountsKeep + level; }
    int* Err() { return dev + kCountsErr; }  // (a post's value `levels`)
    // The counts leave for the chain's mailbox behind the chain's launches,
    // with the next sequence number of that mailbox (counts == NULL: there is
    // no mailbox): NewPost is the request, Sent records who carried it out --
    // the chain's last level launch itself (vds.h VdsPost: a sealed block) or
    // the posting launch. Wait: for that, and returns them. (Both chains
    // post before either is waited for: one host round trip, not two.)
    int posted_seq = 0;
    bool sealed = false;
    VdsPost NewPost() {
        VdsPost p;
        Mailbox* mb = ThreadMailbox(1 + chain);
        if (!mb) return p;
        p.counts = dev;
        p.n = levels + 1;
        p.mail_data = mb->data;
        p.mail_flag = mb->flag;
        p.mail_seq = ++mb->seq;
        return p;
    }
    void Sent(const VdsPost& p, bool by_level_launch) {
        posted_seq = p.mail_seq;
        sealed = by_level_launch;
    }
    // one posting launch: for one chain, or for two built in the same launches
    static int Post(std::initializer_list<ChainCounts*> chains,
                    hipStream_t cs) {
        VdsPost posts[2];
        int n = 0;
        for (ChainCounts* c : chains) {
            posts[n] = c->NewPost();
            c->Sent(posts[n++], false);
        }
        return PostCounts(posts, n, cs);
    }
    int Wait(std::vector<int>& out, hipStream_t cs) {
        out.assign((size_t)levels + 1, 0);
        Mailbox* mb = ThreadMailbox(1 + chain);
        O3DMI_REQUIRE(mb != nullptr && posted_seq != 0, "counts not posted");
        const int seq = posted_seq;
        posted_seq = 0;
        double sealed32[32];
        hipError_t e = sealed ? MailboxWaitSealed(mb, seq, cs, sealed32)
                              : MailboxWait(mb, seq, cs);
        const bool was_sealed = sealed;
        sealed = false;
        if (e != hipSuccess) {
            SetLastError(std::string("pyramid read-back: ") +
                         hipGetErrorString(e));
            return O3DMI_ERR_HIP;
        }
        // the posting launch has run: counts and error word are zero again,
        // every level's last launch has cleaned its workspace
        VdsChainEnd(state);
        for (int k = 0; k <= levels; ++k)
            out[(size_t)k] = (int)(was_sealed ? sealed32[k] : mb->data[k]);
        if (out[(size_t)levels] & kErrKeyRange) {
            SetLastError("VoxelDownSample: voxel coordinate outside +-2^20");
            return O3DMI_ERR_KEY_RANGE;
        }
        return O3DMI_OK;
    }
};

// One cloud's chain of levels: what the level function needs to know about
// the cloud, and the two things in which the clouds differ.
struct CloudChain {
    const void* pos = nullptr;  // the caller's cloud
    const void* attr[kCloudAttrs] = {};
    int64_t n = 0;
    const int* n_dev = nullptr;
    int id = 0;  // chain 0 (source) / 1 (target)
    hipStream_t cs = nullptr;
    CloudLevel Level::*which = nullptr;  // its half of a pyramid level
    // the source is moved in place every iteration: a finest level that is
    // the input itself is a private copy (the target's aliases the caller's)
    bool clone_input = false;
    // coloured ICP: the finest level needs colour gradients (target)
    bool needs_gradients = false;
    // the finest level's size is a host number: it is the input itself, or it
    // was read back for the gradients
    bool finest_on_host = false;
    ChainCounts counts;
    CloudChain(const IcpCall& c, const void* cloud, int64_t size,
               const int32_t* size_dev, int chain, hipStream_t stream,
               CloudLevel Level::*half)
        : pos(cloud), n(size), n_dev((const int*)size_dev), id(chain),
          cs(stream), which(half), finest_on_host(c.finest_is_input) {}
};

int Clone(const IcpCall& c, DeviceBuffer& dst, const void* src, int64_t n,
          hipStream_t cs) {
    int e = dst.Alloc((size_t)n * 3 * c.esz);
    if (e) return e;
    O3DMI_HIP_CHECK(hipMemcpyAsync(dst.p, src, (size_t)n * 3 * c.esz,
                                   hipMemcpyDeviceToDevice, cs));
    return O3DMI_OK;
}

// Registration.cpp:243-262: EstimateColorGradients(30, radius) on the finest
// level of the target pyramid. The operator needs the level's size on the
// host: this (rare) path waits.
int EstimateFinestGradients(const IcpCall& c, CloudChain& ch, CloudLevel& L) {
    const int k = c.num_scales - 1;
    if (!c.finest_is_input) {
        int host_n = 0;
        O3DMI_HIP_CHECK(hipMemcpyAsync(&host_n, ch.counts.Count(k), sizeof(int),
                                       hipMemcpyDeviceToHost, ch.cs));
        O3DMI_HIP_CHECK(hipStreamSynchronize(ch.cs));
        L.n = host_n;
        ch.finest_on_host = true;
    }
    const double radius = c.voxel_sizes[k] <= 0 ? c.max_dists[k] * 2.0
                                                : c.voxel_sizes[k] * 4.0;
    DeviceBuffer& grad = L.attr_buf[kGradients];
    int e = grad.Alloc((size_t)ch.n * 3 * c.esz);
    if (e) return e;
    e = o3dmi_pointcloud_estimate_color_gradients(
            L.pos, L.attr[kNormals], L.attr[kColors], L.n, c.dtype, 30, radius,
            grad.p, (o3dmi_stream_t)ch.cs);
    if (e) return e;
    L.attr[kGradients] = grad.p;
    return O3DMI_OK;
}

// Level k of one cloud's pyramid: the input itself (voxel size <= 0, finest
// level only), else the down-sampled input (finest) or finer level. With
// `job` a level of a single pass is left for the caller to launch.
int BuildLevel(const IcpCall& c, CloudChain& ch, std::vector<Level>& pyr, int k,
               VdsLevelJob* job) {
    int e;
    const int last = c.num_scales - 1;
    CloudLevel& L = pyr[(size_t)k].*ch.which;
    ChainCounts& cc = ch.counts;
    if (k == last && c.finest_is_input) {
        L.n = ch.n;
        L.pos = ch.pos;
        for (int a = 0; a < kCloudAttrs; ++a) L.attr[a] = ch.attr[a];
        if (ch.clone_input) {
            if ((e = Clone(c, L.pos_buf, ch.pos, ch.n, ch.cs))) return e;
            L.pos = L.pos_buf.p;
            for (int a = 0; a < kCloudAttrs; ++a) {
                if (!ch.attr[a]) continue;
                if ((e = Clone(c, L.attr_buf[a], ch.attr[a], ch.n, ch.cs)))
                    return e;
                L.attr[a] = L.attr_buf[a].p;
            }
        }
    } else {
        // (the coarser level is built from this one's output: vds.h)
        const double next_vs = k > 0 ? c.voxel_sizes[k - 1] : 0.0;
        const CloudLevel* F =
                k == last ? nullptr : &(pyr[(size_t)k + 1].*ch.which);
        const void* const* in_attr = F ? F->attr : ch.attr;
        static_assert(kCloudAttrs == 8, "the attribute passes listed below");
        if ((e = L.pos_buf.Alloc((size_t)ch.n * 3 * c.esz))) return e;
        for (int a = 0; a < kCloudAttrs; ++a)
            if (in_attr[a] &&
                (e = L.attr_buf[a].Alloc((size_t)ch.n * 3 * c.esz)))
                return e;
        // the finer level's size is a host number when it is the input
        // itself (or was read back): then n_max = that size
        const bool f_host = F && k + 1 == last && ch.finest_on_host;
        e = DownSampleAttrsAsync(
                F ? F->pos : ch.pos, f_host ? F->n : ch.n,
                F ? (f_host ? nullptr : cc.Count(k + 1)) : ch.n_dev, c.dtype,
                c.voxel_sizes[k], L.pos_buf.p, cc.Count(k), cc.Err(), ch.cs,
                ch.id,
                {{in_attr[0], L.attr_buf[0].p},
                 {in_attr[1], L.attr_buf[1].p},
                 {in_attr[2], L.attr_buf[2].p},
                 {in_attr[3], L.attr_buf[3].p},
                 {in_attr[4], L.attr_buf[4].p},
                 {in_attr[5], L.attr_buf[5].p},
                 {in_attr[6], L.attr_buf[6].p},
                 {in_attr[7], L.attr_buf[7].p}},
                next_vs, F && !f_host, job);
        if (e) return e;
        L.pos = L.pos_buf.p;
        // (an attribute the cloud does not have stays NULL)
        for (int a = 0; a < kCloudAttrs; ++a) L.attr[a] = L.attr_buf[a].p;
    }
    if (k == last && ch.needs_gradients && !L.attr[kGradients])
        return EstimateFinestGradients(c, ch, L);
    return O3DMI_OK;
}

// Every level of both pyramids, coarsest last. `paired`: the two clouds'
// levels go out in the SAME launches on the caller's stream; *counts_posted:
// the coarsest pair's launch took the counts' post with it.
int LaunchLevels(const IcpCall& c, CloudChain& src, CloudChain& tgt,
                 std::vector<Level>& pyr, bool paired, bool* counts_posted) {
    static const bool no_folded_post =
            std::getenv("O3DMI_VDS_POST_LAUNCH") != nullptr;
    int st;
    for (int k = c.num_scales - 1; k >= 0; --k) {
        VdsLevelJob jobs[2];
        // the target level's job is prepared before the source level's
        if ((st = BuildLevel(c, tgt, pyr, k, paired ? &jobs[1] : nullptr)))
            return st;
        if ((st = BuildLevel(c, src, pyr, k, paired ? &jobs[0] : nullptr)))
            return st;
        if (!paired) continue;
        // (a level that is the input itself leaves its job empty)
        VdsLevelJob both[2];
        int n_jobs = 0;
        if (jobs[0].pos) both[n_jobs++] = jobs[0];
        if (jobs[1].pos) both[n_jobs++] = jobs[1];
        // the coarsest level's launch posts both chains' counts itself
        const bool offer = k == 0 && n_jobs == 2 && !no_folded_post;
        if (offer) {
            both[0].post = src.counts.NewPost();
            both[1].post = tgt.counts.NewPost();
        }
        bool posted = false;
        if (n_jobs &&
            (st = VdsPairAsync(both, n_jobs, c.dtype, c.s, &posted)))
            return st;
        if (posted) {
            src.counts.Sent(both[0].post, true);
            tgt.counts.Sent(both[1].post, true);
            *counts_posted = true;
        }
    }
    return O3DMI_OK;
}

}  // namespace

hipStream_t SideStream() {
    static thread_local hipStream_t side[kMaxDevices] = {};
    const int d = CurrentDevice();
    if (d < 0) return nullptr;
    if (!side[d] &&
        hipStreamCreateWithFlags(&side[d], hipStreamNonBlocking) != hipSuccess)
        side[d] = nullptr;
    return side[d];
}

hipEvent_t SideEvent() {
    static thread_local hipEvent_t ev[kMaxDevices] = {};
    const int d = CurrentDevice();
    if (d < 0) return nullptr;
    if (!ev[d] &&
        hipEventCreateWithFlags(&ev[d], hipEventDisableTiming) != hipSuccess)
        ev[d] = nullptr;
    return ev[d];
}

int BuildPyramids(const IcpCall& c, std::vector<Level>& pyr,
                  NnsGuard& first_index) {
    const int last = c.num_scales - 1;
    int st;
    if (c.side != c.s) {
        // the caller's clouds may still be in flight on its stream
        O3DMI_HIP_CHECK(hipEventRecord(c.ev, c.s));
        O3DMI_HIP_CHECK(hipStreamWaitEvent(c.side, c.ev, 0));
    }
    // Round 6: the two pyramids advance level by level in the SAME
    // launches on the caller's stream (VdsPairAsync: blockIdx.y = cloud)
    // -- 7 launches + one posting launch for a three-level pair of
    // pyramids instead of two chains of 8 on two streams (the source chain on
    // the caller's stream, the target chain on the side stream). Coloured ICP
    // (three attribute passes per target level), Doppler ICP (two per
    // source level) and generalized ICP (three per level of either cloud)
    // keep the two chains.
    static const bool unpaired = std::getenv("O3DMI_VDS_UNPAIRED") != nullptr;
    const bool paired = !c.Is(O3DMI_ICP_COLORED) && !c.Is(O3DMI_ICP_DOPPLER) &&
                        !c.Is(O3DMI_ICP_GENERALIZED) && !unpaired;
    hipStream_t ts = paired ? c.s : c.side;
    CloudChain src(c, c.source, c.ns, c.ns_dev, 0, c.s, &Level::source);
    src.attr[kNormals] = c.source_normals;
    src.attr[kColors] = c.source_colors;
    src.attr[kDirections] = c.source_directions;
    src.attr[kDopplers] = c.source_dopplers3;
    for (int r = 0; r < 3; ++r) src.attr[kCovRow0 + r] = c.source_cov_rows[r];
    src.clone_input = true;
    CloudChain tgt(c, c.target, c.nt, c.nt_dev, 1, ts, &Level::target);
    tgt.attr[kNormals] = c.target_normals;
    tgt.attr[kColors] = c.target_colors;
    tgt.attr[kGradients] = c.target_gradients;
    for (int r = 0; r < 3; ++r) tgt.attr[kCovRow0 + r] = c.target_cov_rows[r];
    tgt.needs_gradients = c.Is(O3DMI_ICP_COLORED);
    ChainCounts &scc = src.counts, &tcc = tgt.counts;
    if ((st = scc.Init(c.num_scales, 0, c.s))) return st;
    if ((st = tcc.Init(c.num_scales, 1, ts))) return st;
    bool counts_posted = false;
    if ((st = LaunchLevels(c, src, tgt, pyr, paired, &counts_posted)))
        return st;
    // The coarsest scale's index, queued behind the posting launch BEFORE
    // the sizes are read back (its one-workgroup build takes the target
    // level's size from the count the posting launch keeps): it runs while
    // the counts cross PCIe and the host gets ready to launch the first
    // search -- that search used to wait for count -> host -> allocation ->
    // build launch -> build (a 20 us hole in every tracked frame, r6a).
    NnsGuard early;  // (destroyed with a device-wide wait if not adopted)
    const CloudLevel& T0 = pyr[0].target;
    const void* nrm0 =
            c.SearchesPointToPlane() ? T0.attr[kNormals] : nullptr;
    const bool early_build =
            paired && !(last == 0 && c.finest_is_input) && T0.pos;
    if (paired) {
        if (!counts_posted && (st = ChainCounts::Post({&scc, &tcc}, c.s)))
            return st;
        if (early_build &&
            (st = o3dmi_internal_nns_create_small_deferred(
                     T0.pos, nrm0, tcc.KeptCount(0), c.dtype, c.max_dists[0],
                     c.stream(), &early.nns)))
            return st;
    } else {
        if ((st = ChainCounts::Post({&tcc}, ts))) return st;
        if ((st = ChainCounts::Post({&scc}, c.s))) return st;
    }
    std::vector<int> counts;
    if ((st = tcc.Wait(counts, ts))) return st;
    for (int k = 0; k < c.num_scales; ++k)
        if (!(k == last && tgt.finest_on_host))
            pyr[(size_t)k].target.n = counts[(size_t)k];
    if ((st = scc.Wait(counts, c.s))) return st;
    for (int k = 0; k < c.num_scales; ++k)
        if (!(k == last && c.finest_is_input))
            pyr[(size_t)k].source.n = counts[(size_t)k];
    // Indices: the first scale's on the caller's stream (its first search
    // follows at once). The others go to the side stream LATER, issued while
    // the host would otherwise spin on a search launch's sums (registration.cpp
    // IndexScheduler): issuing them here kept the host busy for ~60 us (eight
    // launch calls) before it got to the first search -- with the GPU idle
    // (tools/slam_timeline.py).
    if (early.nns && o3dmi_internal_nns_adopt_count(early.nns, T0.n)) {
        first_index.nns = early.nns;
        early.nns = nullptr;
        return O3DMI_OK;
    }
    return o3dmi_internal_nns_create_with_normals(T0.pos, nrm0, T0.n, c.dtype,
                                                  c.max_dists[0], c.stream(),
                                                  &first_index.nns);
}

}  // namespace o3dmi
