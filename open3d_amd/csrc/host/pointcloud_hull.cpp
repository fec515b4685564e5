// Host driver of PointCloud::ComputeConvexHull / HiddenPointRemoval
// (t/geometry/PointCloud.cpp:1608, 1668): the checks, the widened (or
// flipped) cloud, the initial simplex, the rounds and the canonical output.
// A call waits once for the finiteness gate (hidden-point removal: once more
// for the flipped cloud), once for the simplex, ONCE PER ROUND for the round's
// word block (winners, new facets, live points) and once for the output's
// counts, then drains the stream. The round loop ends when no facet has a
// conflict and is bounded by the number of points; a bound that is hit is
// O3DMI_ERR_INTERNAL, never a longer loop. The kernels are in
// pointcloud_hull.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../pointcloud_hull.h"
#include "../pointcloud_sample.h"
#include "../scan.h"
#include "../sort.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_hull_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

thread_local int64_t g_stats[4] = {0, 0, 0, 0};

// What both calls refuse from their arguments alone.
int CheckCall(const void* points_dev, int64_t n, int64_t min_n, int dtype,
              const HullOutput& o) {
    int st = CheckFloat(dtype);
    if (st) return st;
    O3DMI_REQUIRE(o.index_dtype == O3DMI_I32 || o.index_dtype == O3DMI_I64,
                  "indices must be Int32 or Int64");
    O3DMI_REQUIRE(n >= min_n, "too few points for a hull");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "n out of range (< 2^31 - 1 points)");
    O3DMI_REQUIRE(points_dev && o.n_vertices && o.n_triangles,
                  "null argument");
    if (o.vertex_capacity > 0)
        O3DMI_REQUIRE(o.positions && o.point_indices, "null argument");
    if (o.vertex_capacity >= 0 && o.triangle_capacity > 0)
        O3DMI_REQUIRE(o.triangles, "null argument");
    return O3DMI_OK;
}

// O3DMI_HULL_WALK (docs/switches.md; per call): "sweep" runs every round in
// the sweep form, a number in [1, kHullWalkCap] is the number of facets a walk
// may hold.
void ReadSwitches(bool* sweep_only, int* walk_cap) {
    *sweep_only = false;
    *walk_cap = kHullWalkCap;
    const char* form = std::getenv("O3DMI_HULL_WALK");
    if (!form) return;
    if (std::string(form) == "sweep") {
        *sweep_only = true;
        return;
    }
    const long c = std::strtol(form, nullptr, 10);
    if (c >= 1 && c <= kHullWalkCap) *walk_cap = (int)c;
}

template <typename P>
int AllocN(PoolScratch& pool, P** out, size_t count) {
    return pool.Alloc(out, sizeof(P) * std::max<size_t>(count, 1));
}

}  // namespace

// The hull of the m widened points P_dev, written by the count / capacity
// protocol (pointcloud_hull_host.h).
int o3dmi::HullOf(PoolScratch& pool, const double* P_dev, int64_t m,
                  bool drop_last, const void* points_dev, int dtype,
                  const HullOutput& o) {
    hipStream_t s = pool.s;
    const int64_t fc = 2 * m;
    HullDev d = {};
    d.P = P_dev;
    d.m = (int)m;
    d.fc = (int)std::min<int64_t>(fc, INT32_MAX);
    double* bound_scratch = nullptr;
    double* bound = nullptr;
    int st = pool.Alloc(&d.w, 256);
    static_assert(sizeof(HullWords) <= 256, "the word block is 256 bytes");
    if (!st) st = AllocN(pool, &bound_scratch, MinMaxScratchDoubles());
    if (!st) st = AllocN(pool, &d.fv, 3 * (size_t)fc);
    if (!st) st = AllocN(pool, &d.fn, 3 * (size_t)fc);
    if (!st) st = AllocN(pool, &d.alive, (size_t)fc);
    if (!st) st = AllocN(pool, &d.sv, 3 * (size_t)fc);
    if (!st) st = AllocN(pool, &d.sn, 3 * (size_t)fc);
    if (!st) st = AllocN(pool, &d.best, (size_t)fc);
    if (!st) st = AllocN(pool, &d.cand, (size_t)fc);
    if (!st) st = AllocN(pool, &d.claim, (size_t)fc);
    if (!st) st = AllocN(pool, &d.owner, (size_t)fc);
    if (!st) st = AllocN(pool, &d.horizon, (size_t)fc);
    if (!st) st = AllocN(pool, &d.start, (size_t)fc);
    if (!st) st = AllocN(pool, &d.dead, (size_t)fc);
    if (!st) st = AllocN(pool, &d.base, (size_t)fc);
    if (!st) st = AllocN(pool, &d.dead_rank, (size_t)fc);
    if (!st) st = AllocN(pool, &d.dead_slot, (size_t)fc);
    if (!st) st = AllocN(pool, &d.conf, (size_t)m);
    if (!st) st = AllocN(pool, &d.live[0], (size_t)m);
    if (!st) st = AllocN(pool, &d.live[1], (size_t)m);
    if (!st) st = AllocN(pool, &d.keep, (size_t)m);
    if (!st) st = AllocN(pool, &d.pos, (size_t)m);
    if (!st) st = pool.Alloc(&d.scan_scratch, ScanScratchBytes(fc));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(d.w, 0, 256, s));
    O3DMI_HIP_CHECK(
            hipMemsetAsync(d.alive, 0, sizeof(int32_t) * (size_t)fc, s));
    if ((st = MinMaxBoundAsync(P_dev, m, O3DMI_F64, bound_scratch, &bound, s)))
        return st;
    d.bound = bound;

    if ((st = HullSimplexAsync(d, s))) return st;
    HullWords h = {};
    if ((st = Download(d.w, &h, sizeof(h), s))) return st;
    if (h.flat) {
        SetLastError(
                "convex hull: the points lie in one plane within eps "
                "(Qhull: QH6154, initial simplex is flat)");
        return O3DMI_ERR_SINGULAR;
    }

    bool sweep_only = false;
    int walk_cap = kHullWalkCap;
    ReadSwitches(&sweep_only, &walk_cap);
    int64_t n_facets = 4, n_live = h.nlive;
    int side = 0;
    int form = sweep_only ? kHullFormSweep : kHullFormWalk;
    int64_t stats[4] = {0, 0, 0, 0};
    // a walk round without a winner is followed by a sweep round, which always
    // has one: at most 2 m rounds
    for (int64_t round = 0; n_live > 0; ++round) {
        if (round > 2 * m + 2) {
            SetLastError("convex hull: the round bound was hit");
            return O3DMI_ERR_INTERNAL;
        }
        if ((st = HullRoundAsync(d, n_facets, n_live, side, form, walk_cap,
                                 s)))
            return st;
        if ((st = Download(d.w, &h, sizeof(h), s))) return st;
        const int64_t grown = std::max<int64_t>(h.newf - h.ndead, 0);
        if (h.err || n_facets + grown > fc ||
            (form == kHullFormSweep && h.winners == 0)) {
            SetLastError("convex hull: a cavity is not a disk");
            return O3DMI_ERR_INTERNAL;
        }
        ++stats[0];
        stats[1] += form == kHullFormSweep;
        stats[2] += (int64_t)h.winners;
        stats[3] += (int64_t)(h.cands - h.winners);
        n_facets += grown;
        n_live = h.nlive;
        side ^= 1;
        // the best candidate saw more facets than a walk holds
        form = (sweep_only || h.winners == 0) ? kHullFormSweep : kHullFormWalk;
    }
    for (int k = 0; k < 4; ++k) g_stats[k] = stats[k];

    int32_t *used = nullptr, *tri_keep = nullptr;
    int64_t *vrank = nullptr, *tpos = nullptr;
    st = AllocN(pool, &used, (size_t)m);
    if (!st) st = AllocN(pool, &vrank, (size_t)m);
    if (!st) st = AllocN(pool, &tri_keep, (size_t)n_facets);
    if (!st) st = AllocN(pool, &tpos, (size_t)n_facets);
    if (st) return st;
    if ((st = HullCountAsync(d, n_facets, drop_last, used, vrank, tri_keep,
                             tpos, s)))
        return st;
    if ((st = Download(d.w, &h, sizeof(h), s))) return st;
    const int64_t n_v = h.nverts, n_t = h.ntris;
    *o.n_vertices = n_v;
    *o.n_triangles = n_t;
    if (o.vertex_capacity < 0) return O3DMI_OK;
    if (o.vertex_capacity < n_v)
        return CapacityError("convex hull: vertex capacity too small");
    if (o.triangle_capacity < n_t)
        return CapacityError("convex hull: triangle capacity too small");

    uint32_t *rows = nullptr, *keys = nullptr, *perm = nullptr;
    void* sort_scratch = nullptr;
    st = AllocN(pool, &rows, 3 * (size_t)n_t);
    if (!st) st = AllocN(pool, &keys, (size_t)n_t);
    if (!st) st = AllocN(pool, &perm, (size_t)n_t);
    if (!st) st = pool.Alloc(&sort_scratch, SortPairsScratchBytes(n_t));
    if (st) return st;
    if ((st = HullEmitAsync(d, n_facets, n_v, n_t, used, vrank, tri_keep, tpos,
                            rows, keys, perm, sort_scratch, points_dev, dtype,
                            o.index_dtype, o.positions, o.point_indices,
                            o.triangles, s)))
        return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

namespace {

int ConvexHull(const void* points_dev, int64_t n, int dtype,
               const HullOutput& o, hipStream_t s) {
    int st = CheckCall(points_dev, n, 4, dtype, o);
    if (st) return st;
    PoolScratch pool(s);
    Words* w = nullptr;
    double* P = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    if ((st = AllocN(pool, &P, 3 * (size_t)n))) return st;
    if ((st = HullWidenAsync(points_dev, n, dtype, P, s))) return st;
    return HullOf(pool, P, n, false, points_dev, dtype, o);
}

int HiddenPointRemoval(const void* points_dev, int64_t n, int dtype,
                       const double* camera, double radius,
                       const HullOutput& o, hipStream_t s) {
    int st = CheckCall(points_dev, n, 3, dtype, o);
    if (st) return st;
    O3DMI_REQUIRE(camera, "null argument");
    O3DMI_REQUIRE(std::isfinite(camera[0]) && std::isfinite(camera[1]) &&
                          std::isfinite(camera[2]),
                  "camera_location must be finite");
    O3DMI_REQUIRE(std::isfinite(radius) && radius > 0,
                  "radius must be larger than zero.");
    PoolScratch pool(s);
    Words* w = nullptr;
    double* P = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    if ((st = AllocN(pool, &P, 3 * ((size_t)n + 1)))) return st;
    if ((st = HullFlipAsync(points_dev, n, dtype, camera, radius, P, &w->bad,
                            s)))
        return st;
    int bad = 0;
    if ((st = Download(&w->bad, &bad, sizeof(bad), s))) return st;
    O3DMI_REQUIRE(!bad,
                  "the spherical flip of a point is not finite (a point at "
                  "the camera location?)");
    return HullOf(pool, P, n + 1, true, points_dev, dtype, o);
}

}  // namespace

extern "C" {

int o3dmi_pointcloud_convex_hull(
        const void* points_dev, int64_t n, int dtype, void* positions_out_dev,
        void* point_indices_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity, int index_dtype,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream) {
    return ConvexHull(points_dev, n, dtype,
                      {positions_out_dev, point_indices_out_dev,
                       vertex_capacity, triangles_out_dev, triangle_capacity,
                       index_dtype, n_vertices_out, n_triangles_out},
                      (hipStream_t)stream);
}

int o3dmi_pointcloud_hidden_point_removal(
        const void* points_dev, int64_t n, int dtype,
        const double* camera_location, double radius, void* positions_out_dev,
        void* point_indices_out_dev, int64_t vertex_capacity,
        void* triangles_out_dev, int64_t triangle_capacity, int index_dtype,
        int64_t* n_vertices_out, int64_t* n_triangles_out,
        o3dmi_stream_t stream) {
    return HiddenPointRemoval(points_dev, n, dtype, camera_location, radius,
                              {positions_out_dev, point_indices_out_dev,
                               vertex_capacity, triangles_out_dev,
                               triangle_capacity, index_dtype, n_vertices_out,
                               n_triangles_out},
                              (hipStream_t)stream);
}

int o3dmi_internal_pointcloud_hull_stats(int64_t out[4]) {
    O3DMI_REQUIRE(out, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = g_stats[k];
    return O3DMI_OK;
}

}  // extern "C"
