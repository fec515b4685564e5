// Private seam between the kernels of PointCloud::ComputeConvexHull /
// HiddenPointRemoval (pointcloud_hull.hip) and their C ABI in
// host/pointcloud_hull.cpp: a 3-D quickhull whose every phase is a launch over
// points, facets or winners (docs/pointcloud_convex_hull.md). Every launcher is
// stream-ordered and waits for nothing; no kernel waits for another workgroup,
// and every device loop is bounded by the facet count it is given.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace o3dmi {

// Point p is outside facet (a, b, c), n = (b - a) x (c - a), iff
// n . (p - a) > eps |n| with eps = kHullEpsUlps * 2^-52 * E, E the largest
// extent of the bounding box. 16 u |b - a| |c - a| |p - a| bounds the rounding
// error of the left side (u = 2^-53), so 256 covers every facet whose angle at
// a is above 3.2 degrees (docs/pointcloud_convex_hull.md).
constexpr int kHullEpsUlps = 256;
constexpr int kHullBlock = kBlock;
// Facets a candidate's walk may hold (thread-private list). A candidate that
// sees more does not win; when that is the best candidate, the driver runs the
// round in the sweep form.
constexpr int kHullWalkCap = 64;

// Forms of the candidate step of a round.
constexpr int kHullFormWalk = 0;   // one thread per candidate walks its cavity
constexpr int kHullFormSweep = 1;  // the best candidate alone, all facets swept

// The device word block of a call (zeroed by the driver; HullSimplexAsync
// sets the simplex words and eps). The driver downloads it once per round.
struct HullWords {
    unsigned long long key[4];  // ordered bits of the simplex stages' maxima
    int p[4];                   // the simplex: min x, max x, line, plane
    double eps;
    int flat;     // the fourth point is not outside the plane of the first three
    int err;      // a bound was hit or the cavity is no disk
    int bad;      // a flipped coordinate is not finite
    int best_pt;  // lowest candidate point of the round
    unsigned long long winners;  // this round
    unsigned long long cands;    // this round
    long long newf;              // new facets of this round
    long long ndead;             // free slots: dead facets, old and new
    long long nlive;             // points that still have a conflict facet
    long long nverts;            // the output's counts
    long long ntris;
};

// Every array of a hull over m points; fc = 2 m facet slots.
struct HullDev {
    const double* P;  // {m,3}
    int m;
    int fc;
    HullWords* w;
    const double* bound;  // {min x, y, z, max x, y, z} of P
    // facets: vertices (counter-clockwise from outside) and the facet across
    // edge k = (v[k], v[(k + 1) % 3])
    int* fv;
    int* fn;
    int32_t* alive;  // 0 for a slot that holds no facet (zeroed by the caller)
    // per facet, per round
    unsigned long long* best;
    int* cand;
    int* claim;
    int* owner;
    int32_t* horizon;
    int* start;
    int32_t* dead;
    int64_t* base;
    int64_t* dead_rank;
    int* dead_slot;
    int* sv;  // the round's new facets before they take their slots
    int* sn;
    // per point
    int* conf;
    int* live[2];
    int32_t* keep;
    int64_t* pos;
    void* scan_scratch;
};

// P[i] = the point widened.
int HullWidenAsync(const void* points_dev, int64_t n, int dtype, double* P_dev,
                   hipStream_t s);
// P[i] = upstream's spherical flip of point i, P[n] = (0, 0, 0); *bad_dev |= 1
// for a flipped coordinate that is not finite.
int HullFlipAsync(const void* points_dev, int64_t n, int dtype,
                  const double camera[3], double radius, double* P_dev,
                  int* bad_dev, hipStream_t s);

// The initial simplex, its four facets, every point's conflict facet and the
// list of live points (w->flat, w->nlive). live[0] holds the list.
int HullSimplexAsync(const HullDev& d, hipStream_t s);

// One round over n_facets facet slots and n_live points listed in live[side]: the
// candidates, their claims (walk form, walk_cap <= kHullWalkCap facets each)
// or the best candidate's sweep, the winners' cones, the re-test of the points
// whose facet died and the new list in live[side ^ 1] (w->winners, w->cands,
// w->newf, w->ndead, w->nlive, w->err). The slots in use grow by newf - ndead
// when that is positive.
int HullRoundAsync(const HullDev& d, int64_t n_facets, int64_t n_live,
                   int side, int form, int walk_cap, hipStream_t s);

// used[i] = 1 for the vertices of the kept facets, tri_keep[f] = 1 for the
// kept facets (drop_last: every facet that names point m - 1 goes, and so does
// that point); their exclusive scans and totals (w->nverts, w->ntris).
int HullCountAsync(const HullDev& d, int64_t n_facets, bool drop_last,
                   int32_t* used_dev, int64_t* vrank_dev, int32_t* tri_keep_dev,
                   int64_t* tpos_dev, hipStream_t s);

// The canonical output: vertices in ascending point index as bit copies of the
// input rows, triangles rotated to their lowest vertex and sorted by (v0, v1,
// v2). rows_dev: 3 * T uint32; keys / perm: T uint32 each.
int HullEmitAsync(const HullDev& d, int64_t n_facets, int64_t n_verts,
                  int64_t n_tris, const int32_t* used_dev,
                  const int64_t* vrank_dev, const int32_t* tri_keep_dev,
                  const int64_t* tpos_dev, uint32_t* rows_dev,
                  uint32_t* keys_dev, uint32_t* perm_dev, void* sort_scratch,
                  const void* points_dev, int dtype, int index_dtype,
                  void* positions_out_dev, void* point_indices_out_dev,
                  void* triangles_out_dev, hipStream_t s);

}  // namespace o3dmi

// What the last hull call of this thread did: {rounds, sweep rounds, winners,
// candidates that did not win} (tools/bench_convex_hull.py).
extern "C" int o3dmi_internal_pointcloud_hull_stats(int64_t out[4]);
