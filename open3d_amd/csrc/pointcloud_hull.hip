// Kernels of PointCloud::ComputeConvexHull / HiddenPointRemoval
// (t/geometry/PointCloud.cpp:1608, 1668; upstream: Qhull on a host copy): a
// 3-D quickhull in float64 whose phases are launches over points, facets or
// winners (docs/pointcloud_convex_hull.md). The library is compiled with
// -ffp-contract=off: every expression below is evaluated as written. Atomics
// are integer only; a kernel boundary is the only grid-wide barrier.
#include <climits>

#include "pointcloud_hull.h"
#include "pointcloud_rows.h"
#include "scan.h"
#include "sort.h"

namespace o3dmi {
namespace {

constexpr int kNone = INT_MAX;

#define HULL_LAUNCH(kernel, count, s, ...)                                  \
    do {                                                                    \
        hipLaunchKernelGGL(kernel, dim3(GridFor((count), kHullBlock)),      \
                           dim3(kHullBlock), 0, (s), __VA_ARGS__);          \
        O3DMI_HIP_CHECK(hipGetLastError());                                 \
    } while (0)

// for (i = first index of this thread; i < n; i += all threads)
#define HULL_FOR(i, n)                                                      \
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;        \
         i < (int64_t)(n); i += (int64_t)gridDim.x * blockDim.x)

struct Vec3 {
    double x, y, z;
};

__device__ __forceinline__ Vec3 PointOf(const double* P, int i) {
    const double* r = P + 3 * (size_t)i;
    return {r[0], r[1], r[2]};
}

// The plane of facet (a, b, c): n = (b - a) x (c - a), its length, and a.
struct Plane {
    Vec3 n;
    double len;
    Vec3 a;
};

__device__ __forceinline__ Plane PlaneOf(const Vec3& a, const Vec3& b,
                                         const Vec3& c) {
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const double vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    Plane pl;
    pl.n.x = uy * vz - uz * vy;
    pl.n.y = uz * vx - ux * vz;
    pl.n.z = ux * vy - uy * vx;
    pl.len = sqrt((pl.n.x * pl.n.x + pl.n.y * pl.n.y) + pl.n.z * pl.n.z);
    pl.a = a;
    return pl;
}

// n . (p - a)
__device__ __forceinline__ double Above(const Plane& pl, const Vec3& p) {
    const double wx = p.x - pl.a.x, wy = p.y - pl.a.y, wz = p.z - pl.a.z;
    return (pl.n.x * wx + pl.n.y * wy) + pl.n.z * wz;
}

__device__ __forceinline__ bool Outside(const Plane& pl, const Vec3& p,
                                        double eps) {
    return Above(pl, p) > eps * pl.len;
}

__device__ __forceinline__ Plane FacetPlane(const double* P, const int* fv,
                                            int64_t f) {
    const int* v = fv + 3 * f;
    return PlaneOf(PointOf(P, v[0]), PointOf(P, v[1]), PointOf(P, v[2]));
}

// Bits whose unsigned order is the order of the finite doubles.
__device__ __forceinline__ unsigned long long OrderedKey(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// The largest key of the wave, in every lane. Every lane must call it.
__device__ __forceinline__ unsigned long long WaveMax(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64);
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        if (t > v) v = t;
    }
    return v;
}

// ---- input --------------------------------------------------------------------------
template <typename T>
__global__ void WidenKernel(const T* __restrict__ in, int64_t n3,
                            double* __restrict__ P) {
    HULL_FOR(i, n3) P[i] = (double)in[i];
}

// PointCloud::HiddenPointRemoval (geometry/PointCloud.cpp:797-808).
template <typename T>
__global__ void FlipKernel(const T* __restrict__ in, int64_t n, Vec3 camera,
                           double radius, double* __restrict__ P,
                           int* __restrict__ bad) {
    HULL_FOR(i, n + 1) {
        double* out = P + 3 * i;
        if (i == n) {
            out[0] = out[1] = out[2] = 0.0;
            continue;
        }
        const double vx = (double)in[3 * i] - camera.x;
        const double vy = (double)in[3 * i + 1] - camera.y;
        const double vz = (double)in[3 * i + 2] - camera.z;
        const double norm = sqrt((vx * vx + vy * vy) + vz * vz);
        const double k = 2.0 * (radius - norm);
        const double fx = vx + (k * vx) / norm;
        const double fy = vy + (k * vy) / norm;
        const double fz = vz + (k * vz) / norm;
        out[0] = fx;
        out[1] = fy;
        out[2] = fz;
        if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) atomicOr(bad, 1);
    }
}

// ---- the initial simplex ------------------------------------------------------------
__global__ void InitKernel(HullDev d) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    HullWords* w = d.w;
    for (int k = 0; k < 4; ++k) {
        w->key[k] = 0;
        w->p[k] = kNone;
    }
    const double* b = d.bound;
    double e = b[3] - b[0];
    if (b[4] - b[1] > e) e = b[4] - b[1];
    if (b[5] - b[2] > e) e = b[5] - b[2];
    w->eps = ((double)kHullEpsUlps * 0x1p-52) * e;
}

// The value stage `stage` maximises at point i: 0 -x, 1 x, 2 the squared
// distance from the line (p0, p1) times |p1 - p0|^2, 3 the distance from the
// plane (p0, p1, p2) times |n|. "+ 0.0": -0.0 and 0.0 are one value.
__device__ __forceinline__ double StageValue(const HullDev& d, int stage,
                                             int64_t i) {
    const Vec3 p = PointOf(d.P, (int)i);
    if (stage == 0) return -p.x + 0.0;
    if (stage == 1) return p.x + 0.0;
    const Vec3 a = PointOf(d.P, d.w->p[0]), b = PointOf(d.P, d.w->p[1]);
    if (stage == 2) {
        const double ex = b.x - a.x, ey = b.y - a.y, ez = b.z - a.z;
        const double wx = p.x - a.x, wy = p.y - a.y, wz = p.z - a.z;
        const double cx = wy * ez - wz * ey;
        const double cy = wz * ex - wx * ez;
        const double cz = wx * ey - wy * ex;
        return (cx * cx + cy * cy) + cz * cz;
    }
    const Plane pl = PlaneOf(a, b, PointOf(d.P, d.w->p[2]));
    return fabs(Above(pl, p));
}

__global__ void StageKeyKernel(HullDev d, int stage) {
    unsigned long long best = 0;
    HULL_FOR(i, d.m) {
        const unsigned long long k = OrderedKey(StageValue(d, stage, i));
        if (k > best) best = k;
    }
    best = WaveMax(best);
    if ((threadIdx.x & 63) == 0) atomicMax(&d.w->key[stage], best);
}

// Ties go to the lowest point index.
__global__ void StagePickKernel(HullDev d, int stage) {
    const unsigned long long key = d.w->key[stage];
    HULL_FOR(i, d.m)
        if (OrderedKey(StageValue(d, stage, i)) == key)
            atomicMin(&d.w->p[stage], (int)i);
}

// Facets 0..3 of the simplex (a, b, c, d), d below (a, b, c): (a, b, c),
// (a, d, b), (b, d, c), (c, d, a), and the facets across their edges.
__global__ void SimplexKernel(HullDev d) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    HullWords* w = d.w;
    int a = w->p[0], b = w->p[1], c = w->p[2], e = w->p[3];
    const Plane pl =
            PlaneOf(PointOf(d.P, a), PointOf(d.P, b), PointOf(d.P, c));
    const double h = Above(pl, PointOf(d.P, e));
    if (!(fabs(h) > w->eps * pl.len)) {
        w->flat = 1;
        return;
    }
    if (h > 0) {
        const int t = b;
        b = c;
        c = t;
    }
    const int v[12] = {a, b, c, a, e, b, b, e, c, c, e, a};
    const int nb[12] = {1, 2, 3, 3, 2, 0, 1, 3, 0, 2, 1, 0};
    for (int k = 0; k < 12; ++k) {
        d.fv[k] = v[k];
        d.fn[k] = nb[k];
    }
    for (int f = 0; f < 4; ++f) d.alive[f] = 1;
}

// The lowest of the four facets point i is outside of; the simplex's own
// points and the points outside of nothing are dead.
__global__ void AssignKernel(HullDev d) {
    const HullWords* w = d.w;
    if (w->flat) {
        HULL_FOR(i, d.m) {
            d.conf[i] = -1;
            d.keep[i] = 0;
            d.live[0][i] = (int)i;
        }
        return;
    }
    const double eps = w->eps;
    HULL_FOR(i, d.m) {
        int f = -1;
        if (i != w->p[0] && i != w->p[1] && i != w->p[2] && i != w->p[3]) {
            const Vec3 p = PointOf(d.P, (int)i);
            for (int g = 3; g >= 0; --g)
                if (Outside(FacetPlane(d.P, d.fv, g), p, eps)) f = g;
        }
        d.conf[i] = f;
        d.keep[i] = f >= 0;
        d.live[0][i] = (int)i;
    }
}

// next[pos[j]] = cur[j] for the kept entries: the list keeps its order.
__global__ void CompactKernel(const int* __restrict__ cur,
                              const int32_t* __restrict__ keep,
                              const int64_t* __restrict__ pos, int64_t n,
                              int* __restrict__ next) {
    HULL_FOR(j, n)
        if (keep[j]) next[pos[j]] = cur[j];
}

// ---- one round ----------------------------------------------------------------------
__global__ void ResetKernel(HullDev d, int64_t nf) {
    HULL_FOR(f, nf) {
        d.best[f] = 0;
        d.cand[f] = kNone;
        d.claim[f] = kNone;
        d.owner[f] = -1;
        d.horizon[f] = 0;
        d.start[f] = kNone;
        d.dead[f] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d.w->best_pt = kNone;
        d.w->winners = 0;
        d.w->cands = 0;
    }
}

// (a) pass one: best[f] = the bits of the largest n . (p - a) among the points
// of facet f (positive, so the bits order as the values do). A wave whose
// lanes all hold points of one facet sends one atomic.
__global__ void FarthestKernel(HullDev d, const int* __restrict__ live,
                               int64_t nl) {
    const int64_t rounds = Rounds(nl);
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t j = (r * gridDim.x + blockIdx.x) * (int64_t)blockDim.x +
                          threadIdx.x;
        int f = -1;
        unsigned long long bits = 0;
        if (j < nl) {
            const int q = live[j];
            f = d.conf[q];
            bits = (unsigned long long)__double_as_longlong(
                    Above(FacetPlane(d.P, d.fv, f), PointOf(d.P, q)));
        }
        const int f0 = __shfl(f, 0, 64);
        const bool uniform =
                __builtin_amdgcn_ballot_w64(f != f0) == 0 && f0 >= 0;
        if (uniform) {
            const unsigned long long m = WaveMax(bits);
            if ((threadIdx.x & 63) == 0) atomicMax(&d.best[f0], m);
        } else if (f >= 0) {
            atomicMax(&d.best[f], bits);
        }
    }
}

// (a) pass two: the lowest point index among those that reach best[f].
__global__ void CandidateKernel(HullDev d, const int* __restrict__ live,
                                int64_t nl) {
    HULL_FOR(j, nl) {
        const int q = live[j];
        const int f = d.conf[q];
        const unsigned long long bits =
                (unsigned long long)__double_as_longlong(
                        Above(FacetPlane(d.P, d.fv, f), PointOf(d.P, q)));
        if (bits == d.best[f]) {
            atomicMin(&d.cand[f], q);
            atomicMin(&d.w->best_pt, q);
        }
    }
}

// The facets visible from point q that can be reached from f0 over visible
// facets, breadth first, into vis[0 .. cap); ring(h) for every facet across
// the horizon (possibly more than once). Returns their number, or -1 past cap.
template <class Ring>
__device__ __forceinline__ int WalkCavity(const HullDev& d, int f0,
                                          const Vec3& p, double eps, int cap,
                                          int* vis, Ring ring) {
    int cnt = 1, head = 0;
    vis[0] = f0;
    while (head < cnt) {  // at most cap rounds: head < cnt <= cap
        const int g = vis[head++];
        for (int k = 0; k < 3; ++k) {
            const int h = d.fn[3 * (int64_t)g + k];
            bool seen = false;
            for (int t = 0; t < cnt; ++t) seen |= vis[t] == h;
            if (seen) continue;
            if (Outside(FacetPlane(d.P, d.fv, h), p, eps)) {
                if (cnt == cap) return -1;
                vis[cnt++] = h;
            } else {
                ring(h);
            }
        }
    }
    return cnt;
}

// (b) every candidate claims its cavity and the ring across its horizon with
// its point index; the lowest index keeps a facet.
__global__ void ClaimKernel(HullDev d, int64_t nf, int cap) {
    const double eps = d.w->eps;
    HULL_FOR(f, nf) {
        const int q = d.cand[f];
        if (q == kNone) continue;
        int vis[kHullWalkCap];
        int* claim = d.claim;
        const int cnt =
                WalkCavity(d, (int)f, PointOf(d.P, q), eps, cap, vis,
                           [claim, q](int h) { atomicMin(&claim[h], q); });
        // past the cap the candidate cannot win; what it claimed only holds
        // back candidates of a higher index
        const int held = cnt < 0 ? cap : cnt;
        for (int t = 0; t < held; ++t) atomicMin(&claim[vis[t]], q);
    }
}

// (c) a candidate wins iff it kept every claim: owner[g] = its facet for the
// facets of its cavity.
__global__ void WinKernel(HullDev d, int64_t nf, int cap) {
    const double eps = d.w->eps;
    const int64_t rounds = Rounds(nf);
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t f = (r * gridDim.x + blockIdx.x) * (int64_t)blockDim.x +
                          threadIdx.x;
        const int q = f < nf ? d.cand[f] : kNone;
        bool won = false;
        if (q != kNone) {
            int vis[kHullWalkCap];
            bool mine = true;
            const int* claim = d.claim;
            const int cnt = WalkCavity(
                    d, (int)f, PointOf(d.P, q), eps, cap, vis,
                    [claim, q, &mine](int h) { mine &= claim[h] == q; });
            if (cnt > 0) {
                for (int t = 0; t < cnt; ++t) mine &= claim[vis[t]] == q;
                if (mine) {
                    for (int t = 0; t < cnt; ++t) d.owner[vis[t]] = (int)f;
                    won = true;
                }
            }
        }
        CountKept(q != kNone, &d.w->cands);
        CountKept(won, &d.w->winners);
    }
}

// The sweep form of (b) and (c): the best candidate alone, every facet tested.
__global__ void SweepKernel(HullDev d, int64_t nf) {
    const int q = d.w->best_pt;
    if (q == kNone) return;
    const int f0 = d.conf[q];
    const Vec3 p = PointOf(d.P, q);
    const double eps = d.w->eps;
    HULL_FOR(g, nf)
        if (d.alive[g] &&
            (g == f0 || Outside(FacetPlane(d.P, d.fv, g), p, eps)))
            d.owner[g] = f0;
}

__global__ void SweepWinKernel(HullDev d) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int q = d.w->best_pt;
    if (q == kNone) return;
    d.w->winners = 1;
    d.w->cands = 1;
}

// dead[g] = 1 for the free slots: the facets of a cavity and the slots left
// free by earlier rounds; horizon[w] = the number of horizon edges of winner
// w, start[w] = the lowest of them, 3 g + k.
__global__ void MarkKernel(HullDev d, int64_t nf) {
    HULL_FOR(g, nf) {
        const int w = d.owner[g];
        if (w < 0) {
            d.dead[g] = !d.alive[g];
            continue;
        }
        d.dead[g] = 1;
        d.alive[g] = 0;
        for (int k = 0; k < 3; ++k)
            if (d.owner[d.fn[3 * g + k]] != w) {
                atomicAdd(&d.horizon[w], 1);
                atomicMin(&d.start[w], (int)(3 * g + k));
            }
    }
}

__global__ void DeadSlotKernel(HullDev d, int64_t nf) {
    HULL_FOR(g, nf)
        if (d.dead[g]) d.dead_slot[d.dead_rank[g]] = (int)g;
}

// The slot new facet j of the round takes: the free slots in ascending order
// first, then the end of the list. A cavity of D facets with I vertices in its
// interior has D + 2 - 2 I horizon edges, so a round may free more slots than
// it fills; they stay free for later rounds and the list never grows past the
// largest number of live facets.
__device__ __forceinline__ int64_t SlotOf(const HullDev& d, int64_t nf,
                                          int64_t j) {
    const int64_t nd = d.w->ndead;
    return j < nd ? d.dead_slot[j] : nf + (j - nd);
}

// The edge k of facet h that runs from `from` to `to`, or -1.
__device__ __forceinline__ int EdgeOf(const int* fv, int64_t h, int from,
                                      int to) {
    const int* v = fv + 3 * h;
    for (int k = 0; k < 3; ++k)
        if (v[k] == from && v[(k + 1) % 3] == to) return k;
    return -1;
}

// (e) winner w walks its horizon cycle from start[w]: new facet i is (u, v,
// q) over horizon edge (u, v); across (u, v) lies the ring facet, across (v,
// q) facet i + 1, across (q, u) facet i - 1. The ring facet's entry for that
// edge is rewritten here, by this winner alone.
__global__ void ConeKernel(HullDev d, int64_t nf) {
    HULL_FOR(f, nf) {
        const int hn = d.horizon[f];
        if (hn == 0) continue;
        const int q = d.cand[f];
        const int e0 = d.start[f];
        const int64_t b = d.base[f];
        if (e0 == kNone || b + hn > d.fc) {
            atomicOr(&d.w->err, 1);
            continue;
        }
        int64_t g = e0 / 3;
        int k = e0 % 3;
        int64_t steps = 0;  // every turn around a horizon vertex, summed
        bool ok = true;
        for (int i = 0; i < hn && ok; ++i) {
            const int u = d.fv[3 * g + k], v = d.fv[3 * g + (k + 1) % 3];
            const int h = d.fn[3 * g + k];
            const int64_t j = b + i;
            const int64_t slot = SlotOf(d, nf, j);
            const int64_t next = SlotOf(d, nf, b + (i + 1) % hn);
            const int64_t prev = SlotOf(d, nf, b + (i + hn - 1) % hn);
            const int back = EdgeOf(d.fv, h, v, u);
            if (back < 0 || slot >= d.fc || next >= d.fc || prev >= d.fc) {
                ok = false;
                break;
            }
            d.sv[3 * j] = u;
            d.sv[3 * j + 1] = v;
            d.sv[3 * j + 2] = q;
            d.sn[3 * j] = h;
            d.sn[3 * j + 1] = (int)next;
            d.sn[3 * j + 2] = (int)prev;
            d.fn[3 * (int64_t)h + back] = (int)slot;
            // the horizon edge that starts at v: turn around v through the
            // cavity
            k = (k + 1) % 3;
            while (true) {
                const int h2 = d.fn[3 * g + k];
                if (d.owner[h2] != (int)f) break;
                if (++steps > 3 * nf) {
                    ok = false;
                    break;
                }
                const int x = d.fv[3 * g + (k + 1) % 3];
                const int m = EdgeOf(d.fv, h2, x, v);
                if (m < 0) {
                    ok = false;
                    break;
                }
                g = h2;
                k = (m + 1) % 3;
            }
        }
        if (!ok || 3 * g + k != e0) atomicOr(&d.w->err, 1);
    }
}

// (f) a point whose facet died takes the lowest slot among its winner's new
// facets it is outside of, or it is dropped; the winner's point itself is
// dropped.
__global__ void RetestKernel(HullDev d, const int* __restrict__ live,
                             int64_t nl, int64_t nf) {
    const double eps = d.w->eps;
    HULL_FOR(j, nl) {
        const int q = live[j];
        const int w = d.owner[d.conf[q]];
        if (w < 0) {
            d.keep[j] = 1;
            continue;
        }
        int64_t best = -1;
        if (q != d.cand[w]) {
            const Vec3 p = PointOf(d.P, q);
            const int64_t b = d.base[w];
            const int hn = d.horizon[w];
            for (int i = 0; i < hn; ++i) {
                if (b + i >= d.fc) break;  // ConeKernel has set err
                if (!Outside(FacetPlane(d.P, d.sv, b + i), p, eps)) continue;
                const int64_t slot = SlotOf(d, nf, b + i);
                if (best < 0 || slot < best) best = slot;
            }
        }
        d.conf[q] = (int)best;
        d.keep[j] = best >= 0;
    }
}

__global__ void PlaceKernel(HullDev d, int64_t nf) {
    int64_t n_new = d.w->newf;
    if (n_new > d.fc) n_new = d.fc;  // ConeKernel has set err
    HULL_FOR(j, n_new) {
        const int64_t slot = SlotOf(d, nf, j);
        if (slot >= d.fc) continue;
        for (int k = 0; k < 3; ++k) {
            d.fv[3 * slot + k] = d.sv[3 * j + k];
            d.fn[3 * slot + k] = d.sn[3 * j + k];
        }
        d.alive[slot] = 1;
    }
}

// ---- output -------------------------------------------------------------------------
__global__ void UsedKernel(HullDev d, int64_t nf, int drop,
                           int32_t* __restrict__ used,
                           int32_t* __restrict__ tri_keep) {
    HULL_FOR(f, nf) {
        const int* v = d.fv + 3 * f;
        const bool keep =
                d.alive[f] &&
                !(drop >= 0 && (v[0] == drop || v[1] == drop || v[2] == drop));
        tri_keep[f] = keep;
        if (keep)
            for (int k = 0; k < 3; ++k) used[v[k]] = 1;
    }
}

// rows[tpos[f]] = the facet in output vertex numbers, its lowest first.
__global__ void RowsKernel(HullDev d, int64_t nf,
                           const int32_t* __restrict__ tri_keep,
                           const int64_t* __restrict__ tpos,
                           const int64_t* __restrict__ vrank,
                           uint32_t* __restrict__ rows) {
    HULL_FOR(f, nf) {
        if (!tri_keep[f]) continue;
        const int* v = d.fv + 3 * f;
        const uint32_t r[3] = {(uint32_t)vrank[v[0]], (uint32_t)vrank[v[1]],
                               (uint32_t)vrank[v[2]]};
        int lo = 0;
        if (r[1] < r[lo]) lo = 1;
        if (r[2] < r[lo]) lo = 2;
        uint32_t* out = rows + 3 * tpos[f];
        for (int k = 0; k < 3; ++k) out[k] = r[(lo + k) % 3];
    }
}

// keys[i] = column c of row perm[i] (perm == nullptr: row i, and vals[i] = i).
__global__ void ColumnKernel(const uint32_t* __restrict__ rows, int64_t t,
                             int c, const uint32_t* __restrict__ perm,
                             uint32_t* __restrict__ keys,
                             uint32_t* __restrict__ vals) {
    HULL_FOR(i, t) {
        const int64_t r = perm ? perm[i] : i;
        keys[i] = rows[3 * r + c];
        if (vals) vals[i] = (uint32_t)i;
    }
}

template <typename I>
__global__ void TrianglesOutKernel(const uint32_t* __restrict__ rows,
                                   const uint32_t* __restrict__ perm,
                                   int64_t t, I* __restrict__ out) {
    HULL_FOR(i, t)
        for (int k = 0; k < 3; ++k)
            out[3 * i + k] = (I)rows[3 * (int64_t)perm[i] + k];
}

template <typename T, typename I>
__global__ void VerticesOutKernel(const T* __restrict__ points, int64_t m,
                                  const int32_t* __restrict__ used,
                                  const int64_t* __restrict__ vrank,
                                  T* __restrict__ positions,
                                  I* __restrict__ indices) {
    HULL_FOR(i, m) {
        if (!used[i]) continue;
        const int64_t r = vrank[i];
        for (int k = 0; k < 3; ++k) positions[3 * r + k] = points[3 * i + k];
        indices[r] = (I)i;
    }
}

int CompactLive(const HullDev& d, int64_t n, int side, hipStream_t s) {
    const int st = PrefixSumAsync(d.keep, n, false, d.pos,
                                  (int64_t*)&d.w->nlive, d.scan_scratch, s);
    if (st) return st;
    HULL_LAUNCH(CompactKernel, n, s, d.live[side], d.keep, d.pos, n,
                d.live[side ^ 1]);
    return O3DMI_OK;
}

}  // namespace

int HullWidenAsync(const void* points_dev, int64_t n, int dtype, double* P_dev,
                   hipStream_t s) {
    if (dtype == O3DMI_F64)
        HULL_LAUNCH(WidenKernel<double>, 3 * n, s, (const double*)points_dev,
                    3 * n, P_dev);
    else
        HULL_LAUNCH(WidenKernel<float>, 3 * n, s, (const float*)points_dev,
                    3 * n, P_dev);
    return O3DMI_OK;
}

int HullFlipAsync(const void* points_dev, int64_t n, int dtype,
                  const double camera[3], double radius, double* P_dev,
                  int* bad_dev, hipStream_t s) {
    const Vec3 c = {camera[0], camera[1], camera[2]};
    if (dtype == O3DMI_F64)
        HULL_LAUNCH(FlipKernel<double>, n + 1, s, (const double*)points_dev, n,
                    c, radius, P_dev, bad_dev);
    else
        HULL_LAUNCH(FlipKernel<float>, n + 1, s, (const float*)points_dev, n,
                    c, radius, P_dev, bad_dev);
    return O3DMI_OK;
}

int HullSimplexAsync(const HullDev& d, hipStream_t s) {
    HULL_LAUNCH(InitKernel, 1, s, d);
    // stages 0 and 1 depend on nothing, 2 on both, 3 on 2
    for (int stage = 0; stage < 2; ++stage)
        HULL_LAUNCH(StageKeyKernel, d.m, s, d, stage);
    for (int stage = 0; stage < 2; ++stage)
        HULL_LAUNCH(StagePickKernel, d.m, s, d, stage);
    for (int stage = 2; stage < 4; ++stage) {
        HULL_LAUNCH(StageKeyKernel, d.m, s, d, stage);
        HULL_LAUNCH(StagePickKernel, d.m, s, d, stage);
    }
    HULL_LAUNCH(SimplexKernel, 1, s, d);
    HULL_LAUNCH(AssignKernel, d.m, s, d);
    // into live[1], then back: the list of a round starts in live[side]
    int st = CompactLive(d, d.m, 0, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(d.live[0], d.live[1],
                                   sizeof(int) * (size_t)d.m,
                                   hipMemcpyDeviceToDevice, s));
    return O3DMI_OK;
}

int HullRoundAsync(const HullDev& d, int64_t nf, int64_t nl, int side,
                   int form, int walk_cap, hipStream_t s) {
    const int* live = d.live[side];
    HULL_LAUNCH(ResetKernel, nf, s, d, nf);
    HULL_LAUNCH(FarthestKernel, nl, s, d, live, nl);
    HULL_LAUNCH(CandidateKernel, nl, s, d, live, nl);
    if (form == kHullFormWalk) {
        HULL_LAUNCH(ClaimKernel, nf, s, d, nf, walk_cap);
        HULL_LAUNCH(WinKernel, nf, s, d, nf, walk_cap);
    } else {
        HULL_LAUNCH(SweepKernel, nf, s, d, nf);
        HULL_LAUNCH(SweepWinKernel, 1, s, d);
    }
    HULL_LAUNCH(MarkKernel, nf, s, d, nf);
    // (d) the winners' horizon lengths and the free slots, numbered by scans
    int st = PrefixSumAsync(d.horizon, nf, false, d.base,
                            (int64_t*)&d.w->newf, d.scan_scratch, s);
    if (st) return st;
    if ((st = PrefixSumAsync(d.dead, nf, false, d.dead_rank,
                             (int64_t*)&d.w->ndead, d.scan_scratch, s)))
        return st;
    HULL_LAUNCH(DeadSlotKernel, nf, s, d, nf);
    HULL_LAUNCH(ConeKernel, nf, s, d, nf);
    HULL_LAUNCH(RetestKernel, nl, s, d, live, nl, nf);
    // (g) the new facets take the free slots, then the end of the list
    HULL_LAUNCH(PlaceKernel, d.fc, s, d, nf);
    return CompactLive(d, nl, side, s);
}

int HullCountAsync(const HullDev& d, int64_t nf, bool drop_last,
                   int32_t* used_dev, int64_t* vrank_dev, int32_t* tri_keep_dev,
                   int64_t* tpos_dev, hipStream_t s) {
    O3DMI_HIP_CHECK(
            hipMemsetAsync(used_dev, 0, sizeof(int32_t) * (size_t)d.m, s));
    HULL_LAUNCH(UsedKernel, nf, s, d, nf, drop_last ? d.m - 1 : -1, used_dev,
                tri_keep_dev);
    int st = PrefixSumAsync(used_dev, d.m, false, vrank_dev,
                            (int64_t*)&d.w->nverts, d.scan_scratch, s);
    if (st) return st;
    return PrefixSumAsync(tri_keep_dev, nf, false, tpos_dev,
                          (int64_t*)&d.w->ntris, d.scan_scratch, s);
}

int HullEmitAsync(const HullDev& d, int64_t nf, int64_t n_verts,
                  int64_t n_tris, const int32_t* used_dev,
                  const int64_t* vrank_dev, const int32_t* tri_keep_dev,
                  const int64_t* tpos_dev, uint32_t* rows_dev,
                  uint32_t* keys_dev, uint32_t* perm_dev, void* sort_scratch,
                  const void* points_dev, int dtype, int index_dtype,
                  void* positions_out_dev, void* point_indices_out_dev,
                  void* triangles_out_dev, hipStream_t s) {
    const int64_t t = n_tris;
    if (t > 0) {
        HULL_LAUNCH(RowsKernel, nf, s, d, nf, tri_keep_dev, tpos_dev,
                    vrank_dev, rows_dev);
        // three stable passes, least significant column first
        const int bits = BitsFor(n_verts);
        for (int c = 2; c >= 0; --c) {
            HULL_LAUNCH(ColumnKernel, t, s, rows_dev, t, c,
                        c == 2 ? (const uint32_t*)nullptr : perm_dev, keys_dev,
                        c == 2 ? perm_dev : (uint32_t*)nullptr);
            const int st = SortPairsAsync(keys_dev, perm_dev, t, bits,
                                          sort_scratch, s);
            if (st) return st;
        }
        if (index_dtype == O3DMI_I64)
            HULL_LAUNCH(TrianglesOutKernel<int64_t>, t, s, rows_dev, perm_dev,
                        t, (int64_t*)triangles_out_dev);
        else
            HULL_LAUNCH(TrianglesOutKernel<int32_t>, t, s, rows_dev, perm_dev,
                        t, (int32_t*)triangles_out_dev);
    }
    // the dropped origin of hidden-point removal is point m - 1 and not used
    const int64_t m = d.m;
#define HULL_VERTS(T, I)                                                     \
    HULL_LAUNCH((VerticesOutKernel<T, I>), m, s, (const T*)points_dev, m,   \
                used_dev, vrank_dev, (T*)positions_out_dev,                  \
                (I*)point_indices_out_dev)
    if (dtype == O3DMI_F64 && index_dtype == O3DMI_I64)
        HULL_VERTS(double, int64_t);
    else if (dtype == O3DMI_F64)
        HULL_VERTS(double, int32_t);
    else if (index_dtype == O3DMI_I64)
        HULL_VERTS(float, int64_t);
    else
        HULL_VERTS(float, int32_t);
#undef HULL_VERTS
    return O3DMI_OK;
}

}  // namespace o3dmi
