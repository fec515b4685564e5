// Kernels of the mesh topology and intersection queries (trianglemesh_
// topology.h): flag counting, the wedge union-find of GetNonManifoldVertices,
// the double cover of OrientTriangles, the box-query traversal of the mesh
// BVH with the exact float64 triangle-triangle test at its leaves, and the
// tetrahedron terms of GetVolume.
#include "trianglemesh_topology.h"

#include <climits>

#include "mesh_launch.h"
#include "union_find.h"

namespace o3dmi {
namespace {

// Coordinate k of vertex u, widened.
__device__ __forceinline__ double Coord(const void* __restrict__ pos,
                                        int dtype, int64_t u, int k) {
    return dtype == O3DMI_F64 ? ((const double*)pos)[3 * u + k]
                              : (double)((const float*)pos)[3 * u + k];
}

// ---- counting ---------------------------------------------------------------------
__global__ void CountFlagsKernel(const int32_t* __restrict__ flags, int64_t n,
                                 unsigned long long* __restrict__ count) {
    unsigned long long sum = 0;
    O3DMI_GRID_STRIDE(i, n) sum += (unsigned long long)(flags[i] != 0);
    for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(count, sum);
}

// ---- non-manifold vertices ----------------------------------------------------------
// The corner of slot e's triangle that names x, one of the slot's two ends.
__device__ __forceinline__ int CornerAt(const int32_t* __restrict__ tri,
                                        uint32_t e, uint32_t x) {
    const uint32_t t = e / 3u, k = e - 3u * t;
    return (uint32_t)tri[e] == x ? (int)e
                                 : (int)(3u * t + (k == 2u ? 0u : k + 1u));
}

// A slot that continues a run with lo != hi unites its corners at lo and at
// hi with those of the slot before it.
__global__ void WedgeUnionKernel(EdgeTable tb, const int32_t* __restrict__ tri,
                                 int64_t n3, int* __restrict__ parent) {
    O3DMI_GRID_STRIDE(j, n3) {
        if (FirstOfRun(tb, j)) continue;
        const uint32_t lo = tb.lo[j], hi = tb.hi[j];
        if (lo == hi) continue;
        const uint32_t e = tb.slot[j], ep = tb.slot[j - 1];
        DbscanUnite(parent, CornerAt(tri, e, lo), CornerAt(tri, ep, lo));
        DbscanUnite(parent, CornerAt(tri, e, hi), CornerAt(tri, ep, hi));
    }
}

// rootw[c] = the root of corner c when it is a wedge (its vertex occurs once
// in its triangle), else -1.
__global__ void WedgeRootKernel(const int32_t* __restrict__ tri, int64_t n3,
                                int* __restrict__ parent,
                                int* __restrict__ rootw) {
    O3DMI_GRID_STRIDE(c, n3) {
        const int64_t t = c / 3;
        const int k = (int)(c - 3 * t);
        const int32_t x = tri[c];
        const int32_t o1 = tri[3 * t + (k == 2 ? 0 : k + 1)];
        const int32_t o2 = tri[3 * t + (k == 0 ? 2 : k - 1)];
        rootw[c] = (o1 != x && o2 != x) ? DbscanFind(parent, (int)c) : -1;
    }
}

__global__ void VertexFlagsThreadKernel(CornerTable tb, int64_t v,
                                        const int* __restrict__ rootw,
                                        int32_t* __restrict__ long_list,
                                        int32_t* __restrict__ flags) {
    O3DMI_GRID_STRIDE(u, v) {
        const int cnt = tb.count[u];
        if (cnt > kLongCornerList) {
            long_list[atomicAdd(&long_list[v], 1)] = (int32_t)u;
            continue;
        }
        const uint32_t* corner = tb.corner + tb.start[u];
        int mn = INT_MAX, mx = -1;
        for (int j = 0; j < cnt; ++j) {
            const int r = rootw[corner[j]];
            if (r >= 0) {
                mn = r < mn ? r : mn;
                mx = r > mx ? r : mx;
            }
        }
        flags[u] = mx >= 0 && mn != mx;
    }
}

// A wave per listed vertex: the lanes take the corners 64 at a time.
__global__ void VertexFlagsWaveKernel(CornerTable tb, int64_t v,
                                      const int* __restrict__ rootw,
                                      const int32_t* __restrict__ long_list,
                                      int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[v];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t u = long_list[w];
        const int cnt = tb.count[u];
        const uint32_t* corner = tb.corner + tb.start[u];
        int mn = INT_MAX, mx = -1;
        for (int j = lane; j < cnt; j += 64) {
            const int r = rootw[corner[j]];
            if (r >= 0) {
                mn = r < mn ? r : mn;
                mx = r > mx ? r : mx;
            }
        }
        for (int x = 32; x > 0; x >>= 1) {
            const int omn = __shfl_xor(mn, x), omx = __shfl_xor(mx, x);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
        }
        if (lane == 0) flags[u] = mx >= 0 && mn != mx;
    }
}

template <typename I>
__global__ void EmitFlaggedKernel(const int32_t* __restrict__ flags,
                                  const int64_t* __restrict__ pos, int64_t n,
                                  I* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, n) {
        if (flags[i]) out[pos[i]] = (I)i;
    }
}

// ---- orientation ------------------------------------------------------------------------
__device__ __forceinline__ bool Forward(const int32_t* __restrict__ tri,
                                        uint32_t e) {
    const uint32_t t = e / 3u, k = e - 3u * t;
    return tri[e] < tri[3u * t + (k == 2u ? 0u : k + 1u)];
}

__global__ void OrientUnionKernel(EdgeTable tb, const int32_t* __restrict__ tri,
                                  int64_t n3, int* __restrict__ parent,
                                  int* __restrict__ bad) {
    O3DMI_GRID_STRIDE(j, n3) {
        if (!FirstOfRun(tb, j)) continue;
        if (tb.lo[j] == tb.hi[j]) continue;
        int mult = 1;
        while (mult < 3 && j + mult < n3 && SameEdge(tb, j, j + mult)) ++mult;
        if (mult > 2) {
            atomicOr(bad, 1);
        } else if (mult == 2) {
            const uint32_t e0 = tb.slot[j], e1 = tb.slot[j + 1];
            const int t = (int)(e0 / 3u), u = (int)(e1 / 3u);
            if (t == u) continue;
            const int p = Forward(tri, e0) == Forward(tri, e1) ? 1 : 0;
            DbscanUnite(parent, 2 * t, 2 * u + p);
            DbscanUnite(parent, 2 * t + 1, 2 * u + 1 - p);
        }
    }
}

__global__ void OrientFlattenKernel(int* __restrict__ parent, int64_t m,
                                    int32_t* __restrict__ flip,
                                    int* __restrict__ bad) {
    O3DMI_GRID_STRIDE(t, m) {
        const int r0 = DbscanFind(parent, (int)(2 * t));
        const int r1 = DbscanFind(parent, (int)(2 * t + 1));
        if (r0 == r1) atomicOr(bad, 1);
        flip[t] = r0 & 1;
    }
}

template <typename I>
__global__ void WriteOrientedKernel(const int32_t* __restrict__ tri, int64_t m,
                                    const int32_t* __restrict__ flip,
                                    const int* __restrict__ bad,
                                    I* __restrict__ out) {
    const bool keep = *bad != 0;
    O3DMI_GRID_STRIDE(t, m) {
        const bool f = !keep && flip[t] != 0;
        const int32_t b = tri[3 * t + 1], c = tri[3 * t + 2];
        out[3 * t] = (I)tri[3 * t];
        out[3 * t + 1] = (I)(f ? c : b);
        out[3 * t + 2] = (I)(f ? b : c);
    }
}

// ---- the per-pair function ------------------------------------------------------------
struct Tri64 {
    double p[3][3];  // vertex, axis
};

__device__ __forceinline__ Tri64 LoadTri64(const void* __restrict__ pos,
                                           int dtype,
                                           const int32_t idx[3]) {
    Tri64 t;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) t.p[a][k] = Coord(pos, dtype, idx[a], k);
    return t;
}

__device__ __forceinline__ void Box64(const Tri64& t, double lo[3],
                                      double hi[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fmin(t.p[0][k], fmin(t.p[1][k], t.p[2][k]));
        hi[k] = fmax(t.p[0][k], fmax(t.p[1][k], t.p[2][k]));
    }
}

template <typename T>
__device__ __forceinline__ bool BoxesOverlap(const T lo0[3], const T hi0[3],
                                             const T lo1[3], const T hi1[3]) {
    if (hi0[0] < lo1[0] || lo0[0] > hi1[0]) return false;
    if (hi0[1] < lo1[1] || lo0[1] > hi1[1]) return false;
    if (hi0[2] < lo1[2] || lo0[2] > hi1[2]) return false;
    return true;
}

__device__ __forceinline__ double Dot64(const double x[3], const double y[3]) {
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

__device__ __forceinline__ void Cross64(const double x[3], const double y[3],
                                        double out[3]) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

// Component k of p by selects: a runtime subscript would send p to scratch.
__device__ __forceinline__ double Pick(const double p[3], int k) {
    return k == 0 ? p[0] : (k == 1 ? p[1] : p[2]);
}

struct P2 {
    double x, y;
};

// Whether segment (v0, v0 + a) meets segment (u0, u1) in the plane
// (Antonio's test, as the coplanar branch uses it).
__device__ __forceinline__ bool EdgeEdge2(const P2& v0, double ax, double ay,
                                          const P2& u0, const P2& u1) {
    const double bx = u0.x - u1.x;
    const double by = u0.y - u1.y;
    const double cx = v0.x - u0.x;
    const double cy = v0.y - u0.y;
    const double f = ay * bx - ax * by;
    const double d = by * cx - bx * cy;
    if ((f > 0 && d >= 0 && d <= f) || (f < 0 && d <= 0 && d >= f)) {
        const double e = ax * cy - ay * cx;
        if (f > 0) {
            if (e >= 0 && e <= f) return true;
        } else {
            if (e <= 0 && e >= f) return true;
        }
    }
    return false;
}

__device__ __forceinline__ bool EdgeTri2(const P2& v0, const P2& v1,
                                         const P2 u[3]) {
    const double ax = v1.x - v0.x;
    const double ay = v1.y - v0.y;
    return EdgeEdge2(v0, ax, ay, u[0], u[1]) ||
           EdgeEdge2(v0, ax, ay, u[1], u[2]) ||
           EdgeEdge2(v0, ax, ay, u[2], u[0]);
}

// The signed line value of p for the edge (u0, u1).
__device__ __forceinline__ double Side2(const P2& p, const P2& u0,
                                        const P2& u1) {
    const double a = u1.y - u0.y;
    const double b = -(u1.x - u0.x);
    const double c = -a * u0.x - b * u0.y;
    return a * p.x + b * p.y + c;
}

__device__ __forceinline__ bool PointInTri2(const P2& p, const P2 u[3]) {
    const double d0 = Side2(p, u[0], u[1]);
    const double d1 = Side2(p, u[1], u[2]);
    const double d2 = Side2(p, u[2], u[0]);
    return d0 * d1 > 0.0 && d0 * d2 > 0.0;
}

__device__ __forceinline__ bool CoplanarHit(const double n[3], const Tri64& v,
                                            const Tri64& u) {
    const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
    int i0, i1;
    if (a0 > a1) {
        if (a0 > a2) {
            i0 = 1;
            i1 = 2;
        } else {
            i0 = 0;
            i1 = 1;
        }
    } else {
        if (a2 > a1) {
            i0 = 0;
            i1 = 1;
        } else {
            i0 = 0;
            i1 = 2;
        }
    }
    P2 pv[3], pu[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pv[k].x = Pick(v.p[k], i0);
        pv[k].y = Pick(v.p[k], i1);
        pu[k].x = Pick(u.p[k], i0);
        pu[k].y = Pick(u.p[k], i1);
    }
    if (EdgeTri2(pv[0], pv[1], pu)) return true;
    if (EdgeTri2(pv[1], pv[2], pu)) return true;
    if (EdgeTri2(pv[2], pv[0], pu)) return true;
    if (PointInTri2(pv[0], pu)) return true;
    if (PointInTri2(pu[0], pv)) return true;
    return false;
}

// The interval of a triangle on the intersection line, without divisions:
// false when the three distances are all zero (coplanar).
__device__ __forceinline__ bool Interval(double vv0, double vv1, double vv2,
                                         double d0, double d1, double d2,
                                         double d0d1, double d0d2, double* a,
                                         double* b, double* c, double* x0,
                                         double* x1) {
    if (d0d1 > 0.0) {
        *a = vv2; *b = (vv0 - vv2) * d2; *c = (vv1 - vv2) * d2;
        *x0 = d2 - d0; *x1 = d2 - d1;
    } else if (d0d2 > 0.0) {
        *a = vv1; *b = (vv0 - vv1) * d1; *c = (vv2 - vv1) * d1;
        *x0 = d1 - d0; *x1 = d1 - d2;
    } else if (d1 * d2 > 0.0 || d0 != 0.0) {
        *a = vv0; *b = (vv1 - vv0) * d0; *c = (vv2 - vv0) * d0;
        *x0 = d0 - d1; *x1 = d0 - d2;
    } else if (d1 != 0.0) {
        *a = vv1; *b = (vv0 - vv1) * d1; *c = (vv2 - vv1) * d1;
        *x0 = d1 - d0; *x1 = d1 - d2;
    } else if (d2 != 0.0) {
        *a = vv2; *b = (vv0 - vv2) * d2; *c = (vv1 - vv2) * d2;
        *x0 = d2 - d0; *x1 = d2 - d1;
    } else {
        return false;
    }
    return true;
}

constexpr double kPlaneSnap = 0.000001;

// Moeller's test on two triangles as they are.
__device__ __forceinline__ bool MoellerHit(const Tri64& v, const Tri64& u) {
    double e1[3], e2[3], n1[3], n2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = v.p[1][k] - v.p[0][k];
        e2[k] = v.p[2][k] - v.p[0][k];
    }
    Cross64(e1, e2, n1);
    const double d1 = -Dot64(n1, v.p[0]);
    double du0 = Dot64(n1, u.p[0]) + d1;
    double du1 = Dot64(n1, u.p[1]) + d1;
    double du2 = Dot64(n1, u.p[2]) + d1;
    if (fabs(du0) < kPlaneSnap) du0 = 0.0;
    if (fabs(du1) < kPlaneSnap) du1 = 0.0;
    if (fabs(du2) < kPlaneSnap) du2 = 0.0;
    const double du0du1 = du0 * du1;
    const double du0du2 = du0 * du2;
    if (du0du1 > 0.0 && du0du2 > 0.0) return false;

#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = u.p[1][k] - u.p[0][k];
        e2[k] = u.p[2][k] - u.p[0][k];
    }
    Cross64(e1, e2, n2);
    const double d2 = -Dot64(n2, u.p[0]);
    double dv0 = Dot64(n2, v.p[0]) + d2;
    double dv1 = Dot64(n2, v.p[1]) + d2;
    double dv2 = Dot64(n2, v.p[2]) + d2;
    if (fabs(dv0) < kPlaneSnap) dv0 = 0.0;
    if (fabs(dv1) < kPlaneSnap) dv1 = 0.0;
    if (fabs(dv2) < kPlaneSnap) dv2 = 0.0;
    const double dv0dv1 = dv0 * dv1;
    const double dv0dv2 = dv0 * dv2;
    if (dv0dv1 > 0.0 && dv0dv2 > 0.0) return false;

    double dir[3];
    Cross64(n1, n2, dir);
    double mx = fabs(dir[0]);
    int index = 0;
    const double bb = fabs(dir[1]), cc = fabs(dir[2]);
    if (bb > mx) {
        mx = bb;
        index = 1;
    }
    if (cc > mx) {
        mx = cc;
        index = 2;
    }
    const double vp0 = Pick(v.p[0], index), vp1 = Pick(v.p[1], index),
                 vp2 = Pick(v.p[2], index);
    const double up0 = Pick(u.p[0], index), up1 = Pick(u.p[1], index),
                 up2 = Pick(u.p[2], index);

    double a, b, c, x0, x1, d, e, f, y0, y1;
    if (!Interval(vp0, vp1, vp2, dv0, dv1, dv2, dv0dv1, dv0dv2, &a, &b, &c,
                  &x0, &x1))
        return CoplanarHit(n1, v, u);
    if (!Interval(up0, up1, up2, du0, du1, du2, du0du1, du0du2, &d, &e, &f,
                  &y0, &y1))
        return CoplanarHit(n1, v, u);

    const double xx = x0 * x1;
    const double yy = y0 * y1;
    const double xxyy = xx * yy;
    double tmp = a * xxyy;
    double s0 = tmp + b * x1 * yy;
    double s1 = tmp + c * x0 * yy;
    tmp = d * xxyy;
    double t0 = tmp + e * xx * y1;
    double t1 = tmp + f * xx * y0;
    if (s0 > s1) {
        const double w = s0;
        s0 = s1;
        s1 = w;
    }
    if (t0 > t1) {
        const double w = t0;
        t0 = t1;
        t1 = w;
    }
    return !(s1 < t0 || t1 < s0);
}

// hit(P, Q) of the header: the normalisation, then MoellerHit.
__device__ __forceinline__ bool TriTriHit(const Tri64& p, const Tri64& q) {
    Tri64 pn, qn;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mu = (((((p.p[0][k] + p.p[1][k]) + p.p[2][k]) +
                             q.p[0][k]) + q.p[1][k]) + q.p[2][k]) / 6;
        const double a0 = p.p[0][k] - mu, a1 = p.p[1][k] - mu,
                     a2 = p.p[2][k] - mu;
        const double b0 = q.p[0][k] - mu, b1 = q.p[1][k] - mu,
                     b2 = q.p[2][k] - mu;
        const double sigma =
                sqrt((((((a0 * a0 + a1 * a1) + a2 * a2) + b0 * b0) + b1 * b1) +
                      b2 * b2) / 5) + 1e-12;
        pn.p[0][k] = a0 / sigma;
        pn.p[1][k] = a1 / sigma;
        pn.p[2][k] = a2 / sigma;
        qn.p[0][k] = b0 / sigma;
        qn.p[1][k] = b1 / sigma;
        qn.p[2][k] = b2 / sigma;
    }
    return MoellerHit(pn, qn);
}

// ---- the traversal ------------------------------------------------------------------------
constexpr int kIsectBlock = 128;

__global__ void CheckReferencedFiniteKernel(const void* __restrict__ pos,
                                            int dtype,
                                            const int32_t* __restrict__ tri,
                                            int64_t n3, int* __restrict__ bad) {
    O3DMI_GRID_STRIDE(e, n3) {
        const int64_t u = tri[e];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = Coord(pos, dtype, u, k);
            const float f = (float)x;
            ok = ok && x - x == 0.0 && f - f == 0.0f;
        }
        if (!ok) atomicOr(bad, 1);
    }
}

// One lane per query triangle; a node is opened iff its float box overlaps the
// query's float box, both children that do are visited (one of them from this
// lane's stack, entry e at stack[e * kIsectBlock], as mesh_bvh.hip's queries
// keep theirs: one push per level).
__global__ void __launch_bounds__(kIsectBlock)
IntersectKernel(int kind, IntersectQuery query, IntersectTarget target,
                uint32_t* __restrict__ is_out, uint32_t* __restrict__ js_out,
                int64_t capacity, unsigned long long* __restrict__ count,
                int* __restrict__ status,
                unsigned long long* __restrict__ visits) {
    __shared__ int32_t stack_all[kBvhStack * kIsectBlock];
    int32_t* stack = stack_all + threadIdx.x;
    const MeshBvhView& bvh = target.bvh;
    unsigned long long opened = 0, tested = 0;
    bool overflow = false;
    O3DMI_GRID_STRIDE(slot, query.m) {
        if (kind == kIntersectAny &&
            __hip_atomic_load(count, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) != 0)
            break;  // somebody found a pair: the answer is known
        const uint32_t i =
                query.self ? bvh.leaves[slot].id : (uint32_t)slot;
        int32_t pi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pi[a] = query.tri[3 * (int64_t)i + a];
        const Tri64 p = LoadTri64(query.positions, query.dtype, pi);
        double plo[3], phi[3];
        Box64(p, plo, phi);
        float flo[3], fhi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            flo[k] = (float)plo[k];
            fhi[k] = (float)phi[k];
        }
        int sp = 0;
        int32_t node = bvh.m == 1 ? ~0 : 0;
        bool found = false;
        for (;;) {
            bool pop = true;
            if (node < 0) {
                const uint32_t j = bvh.leaves[~node].id;
                if (!query.self || j > i) {
                    int32_t qi[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        qi[a] = target.tri[3 * (int64_t)j + a];
                    const bool shared =
                            query.self &&
                            (pi[0] == qi[0] || pi[0] == qi[1] ||
                             pi[0] == qi[2] || pi[1] == qi[0] ||
                             pi[1] == qi[1] || pi[1] == qi[2] ||
                             pi[2] == qi[0] || pi[2] == qi[1] ||
                             pi[2] == qi[2]);
                    if (!shared) {
                        const Tri64 q =
                                LoadTri64(target.positions, target.dtype, qi);
                        double qlo[3], qhi[3];
                        Box64(q, qlo, qhi);
                        if (BoxesOverlap(plo, phi, qlo, qhi)) {
                            ++tested;
                            if (TriTriHit(p, q)) {
                                if (kind == kIntersectAny) {
                                    __hip_atomic_store(
                                            count, 1ull, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
                                    found = true;
                                    break;
                                }
                                const unsigned long long at =
                                        atomicAdd(count, 1ull);
                                if ((int64_t)at < capacity) {
                                    is_out[at] = i;
                                    js_out[at] = j;
                                }
                            }
                        }
                    }
                }
            } else {
                const float4* w = (const float4*)(bvh.nodes + node);
                const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                const int32_t c0 = (int32_t)__float_as_uint(w0.x);
                const int32_t c1 = (int32_t)__float_as_uint(w0.y);
                const float lo0[3] = {w1.x, w1.y, w1.z};
                const float hi0[3] = {w1.w, w2.x, w2.y};
                const float lo1[3] = {w2.z, w2.w, w3.x};
                const float hi1[3] = {w3.y, w3.z, w3.w};
                const bool go0 = BoxesOverlap(flo, fhi, lo0, hi0);
                const bool go1 = BoxesOverlap(flo, fhi, lo1, hi1);
                ++opened;
                if (go0 && go1) {
                    if (sp < kBvhStack) {
                        stack[sp * kIsectBlock] = c1;
                        ++sp;
                    } else {
                        overflow = true;  // never, by the bound in mesh_bvh.h
                    }
                    node = c0;
                    pop = false;
                } else if (go0 || go1) {
                    node = go0 ? c0 : c1;
                    pop = false;
                }
            }
            if (pop) {
                if (sp == 0) break;
                --sp;
                node = stack[sp * kIsectBlock];
            }
        }
        if (found) break;
    }
    if (overflow) atomicOr(status, 1);
    if (visits) {
        for (int w = 32; w > 0; w >>= 1) {
            opened += __shfl_xor(opened, w);
            tested += __shfl_xor(tested, w);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&visits[0], opened);
            atomicAdd(&visits[1], tested);
        }
    }
}

template <typename I>
__global__ void WritePairsKernel(const uint32_t* __restrict__ is,
                                 const uint32_t* __restrict__ js, int64_t n,
                                 I* __restrict__ out) {
    O3DMI_GRID_STRIDE(k, n) {
        out[2 * k] = (I)is[k];
        out[2 * k + 1] = (I)js[k];
    }
}

// ---- volume --------------------------------------------------------------------------------
__global__ void TetraVolumesKernel(const void* __restrict__ pos, int dtype,
                                   const int32_t* __restrict__ tri, int64_t m,
                                   double* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        const Tri64 p = LoadTri64(pos, dtype, idx);
        double c[3];
        Cross64(p.p[1], p.p[2], c);
        out[t] = Dot64(p.p[0], c) / 6.0;
    }
}

}  // namespace

int CountFlagsAsync(const int32_t* flags_dev, int64_t n,
                    unsigned long long* count_dev, hipStream_t s) {
    O3DMI_REQUIRE(flags_dev && n > 0 && count_dev, "null argument");
    O3DMI_LAUNCH(CountFlagsKernel, n, flags_dev, n, count_dev);
    return O3DMI_OK;
}

int NonManifoldVertexFlagsAsync(const int32_t* tri, int64_t m, int64_t v,
                                const EdgeTable& edges,
                                const CornerTable& corners, int* parent_dev,
                                int32_t* long_list_dev, int32_t* flags_dev,
                                hipStream_t s) {
    O3DMI_REQUIRE(tri && m > 0 && v > 0 && parent_dev && long_list_dev &&
                          flags_dev,
                  "null argument");
    const int64_t n3 = 3 * m;
    const int st = IotaAsync(parent_dev, n3, s);
    if (st) return st;
    O3DMI_LAUNCH(WedgeUnionKernel, n3, edges, tri, n3, parent_dev);
    // the sorted corner keys are done with: they carry the wedge roots
    int* rootw = (int*)corners.vertex;
    O3DMI_LAUNCH(WedgeRootKernel, n3, tri, n3, parent_dev, rootw);
    O3DMI_LAUNCH(VertexFlagsThreadKernel, v, corners, v, rootw, long_list_dev,
                 flags_dev);
    hipLaunchKernelGGL(VertexFlagsWaveKernel, WaveGrid(v), dim3(kBlock), 0, s,
                       corners, v, rootw, long_list_dev, flags_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int EmitFlaggedAsync(const int32_t* flags_dev, const int64_t* pos_dev,
                     int64_t n, int index_dtype, void* out_dev,
                     hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(EmitFlaggedKernel<int64_t>, n, flags_dev, pos_dev, n,
                     (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(EmitFlaggedKernel<int32_t>, n, flags_dev, pos_dev, n,
                     (int32_t*)out_dev);
    return O3DMI_OK;
}

int OrientFlipsAsync(const int32_t* tri, int64_t m, const EdgeTable& edges,
                     int* parent_dev, int32_t* flip_dev, int* bad_dev,
                     hipStream_t s) {
    O3DMI_REQUIRE(tri && m > 0 && parent_dev && flip_dev && bad_dev,
                  "null argument");
    const int st = IotaAsync(parent_dev, 2 * m, s);
    if (st) return st;
    O3DMI_LAUNCH(OrientUnionKernel, 3 * m, edges, tri, 3 * m, parent_dev,
                 bad_dev);
    O3DMI_LAUNCH(OrientFlattenKernel, m, parent_dev, m, flip_dev, bad_dev);
    return O3DMI_OK;
}

int WriteOrientedAsync(const int32_t* tri, int64_t m, const int32_t* flip_dev,
                       const int* bad_dev, int index_dtype, void* out_dev,
                       hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(WriteOrientedKernel<int64_t>, m, tri, m, flip_dev,
                     bad_dev, (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(WriteOrientedKernel<int32_t>, m, tri, m, flip_dev,
                     bad_dev, (int32_t*)out_dev);
    return O3DMI_OK;
}

int CheckReferencedFiniteAsync(const void* positions_dev, int dtype,
                               const int32_t* tri, int64_t m, int* bad_dev,
                               hipStream_t s) {
    O3DMI_REQUIRE(positions_dev && tri && m > 0 && bad_dev, "null argument");
    O3DMI_LAUNCH(CheckReferencedFiniteKernel, 3 * m, positions_dev, dtype, tri,
                 3 * m, bad_dev);
    return O3DMI_OK;
}

int MeshIntersectAsync(IntersectKind kind, const IntersectQuery& query,
                       const IntersectTarget& target, uint32_t* is_out_dev,
                       uint32_t* js_out_dev, int64_t capacity,
                       unsigned long long* count_dev, int* status_dev,
                       unsigned long long* visits_dev, hipStream_t s) {
    const MeshBvhView& bvh = target.bvh;
    O3DMI_REQUIRE(bvh.leaves && bvh.m > 0 && (bvh.m == 1 || bvh.nodes) &&
                          query.positions && query.tri && query.m > 0 &&
                          target.positions && target.tri && count_dev &&
                          status_dev,
                  "null argument");
    O3DMI_REQUIRE(!query.self || query.m == bvh.m, "self query: m differs");
    O3DMI_REQUIRE(capacity <= 0 || (is_out_dev && js_out_dev),
                  "null argument");
    hipLaunchKernelGGL(IntersectKernel,
                       dim3((unsigned)GridFor(query.m, kIsectBlock,
                                              kCUs * 16)),
                       dim3(kIsectBlock), 0, s, (int)kind, query, target,
                       is_out_dev, js_out_dev, capacity, count_dev, status_dev,
                       visits_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int WritePairsAsync(const uint32_t* is_dev, const uint32_t* js_dev, int64_t n,
                    int index_dtype, void* out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(WritePairsKernel<int64_t>, n, is_dev, js_dev, n,
                     (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(WritePairsKernel<int32_t>, n, is_dev, js_dev, n,
                     (int32_t*)out_dev);
    return O3DMI_OK;
}

int TetraVolumesAsync(const void* positions_dev, int dtype, const int32_t* tri,
                      int64_t m, double* out_dev, hipStream_t s) {
    O3DMI_REQUIRE(positions_dev && tri && m > 0 && out_dev, "null argument");
    O3DMI_LAUNCH(TetraVolumesKernel, m, positions_dev, dtype, tri, m, out_dev);
    return O3DMI_OK;
}

}  // namespace o3dmi
