// Kernels of the oriented bounding boxes and the bounding ellipsoid
// (OrientedBoundingBox::CreateFromPoints with MINIMAL_APPROX or PCA,
// OrientedBoundingEllipsoid::CreateFromPoints; docs/bounding_volumes.md) on the
// convex hull's V vertices X (float64) and T triangles. The library is compiled
// with -ffp-contract=off: every expression below is evaluated as written.
// Atomics are integer only. Minima, maxima and arg-maxima are exact whatever
// the order; every SUM goes through the fixed tree of bounding_volume.h.
#include <climits>

#include "bounding_volume.h"

namespace o3dmi {
namespace {

struct Vec3 {
    double x, y, z;
};

__device__ __forceinline__ Vec3 VertexOf(const double* X, int64_t i) {
    const double* r = X + 3 * i;
    return {r[0], r[1], r[2]};
}

// Bits whose unsigned order is the order of the finite doubles
// (pointcloud_hull.hip's), and back.
__device__ __forceinline__ unsigned long long OrderedKey(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double KeyValue(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double Dot3(const Vec3& d, const Vec3& r) {
    return (d.x * r.x + d.y * r.y) + d.z * r.z;
}

__device__ __forceinline__ Vec3 Normalized(const Vec3& v) {
    const double n = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    return {v.x / n, v.y / n, v.z / n};
}

__device__ __forceinline__ Vec3 Cross(const Vec3& a, const Vec3& b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z,
            a.x * b.y - a.y * b.x};
}

// ---- (a) MINIMAL_APPROX ----------------------------------------------------------
// The frame of a candidate: origin a and the unit axes u, v, w
// (MinimumOBB.cpp:1287-1296). Candidate -1: the origin and the identity.
struct Frame {
    Vec3 a, u, v, w;
};

__device__ __forceinline__ Frame FrameOf(const double* X, const int32_t* tri,
                                         int64_t cand) {
    Frame f;
    if (cand < 0) {
        f.a = {0.0, 0.0, 0.0};
        f.u = {1.0, 0.0, 0.0};
        f.v = {0.0, 1.0, 0.0};
        f.w = {0.0, 0.0, 1.0};
        return f;
    }
    const int32_t* t = tri + 3 * cand;
    f.a = VertexOf(X, t[0]);
    const Vec3 b = VertexOf(X, t[1]), c = VertexOf(X, t[2]);
    Vec3 u = {b.x - f.a.x, b.y - f.a.y, b.z - f.a.z};
    Vec3 v = {c.x - f.a.x, c.y - f.a.y, c.z - f.a.z};
    const Vec3 w = Cross(u, v);
    v = Cross(w, u);
    f.u = Normalized(u);
    f.v = Normalized(v);
    f.w = Normalized(w);
    return f;
}

// lohi[(slice * n_cand + item) * 6 ..] = the minima and maxima of item's frame
// over the vertices of slice blockIdx.y; item = candidate + 1. Lane = one
// candidate; the vertices come wave-uniformly from an LDS tile.
__global__ void __launch_bounds__(kObbBlock)
ObbBoxKernel(const double* __restrict__ X, int n_verts,
             const int32_t* __restrict__ tri, int n_cand, int per_slice,
             double* __restrict__ lohi) {
    __shared__ double tile[3 * kObbTile];
    const int item = blockIdx.x * kObbBlock + threadIdx.x;
    const bool live = item < n_cand;
    const Frame f = FrameOf(X, tri, live ? (int64_t)item - 1 : -1);
    const int begin = blockIdx.y * per_slice;
    const int end = begin + per_slice < n_verts ? begin + per_slice : n_verts;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int base = begin; base < end; base += kObbTile) {
        const int cnt = end - base < kObbTile ? end - base : kObbTile;
        __syncthreads();
        for (int k = threadIdx.x; k < 3 * cnt; k += kObbBlock)
            tile[k] = X[3 * (int64_t)base + k];
        __syncthreads();
        if (!live) continue;
        for (int k = 0; k < cnt; ++k) {
            const Vec3 d = {tile[3 * k] - f.a.x, tile[3 * k + 1] - f.a.y,
                            tile[3 * k + 2] - f.a.z};
            const double c[3] = {Dot3(d, f.u), Dot3(d, f.v), Dot3(d, f.w)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = c[a] < lo[a] ? c[a] : lo[a];
                hi[a] = c[a] > hi[a] ? c[a] : hi[a];
            }
        }
    }
    if (!live) return;
    double* out = lohi + ((int64_t)blockIdx.y * n_cand + item) * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = lo[a];
        out[3 + a] = hi[a];
    }
}

// The slices of a candidate joined (into slice 0), its volume (NaN when a
// coordinate of the frame is NaN: no minimum was ever taken) and the smallest
// volume's ordered bits in words[0].
__global__ void __launch_bounds__(kObbBlock)
ObbVolumeKernel(int n_cand, int split, double* __restrict__ lohi,
                double* __restrict__ vol, unsigned long long* words) {
    const int item = blockIdx.x * kObbBlock + threadIdx.x;
    if (item >= n_cand) return;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = lohi[(int64_t)item * 6 + a];
        hi[a] = lohi[(int64_t)item * 6 + 3 + a];
    }
    for (int sl = 1; sl < split; ++sl) {
        const double* in = lohi + ((int64_t)sl * n_cand + item) * 6;
        for (int a = 0; a < 3; ++a) {
            lo[a] = in[a] < lo[a] ? in[a] : lo[a];
            hi[a] = in[3 + a] > hi[a] ? in[3 + a] : hi[a];
        }
    }
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
        lohi[(int64_t)item * 6 + a] = lo[a];
        lohi[(int64_t)item * 6 + 3 + a] = hi[a];
        ok = ok && lo[a] <= hi[a];
    }
    const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
    const double v = ok ? (e0 * e1) * e2 : __longlong_as_double(0x7FF8000000000000ll);
    vol[item] = v;
    if (v == v) atomicMin(&words[0], OrderedKey(v));
}

// Ties go to the lowest candidate index.
__global__ void __launch_bounds__(kObbBlock)
ObbPickKernel(int n_cand, const double* __restrict__ vol,
              unsigned long long* words) {
    const int item = blockIdx.x * kObbBlock + threadIdx.x;
    if (item >= n_cand) return;
    const double v = vol[item];
    if (v == v && OrderedKey(v) == words[0])
        atomicMin(&words[1], (unsigned long long)item);
}

// The winner's box (MinimumOBB.cpp:1307-1312).
__global__ void ObbFinalKernel(const double* __restrict__ X,
                               const int32_t* __restrict__ tri, int n_cand,
                               const double* __restrict__ lohi,
                               const double* __restrict__ vol,
                               const unsigned long long* words,
                               ObbResult* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long item = words[1];
    if (item >= (unsigned long long)n_cand) {
        out->winner = -2.0;
        return;
    }
    const Frame f = FrameOf(X, tri, (int64_t)item - 1);
    const double* b = lohi + (int64_t)item * 6;
    double m[3];
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = b[a];
        out->hi[a] = b[3 + a];
        out->extent[a] = b[3 + a] - b[a];
        m[a] = (b[a] + b[3 + a]) / 2.0;
    }
    const double R[9] = {f.u.x, f.v.x, f.w.x, f.u.y, f.v.y,
                         f.w.y, f.u.z, f.v.z, f.w.z};
    const double a3[3] = {f.a.x, f.a.y, f.a.z};
    for (int r = 0; r < 3; ++r)
        out->center[r] = a3[r] + ((R[3 * r] * m[0] + R[3 * r + 1] * m[1]) +
                                  R[3 * r + 2] * m[2]);
    for (int k = 0; k < 9; ++k) out->rotation[k] = R[k];
    out->volume = vol[item];
    out->winner = (double)((long long)item - 1);
}

// ---- the tree ---------------------------------------------------------------------
// s[v][0 .. count) -> s[v][0] by the fixed tree, for v < NV; count <= kBvBlock.
// Every lane of the workgroup calls it; the result is visible to all on return.
template <int NV>
__device__ __forceinline__ void BlockTree(double (*s)[kBvBlock], int count) {
    while (count > 1) {
        const int next = (count + kBvRun - 1) / kBvRun;
        double acc[NV];
        if ((int)threadIdx.x < next) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                acc[v] = 0.0;
                for (int k = 0; k < kBvRun; ++k) {
                    const int i = kBvRun * threadIdx.x + k;
                    acc[v] += i < count ? s[v][i] : 0.0;
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < next) {
#pragma unroll
            for (int v = 0; v < NV; ++v) s[v][threadIdx.x] = acc[v];
        }
        __syncthreads();
        count = next;
    }
}

__device__ __forceinline__ void StoreBits(unsigned long long* at, double v) {
    __hip_atomic_store(at, (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double LoadBits(const unsigned long long* at) {
    return __longlong_as_double((long long)__hip_atomic_load(
            at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The rows a[0 .. count)[NV] of the workgroups -> one row, by the same tree,
// through the two buffers; run by the last workgroup to arrive. Returns the
// buffer whose row 0 holds the result, visible to every lane.
template <int NV>
__device__ __forceinline__ unsigned long long* GlobalTree(
        unsigned long long* a, unsigned long long* b, int count) {
    while (count > 1) {
        const int next = (count + kBvRun - 1) / kBvRun;
        for (int t = threadIdx.x; t < next * NV; t += kBvBlock) {
            const int row = t / NV, v = t % NV;
            double acc = 0.0;
            for (int k = 0; k < kBvRun; ++k) {
                const int i = kBvRun * row + k;
                if (i < count) acc += LoadBits(&a[(int64_t)i * NV + v]);
            }
            StoreBits(&b[(int64_t)row * NV + v], acc);
        }
        __threadfence();
        __syncthreads();
        unsigned long long* t = a;
        a = b;
        b = t;
        count = next;
    }
    return a;
}

// One arrival per workgroup after its partial row is stored; true in every
// lane of the last workgroup to arrive (the hand-over of the streamed
// farthest-point sampler: write-through stores, a fence, one atomic add).
__device__ __forceinline__ bool ArriveLast(unsigned* ticket) {
    __shared__ int s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned drawn = __hip_atomic_fetch_add(
                ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = drawn == gridDim.x - 1;
    }
    __syncthreads();
    const bool last = s_last != 0;
    if (last) __threadfence();
    return last;
}

// The run of kBvRun vertices of a lane: zeros past the end (they add 0.0).
struct Run {
    double x[kBvRun][3];
    bool valid[kBvRun];
};

__device__ __forceinline__ void LoadRun(const double* __restrict__ X,
                                        int64_t first, int64_t n_verts,
                                        Run& r) {
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) {
        const int64_t i = first + k;
        r.valid[k] = i < n_verts;
#pragma unroll
        for (int a = 0; a < 3; ++a) r.x[k][a] = r.valid[k] ? X[3 * i + a] : 0.0;
    }
}

// acc[0..9) += {x, y, z, xx, xy, xz, yy, yz, zz} of the run scaled by p (terms
// (p x) y), acc[9] += p, in index order.
__device__ __forceinline__ void WeightedRunSums(const Run& r,
                                                const double (&p)[kBvRun],
                                                double* acc) {
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) {
        const double px = p[k] * r.x[k][0], py = p[k] * r.x[k][1],
                     pz = p[k] * r.x[k][2];
        acc[0] += px;
        acc[1] += py;
        acc[2] += pz;
        acc[3] += px * r.x[k][0];
        acc[4] += px * r.x[k][1];
        acc[5] += px * r.x[k][2];
        acc[6] += py * r.x[k][1];
        acc[7] += py * r.x[k][2];
        acc[8] += pz * r.x[k][2];
        acc[9] += p[k];
    }
}

// M of a vertex: t_r = ((G[r][0] x + G[r][1] y) + G[r][2] z) + G[r][3], then
// ((x t_0 + y t_1) + z t_2) + t_3.
__device__ __forceinline__ double MOf(const double* G, const double* x) {
    double t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        t[r] = ((G[4 * r] * x[0] + G[4 * r + 1] * x[1]) + G[4 * r + 2] * x[2]) +
               G[4 * r + 3];
    return ((x[0] * t[0] + x[1] * t[1]) + x[2] * t[2]) + t[3];
}

__device__ __forceinline__ bool Better(double v, int i, double bv, int bi) {
    return v > bv || (v == bv && i < bi);
}

// The run's largest M, ties to the lowest index (ascending order, strict >).
__device__ __forceinline__ void RunArgmax(const Run& r, const double* G,
                                          int first, double& bv, int& bi) {
    bv = -__longlong_as_double(0x7FF0000000000000ll);
    bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) {
        if (!r.valid[k]) continue;
        const double m = MOf(G, r.x[k]);
        if (m > bv) {
            bv = m;
            bi = first + k;
        }
    }
}

// The workgroup's best (value, index) in s_v[0], s_i[0], visible to all.
__device__ __forceinline__ void BlockArgmax(double bv, int bi, double* s_v,
                                            int* s_i) {
    s_v[threadIdx.x] = bv;
    s_i[threadIdx.x] = bi;
    __syncthreads();
    for (int o = kBvBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o &&
            Better(s_v[threadIdx.x + o], s_i[threadIdx.x + o],
                   s_v[threadIdx.x], s_i[threadIdx.x])) {
            s_v[threadIdx.x] = s_v[threadIdx.x + o];
            s_i[threadIdx.x] = s_i[threadIdx.x + o];
        }
        __syncthreads();
    }
}

// p <- (1 - step) p, p_j += step over the run; returns the run's sum of the
// squared differences, in index order (MinimumOBE.cpp:158-162).
__device__ __forceinline__ double UpdateRun(double (&p)[kBvRun], int first,
                                            double step, int j) {
    double dsq = 0.0;
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) {
        double np = (1.0 - step) * p[k];
        if (first + k == j) np += step;
        const double d = np - p[k];
        dsq += d * d;
        p[k] = np;
    }
    return dsq;
}

__device__ __forceinline__ double StepOf(double max_m) {
    return (max_m - 4.0) / (4.0 * (max_m - 1.0));
}

// ---- (b) the nine sums ------------------------------------------------------------
__global__ void __launch_bounds__(kBvBlock)
MomentsKernel(const double* __restrict__ X, int64_t n_verts,
              unsigned long long* part_a, unsigned long long* part_b,
              unsigned* ticket, double* __restrict__ sums_out) {
    __shared__ double s[9][kBvBlock];
    Run r;
    LoadRun(X, ((int64_t)blockIdx.x * kBvBlock + threadIdx.x) * kBvRun,
            n_verts, r);
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) {
        const double x = r.x[k][0], y = r.x[k][1], z = r.x[k][2];
        acc[0] += x;
        acc[1] += y;
        acc[2] += z;
        acc[3] += x * x;
        acc[4] += x * y;
        acc[5] += x * z;
        acc[6] += y * y;
        acc[7] += y * z;
        acc[8] += z * z;
    }
#pragma unroll
    for (int v = 0; v < 9; ++v) s[v][threadIdx.x] = acc[v];
    __syncthreads();
    BlockTree<9>(s, kBvBlock);
    if (threadIdx.x < 9)
        StoreBits(&part_a[(int64_t)blockIdx.x * 9 + threadIdx.x],
                  s[threadIdx.x][0]);
    if (!ArriveLast(ticket)) return;
    const unsigned long long* total =
            GlobalTree<9>(part_a, part_b, (int)gridDim.x);
    if (threadIdx.x < 9) sums_out[threadIdx.x] = LoadBits(&total[threadIdx.x]);
    if (threadIdx.x == 0)
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

struct FrameArg {
    double mean[3];
    double r[9];  // row-major
};

__global__ void ExtentsInitKernel(unsigned long long* keys) {
    if (blockIdx.x != 0 || threadIdx.x >= 6) return;
    keys[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(kBlock)
ExtentsKernel(const double* __restrict__ X, int64_t n_verts, FrameArg f,
              unsigned long long* keys) {
    __shared__ unsigned long long s[6][kBlock];
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n_verts;
         i += (int64_t)gridDim.x * kBlock) {
        const Vec3 x = VertexOf(X, i);
        const Vec3 d = {x.x - f.mean[0], x.y - f.mean[1], x.z - f.mean[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const Vec3 col = {f.r[a], f.r[3 + a], f.r[6 + a]};
            const unsigned long long k = OrderedKey(Dot3(d, col));
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = lo[a];
        s[3 + a][threadIdx.x] = hi[a];
    }
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned long long l = s[a][threadIdx.x + o];
                const unsigned long long h = s[3 + a][threadIdx.x + o];
                if (l < s[a][threadIdx.x]) s[a][threadIdx.x] = l;
                if (h > s[3 + a][threadIdx.x]) s[3 + a][threadIdx.x] = h;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) atomicMin(&keys[threadIdx.x], s[threadIdx.x][0]);
    else if (threadIdx.x < 6) atomicMax(&keys[threadIdx.x], s[threadIdx.x][0]);
}

// ---- (c) Khachiyan's loop, resident form ------------------------------------------
// One workgroup; lane l holds the run [kBvRun l, kBvRun (l + 1)) of vertices and
// weights in registers, which is level 0 of the tree; the levels above run in
// LDS. Every lane evaluates the 4x4 inverse and the step itself from the same
// LDS values: no broadcast, the same bits.
__global__ void __launch_bounds__(kBvBlock)
ObeResidentKernel(const double* __restrict__ X, int n_verts, ObeWords* w) {
    __shared__ double s[kBvSums][kBvBlock];
    __shared__ double s_v[kBvBlock];
    __shared__ int s_i[kBvBlock];
    const int first = threadIdx.x * kBvRun;
    Run r;
    LoadRun(X, first, n_verts, r);
    double p[kBvRun];
#pragma unroll
    for (int k = 0; k < kBvRun; ++k)
        p[k] = r.valid[k] ? 1.0 / (double)n_verts : 0.0;
    double dsq = 0.0, sums[kBvSums], max_m = 0.0, step = 0.0;
    int it = 0, singular = 0, arg = 0;
    for (;;) {
        double acc[kBvSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        WeightedRunSums(r, p, acc);
        acc[10] = dsq;
#pragma unroll
        for (int v = 0; v < kBvSums; ++v) s[v][threadIdx.x] = acc[v];
        __syncthreads();
        BlockTree<kBvSums>(s, kBvBlock);
#pragma unroll
        for (int v = 0; v < kBvSums; ++v) sums[v] = s[v][0];
        __syncthreads();
        if (it > 0 &&
            (sqrt(sums[10]) <= kObeTolerance || it == kObeMaxIterations))
            break;
        double G[16];
        if (!ObeInverse(sums, G)) {
            singular = 1;
            break;
        }
        double bv;
        int bi;
        RunArgmax(r, G, first, bv, bi);
        BlockArgmax(bv, bi, s_v, s_i);
        max_m = s_v[0];
        arg = s_i[0];
        __syncthreads();
        if (arg == INT_MAX) {  // every M is NaN
            singular = 1;
            break;
        }
        step = StepOf(max_m);
        dsq = UpdateRun(p, first, step, arg);
        ++it;
    }
    if (threadIdx.x == 0) {
        w->iterations = it;
        w->singular = singular;
        w->argmax = arg;
        w->step = step;
        w->max_m = max_m;
        for (int v = 0; v < kBvSums; ++v) w->sums[v] = sums[v];
        w->done = 1;
    }
}

// ---- (c) streamed form -------------------------------------------------------------
// Scratch: weights {G kBvBlockVertices} | rows a {G, 11} | rows b {G, 11} |
// arg-max values {G} | arg-max indices {G}, G = workgroups, all 8-byte words.
struct ObeStream {
    double* p;
    unsigned long long* part_a;
    unsigned long long* part_b;
    unsigned long long* part_v;
    unsigned long long* part_i;
    int grid;
};

int ObeGrid(int64_t n_verts) {
    return (int)((n_verts + kBvBlockVertices - 1) / kBvBlockVertices);
}

ObeStream CarveObe(double* scratch, int64_t n_verts) {
    ObeStream o;
    o.grid = ObeGrid(n_verts);
    const size_t g = (size_t)o.grid;
    o.p = scratch;
    o.part_a = (unsigned long long*)(scratch + g * kBvBlockVertices);
    o.part_b = o.part_a + g * kBvSums;
    o.part_v = o.part_b + g * kBvSums;
    o.part_i = o.part_v + g;
    return o;
}

__global__ void ObeInitKernel(double* __restrict__ p, int64_t n_verts,
                              int64_t padded) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < padded;
         i += (int64_t)gridDim.x * blockDim.x)
        p[i] = i < n_verts ? 1.0 / (double)n_verts : 0.0;
}

// Ends iteration `iteration` (its weight update and stop value) and forms the
// sums of the next Lambda. p is padded to whole workgroups.
__global__ void __launch_bounds__(kBvBlock)
ObeSumsKernel(const double* __restrict__ X, int64_t n_verts, int iteration,
              ObeStream o, ObeWords* w) {
    __shared__ double s[kBvSums][kBvBlock];
    if (w->done) return;
    const int64_t first =
            ((int64_t)blockIdx.x * kBvBlock + threadIdx.x) * kBvRun;
    Run r;
    LoadRun(X, first, n_verts, r);
    double p[kBvRun];
#pragma unroll
    for (int k = 0; k < kBvRun; ++k) p[k] = o.p[first + k];
    double dsq = 0.0;
    if (iteration > 0) {
        dsq = UpdateRun(p, (int)first, w->step, w->argmax);
#pragma unroll
        for (int k = 0; k < kBvRun; ++k) o.p[first + k] = p[k];
    }
    double acc[kBvSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    WeightedRunSums(r, p, acc);
    acc[10] = dsq;
#pragma unroll
    for (int v = 0; v < kBvSums; ++v) s[v][threadIdx.x] = acc[v];
    __syncthreads();
    BlockTree<kBvSums>(s, kBvBlock);
    if (threadIdx.x < kBvSums)
        StoreBits(&o.part_a[(int64_t)blockIdx.x * kBvSums + threadIdx.x],
                  s[threadIdx.x][0]);
    if (!ArriveLast(&w->ticket[0])) return;
    const unsigned long long* total =
            GlobalTree<kBvSums>(o.part_a, o.part_b, (int)gridDim.x);
    if (threadIdx.x != 0) return;
    double sums[kBvSums];
    for (int v = 0; v < kBvSums; ++v) {
        sums[v] = LoadBits(&total[v]);
        w->sums[v] = sums[v];
    }
    w->iterations = iteration;
    if (iteration > 0 && (sqrt(sums[10]) <= kObeTolerance ||
                          iteration == kObeMaxIterations)) {
        w->done = 1;
    } else if (!ObeInverse(sums, w->inv)) {
        w->singular = 1;
        w->done = 1;
    }
    __hip_atomic_store(&w->ticket[0], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kBvBlock)
ObeArgmaxKernel(const double* __restrict__ X, int64_t n_verts, ObeStream o,
                ObeWords* w) {
    __shared__ double s_v[kBvBlock];
    __shared__ int s_i[kBvBlock];
    if (w->done) return;
    double G[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = w->inv[k];
    const int64_t first =
            ((int64_t)blockIdx.x * kBvBlock + threadIdx.x) * kBvRun;
    Run r;
    LoadRun(X, first, n_verts, r);
    double bv;
    int bi;
    RunArgmax(r, G, (int)first, bv, bi);
    BlockArgmax(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) {
        StoreBits(&o.part_v[blockIdx.x], s_v[0]);
        __hip_atomic_store(&o.part_i[blockIdx.x], (unsigned long long)s_i[0],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ArriveLast(&w->ticket[1])) return;
    bv = -__longlong_as_double(0x7FF0000000000000ll);
    bi = INT_MAX;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kBvBlock) {
        const double ov = LoadBits(&o.part_v[b]);
        const int oi = (int)__hip_atomic_load(&o.part_i[b], __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        if (Better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    BlockArgmax(bv, bi, s_v, s_i);
    if (threadIdx.x != 0) return;
    w->max_m = s_v[0];
    w->argmax = s_i[0];
    if (s_i[0] == INT_MAX) {  // every M is NaN
        w->singular = 1;
        w->done = 1;
    } else {
        w->step = StepOf(s_v[0]);
    }
    __hip_atomic_store(&w->ticket[1], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------
size_t ObbApproxScratchDoubles(int64_t n_tris, int split) {
    const size_t cand = (size_t)n_tris + 1;
    return cand * 6 * (size_t)split + cand;
}

int BvExtentsAsync(const double* X_dev, int64_t n_verts, const double mean[3],
                   const double rotation[9], unsigned long long* keys_dev,
                   hipStream_t s) {
    FrameArg f;
    for (int k = 0; k < 3; ++k) f.mean[k] = mean[k];
    for (int k = 0; k < 9; ++k) f.r[k] = rotation[k];
    hipLaunchKernelGGL(ExtentsInitKernel, dim3(1), dim3(64), 0, s, keys_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ExtentsKernel, dim3(GridFor(n_verts, kBlock, kCUs)),
                       dim3(kBlock), 0, s, X_dev, n_verts, f, keys_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ObbApproxAsync(const double* X_dev, int64_t n_verts, const int32_t* tri_dev,
                   int64_t n_tris, int split, double* scratch_dev,
                   unsigned long long* words_dev, ObbResult* result_dev,
                   hipStream_t s) {
    O3DMI_REQUIRE(split >= 1 && split <= kObbMaxSplit, "split out of range");
    O3DMI_REQUIRE(n_verts >= 1 && n_verts < INT_MAX && n_tris < INT_MAX - 1,
                  "hull out of range");
    const int n_cand = (int)n_tris + 1;
    const int per_slice = (int)((n_verts + split - 1) / split);
    double* lohi = scratch_dev;
    double* vol = scratch_dev + (size_t)n_cand * 6 * split;
    O3DMI_HIP_CHECK(hipMemsetAsync(words_dev, 0xFF, 16, s));
    const int blocks = (n_cand + kObbBlock - 1) / kObbBlock;
    hipLaunchKernelGGL(ObbBoxKernel, dim3(blocks, split), dim3(kObbBlock), 0, s,
                       X_dev, (int)n_verts, tri_dev, n_cand, per_slice, lohi);
    O3DMI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ObbVolumeKernel, dim3(blocks), dim3(kObbBlock), 0, s,
                       n_cand, split, lohi, vol, words_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ObbPickKernel, dim3(blocks), dim3(kObbBlock), 0, s,
                       n_cand, vol, words_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ObbFinalKernel, dim3(1), dim3(64), 0, s, X_dev, tri_dev,
                       n_cand, lohi, vol, words_dev, result_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

size_t BvSumScratchDoubles(int64_t n_verts) {
    return 2 * (size_t)ObeGrid(n_verts) * kBvSums;
}

int BvMomentsAsync(const double* X_dev, int64_t n_verts, double* scratch_dev,
                   unsigned* ticket_dev, double* sums_dev, hipStream_t s) {
    const int grid = ObeGrid(n_verts);
    unsigned long long* a = (unsigned long long*)scratch_dev;
    hipLaunchKernelGGL(MomentsKernel, dim3(grid), dim3(kBvBlock), 0, s, X_dev,
                       n_verts, a, a + (size_t)grid * kBvSums, ticket_dev,
                       sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

size_t ObeStreamScratchDoubles(int64_t n_verts) {
    const size_t g = (size_t)ObeGrid(n_verts);
    return g * kBvBlockVertices + 2 * g * kBvSums + 2 * g;
}

int ObeResidentAsync(const double* X_dev, int64_t n_verts, ObeWords* words_dev,
                     hipStream_t s) {
    if (n_verts > kObeResidentCapacity) {
        SetLastError("bounding ellipsoid: the hull is above the resident "
                     "form's capacity");
        return O3DMI_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(ObeResidentKernel, dim3(1), dim3(kBvBlock), 0, s, X_dev,
                       (int)n_verts, words_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ObeStreamInitAsync(int64_t n_verts, double* scratch_dev, hipStream_t s) {
    const int64_t padded = (int64_t)ObeGrid(n_verts) * kBvBlockVertices;
    hipLaunchKernelGGL(ObeInitKernel, dim3(GridFor(padded, kBlock)),
                       dim3(kBlock), 0, s, scratch_dev, n_verts, padded);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ObeStreamSumsAsync(const double* X_dev, int64_t n_verts, int iteration,
                       double* scratch_dev, ObeWords* words_dev,
                       hipStream_t s) {
    const ObeStream o = CarveObe(scratch_dev, n_verts);
    hipLaunchKernelGGL(ObeSumsKernel, dim3(o.grid), dim3(kBvBlock), 0, s, X_dev,
                       n_verts, iteration, o, words_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int ObeStreamArgmaxAsync(const double* X_dev, int64_t n_verts,
                         double* scratch_dev, ObeWords* words_dev,
                         hipStream_t s) {
    const ObeStream o = CarveObe(scratch_dev, n_verts);
    hipLaunchKernelGGL(ObeArgmaxKernel, dim3(o.grid), dim3(kBvBlock), 0, s,
                       X_dev, n_verts, o, words_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi
