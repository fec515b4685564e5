// Kernels of the TriangleMesh operators (trianglemesh.h): the elementwise
// statements of t/geometry/kernel/TriangleMeshImpl.h, the vertex -> corner and
// edge -> slot incidence structures built with the stable pair sort (sort.h),
// and what ComputeVertexNormals, GetNonManifoldEdges, ClusterConnectedTriangles
// and the selections make of them. Nothing here adds floats in arrival order:
// every float sum walks a sorted list, and the only atomics are integer
// counts, flags and the union-find's CAS.
#include "trianglemesh.h"

#include "mesh_launch.h"
#include "scan.h"
#include "sort.h"
#include "union_find.h"

namespace o3dmi {
namespace {

__device__ __forceinline__ float MeshSqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double MeshSqrt(double x) { return sqrt(x); }

template <typename I>
__global__ void CheckTrianglesKernel(const I* __restrict__ tri, int64_t n3,
                                     int64_t v, int32_t* __restrict__ narrowed,
                                     int* __restrict__ bad) {
    bool any = false;
    O3DMI_GRID_STRIDE(i, n3) {
        const I x = tri[i];
        any |= x < 0 || (int64_t)x >= v;
        if (narrowed) narrowed[i] = (int32_t)x;
    }
    if (any) atomicOr(bad, 1);
}

// ---- elementwise --------------------------------------------------------------
// cross_3x1(p2 - p1, p3 - p1), core/linalg/kernel/Matrix.h:63-73.
template <typename T>
__device__ __forceinline__ void TriangleCross(const T* __restrict__ pos,
                                              const int32_t* __restrict__ tri,
                                              int64_t t, T c[3]) {
    const int64_t i1 = tri[3 * t], i2 = tri[3 * t + 1], i3 = tri[3 * t + 2];
    T v01[3], v02[3];
    v01[0] = pos[3 * i2] - pos[3 * i1];
    v01[1] = pos[3 * i2 + 1] - pos[3 * i1 + 1];
    v01[2] = pos[3 * i2 + 2] - pos[3 * i1 + 2];
    v02[0] = pos[3 * i3] - pos[3 * i1];
    v02[1] = pos[3 * i3 + 1] - pos[3 * i1 + 1];
    v02[2] = pos[3 * i3 + 2] - pos[3 * i1 + 2];
    c[0] = v01[1] * v02[2] - v01[2] * v02[1];
    c[1] = v01[2] * v02[0] - v01[0] * v02[2];
    c[2] = v01[0] * v02[1] - v01[1] * v02[0];
}

template <typename T>
__global__ void TriangleNormalsKernel(const T* __restrict__ pos,
                                      const int32_t* __restrict__ tri,
                                      int64_t m, T* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        T c[3];
        TriangleCross(pos, tri, t, c);
        out[3 * t] = c[0];
        out[3 * t + 1] = c[1];
        out[3 * t + 2] = c[2];
    }
}

template <typename T>
__global__ void TriangleAreasKernel(const T* __restrict__ pos,
                                    const int32_t* __restrict__ tri, int64_t m,
                                    T* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        T c[3];
        TriangleCross(pos, tri, t, c);
        // 0.5 is a double upstream; halving is exact in either width
        out[t] = (T)0.5 * MeshSqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    }
}

// geometry/TriangleMesh.cpp:1175-1182 (Eigen: cross, then norm).
template <typename T>
__global__ void TriangleAreasF64Kernel(const T* __restrict__ pos,
                                       const int32_t* __restrict__ tri,
                                       int64_t m, double* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        double x[3], y[3];
        for (int k = 0; k < 3; ++k) {
            x[k] = (double)pos[3 * i0 + k] - (double)pos[3 * i1 + k];
            y[k] = (double)pos[3 * i0 + k] - (double)pos[3 * i2 + k];
        }
        const double c0 = x[1] * y[2] - x[2] * y[1];
        const double c1 = x[2] * y[0] - x[0] * y[2];
        const double c2 = x[0] * y[1] - x[1] * y[0];
        out[t] = 0.5 * sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    }
}

// TriangleMeshImpl.h:40-69. A row whose x is NaN is not stored to.
template <typename T>
__global__ void NormalizeMeshNormalsKernel(T* __restrict__ ptr, int64_t n) {
    O3DMI_GRID_STRIDE(i, n) {
        T x = ptr[3 * i], y = ptr[3 * i + 1], z = ptr[3 * i + 2];
        if (x != x) continue;
        const T norm = MeshSqrt(x * x + y * y + z * z);
        if (norm > 0) {
            x /= norm;
            y /= norm;
            z /= norm;
        }
        ptr[3 * i] = x;
        ptr[3 * i + 1] = y;
        ptr[3 * i + 2] = z;
    }
}

// out[r] = the values in[512 r ..] added in index order as doubles; one thread
// per run.
template <typename T>
__global__ void RunSumKernel(const T* __restrict__ in, int64_t n,
                             double* __restrict__ out) {
    const int64_t run = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t start = run * kMeshRun;
    if (start >= n) return;
    const int len = (int)(n - start < kMeshRun ? n - start : kMeshRun);
    double sum = (double)in[start];
#pragma unroll 8  // the loads do not depend on the adds: eight in flight
    for (int j = 1; j < len; ++j) sum += (double)in[start + j];
    out[run] = sum;
}

inline int64_t RunsOf(int64_t n) { return (n + kMeshRun - 1) / kMeshRun; }

// ---- vertex -> corners ----------------------------------------------------------
__global__ void CornerPairsKernel(const int32_t* __restrict__ tri, int64_t n3,
                                  uint32_t* __restrict__ keys,
                                  uint32_t* __restrict__ vals,
                                  int32_t* __restrict__ count) {
    O3DMI_GRID_STRIDE(e, n3) {
        const int32_t u = tri[e];
        keys[e] = (uint32_t)u;
        vals[e] = (uint32_t)e;
        atomicAdd(&count[u], 1);
    }
}

constexpr int kWalk = 8;  // normals in flight per walk step

template <typename T>
__global__ void VertexNormalThreadKernel(CornerTable tb, int64_t v,
                                         const T* __restrict__ tn,
                                         T* __restrict__ out,
                                         int32_t* __restrict__ long_list) {
    O3DMI_GRID_STRIDE(u, v) {
        const int cnt = tb.count[u];
        if (cnt > kLongCornerList) {
            long_list[atomicAdd(&long_list[v], 1)] = (int32_t)u;
            continue;
        }
        const uint32_t* corner = tb.corner + tb.start[u];
        T s[3] = {0, 0, 0};
        for (int j0 = 0; j0 < cnt; j0 += kWalk) {
            T n[kWalk][3];
#pragma unroll
            for (int j = 0; j < kWalk; ++j) {
                if (j0 + j < cnt) {
                    const int64_t t = corner[j0 + j] / 3u;
                    n[j][0] = tn[3 * t];
                    n[j][1] = tn[3 * t + 1];
                    n[j][2] = tn[3 * t + 2];
                }
            }
#pragma unroll
            for (int j = 0; j < kWalk; ++j) {
                if (j0 + j < cnt) {
                    s[0] += n[j][0];
                    s[1] += n[j][1];
                    s[2] += n[j][2];
                }
            }
        }
        out[3 * u] = s[0];
        out[3 * u + 1] = s[1];
        out[3 * u + 2] = s[2];
    }
}

// A wave per listed vertex: 64 corners' normals are fetched at once, then
// added in corner order (every lane does the same adds; lane 0 stores).
template <typename T>
__global__ void VertexNormalWaveKernel(CornerTable tb, int64_t v,
                                       const T* __restrict__ tn,
                                       T* __restrict__ out,
                                       const int32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_long = long_list[v];
    for (int64_t w = wave; w < n_long; w += n_waves) {
        const int64_t u = long_list[w];
        const int cnt = tb.count[u];
        const uint32_t* corner = tb.corner + tb.start[u];
        T s[3] = {0, 0, 0};
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            T n[3] = {0, 0, 0};
            if (j0 + lane < cnt) {
                const int64_t t = corner[j0 + lane] / 3u;
                n[0] = tn[3 * t];
                n[1] = tn[3 * t + 1];
                n[2] = tn[3 * t + 2];
            }
            const int len = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int l = 0; l < len; ++l) {
                s[0] += __shfl(n[0], l);
                s[1] += __shfl(n[1], l);
                s[2] += __shfl(n[2], l);
            }
        }
        if (lane == 0) {
            out[3 * u] = s[0];
            out[3 * u + 1] = s[1];
            out[3 * u + 2] = s[2];
        }
    }
}

// ---- edge -> slots --------------------------------------------------------------
// The two vertices of edge slot e = 3 t + k: (v_k, v_(k+1)%3).
__device__ __forceinline__ void SlotEnds(const int32_t* __restrict__ tri,
                                         uint32_t e, uint32_t* lo,
                                         uint32_t* hi) {
    const uint32_t t = e / 3u, k = e - 3u * t;
    const uint32_t a = (uint32_t)tri[e];
    const uint32_t b = (uint32_t)tri[3u * t + (k == 2u ? 0u : k + 1u)];
    *lo = a < b ? a : b;
    *hi = a < b ? b : a;
}

// kWhich 0: keys[j] = hi of slot j, vals[j] = j (the unsorted table);
// 1: keys[j] = lo of slot vals[j]; 2: keys[j] = hi of slot vals[j].
template <int kWhich>
__global__ void SlotKeysKernel(const int32_t* __restrict__ tri, int64_t n3,
                               uint32_t* __restrict__ keys,
                               uint32_t* __restrict__ vals) {
    O3DMI_GRID_STRIDE(j, n3) {
        uint32_t lo, hi;
        if (kWhich == 0) vals[j] = (uint32_t)j;
        SlotEnds(tri, kWhich == 0 ? (uint32_t)j : vals[j], &lo, &hi);
        keys[j] = kWhich == 1 ? lo : hi;
    }
}

__global__ void NonManifoldFlagsKernel(EdgeTable tb, int64_t n3,
                                       bool allow_boundary,
                                       int32_t* __restrict__ flags) {
    O3DMI_GRID_STRIDE(j, n3) {
        int32_t flag = 0;
        if (FirstOfRun(tb, j)) {
            // the first slot of an edge: nothing past the third slot changes
            // either rule
            int mult = 1;
            while (mult < 3 && j + mult < n3 && SameEdge(tb, j, j + mult))
                ++mult;
            flag = allow_boundary ? mult > 2 : mult != 2;
        }
        flags[j] = flag;
    }
}

template <typename I>
__global__ void EmitEdgesKernel(EdgeTable tb, int64_t n3,
                                const int32_t* __restrict__ flags,
                                const int64_t* __restrict__ pos,
                                I* __restrict__ out) {
    O3DMI_GRID_STRIDE(j, n3) {
        if (!flags[j]) continue;
        out[2 * pos[j]] = (I)tb.lo[j];
        out[2 * pos[j] + 1] = (I)tb.hi[j];
    }
}

// ---- connected components ---------------------------------------------------------
__global__ void IotaKernel(int* __restrict__ p, int64_t n) {
    O3DMI_GRID_STRIDE(i, n) p[i] = (int)i;
}

// A slot that continues an edge unites its triangle with the slot before it:
// the edge's slots end up in one tree, as if each had been united with the
// first.
__global__ void EdgeUnionKernel(EdgeTable tb, int64_t n3,
                                int* __restrict__ parent) {
    O3DMI_GRID_STRIDE(j, n3) {
        if (FirstOfRun(tb, j)) continue;
        const int a = (int)(tb.slot[j] / 3u), b = (int)(tb.slot[j - 1] / 3u);
        if (a != b) DbscanUnite(parent, a, b);
    }
}

__global__ void FlattenKernel(int* __restrict__ parent, int64_t m,
                              int* __restrict__ root,
                              int32_t* __restrict__ is_root) {
    O3DMI_GRID_STRIDE(t, m) {
        const int r = DbscanFind(parent, (int)t);
        root[t] = r;
        is_root[t] = r == (int)t;
    }
}

__global__ void ClusterLabelsKernel(const int* __restrict__ root,
                                    const int64_t* __restrict__ rank, int64_t m,
                                    int32_t* __restrict__ labels,
                                    int32_t* __restrict__ counts) {
    O3DMI_GRID_STRIDE(t, m) {
        const int32_t label = (int32_t)rank[root[t]];
        labels[t] = label;
        // One atomic per label a wave holds, not per triangle: neighbours in
        // index mostly share a cluster, and two million adds to one word
        // took 23 ms. The lanes of the first lane's label leave together.
        const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
        bool counted = false;
        while (!counted) {
            const int32_t lead = __builtin_amdgcn_readfirstlane(label);
            const unsigned long long same = __ballot(label == lead);
            if (label == lead) {
                if ((same & lt) == 0ull)
                    atomicAdd(&counts[lead], __popcll(same));
                counted = true;
            }
        }
    }
}

__global__ void LabelPairsKernel(const int32_t* __restrict__ labels, int64_t m,
                                 uint32_t* __restrict__ keys,
                                 uint32_t* __restrict__ vals) {
    O3DMI_GRID_STRIDE(t, m) {
        keys[t] = (uint32_t)labels[t];
        vals[t] = (uint32_t)t;
    }
}

__global__ void ClusterRunCountsKernel(const int32_t* __restrict__ counts,
                                       int64_t n, int32_t* __restrict__ runs) {
    O3DMI_GRID_STRIDE(c, n) runs[c] = (counts[c] + kMeshRun - 1) / kMeshRun;
}

// One thread per run of every cluster; the run's cluster is the last one
// whose first run is not past it (every cluster has at least one run).
__global__ void ClusterRunSumKernel(const double* __restrict__ area,
                                    const uint32_t* __restrict__ sorted_tri,
                                    const int32_t* __restrict__ counts,
                                    const int64_t* __restrict__ start,
                                    const int64_t* __restrict__ run_start,
                                    int64_t n_clusters, int64_t max_runs,
                                    double* __restrict__ run_sums) {
    const int64_t last = n_clusters - 1;
    const int64_t n_runs =
            run_start[last] + (counts[last] + kMeshRun - 1) / kMeshRun;
    O3DMI_GRID_STRIDE(r, max_runs) {
        if (r >= n_runs) break;
        int64_t lo = 0, hi = last;  // run_start[lo] <= r
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (run_start[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
        const int64_t first = (r - run_start[lo]) * kMeshRun;
        const int64_t left = counts[lo] - first;
        const int len = (int)(left < kMeshRun ? left : kMeshRun);
        const uint32_t* member = sorted_tri + start[lo] + first;
        double sum = area[member[0]];
#pragma unroll 8
        for (int j = 1; j < len; ++j) sum += area[member[j]];
        run_sums[r] = sum;
    }
}

__global__ void ClusterAreaKernel(const double* __restrict__ run_sums,
                                  const int32_t* __restrict__ counts,
                                  const int64_t* __restrict__ run_start,
                                  int64_t n_clusters,
                                  double* __restrict__ area_out) {
    O3DMI_GRID_STRIDE(c, n_clusters) {
        const int runs = (counts[c] + kMeshRun - 1) / kMeshRun;
        const double* v = run_sums + run_start[c];
        double sum = v[0];
        for (int j = 1; j < runs; ++j) sum += v[j];
        area_out[c] = sum;
    }
}

__global__ void WidenCountsKernel(const int32_t* __restrict__ in, int64_t n,
                                  int64_t* __restrict__ out) {
    O3DMI_GRID_STRIDE(i, n) out[i] = in[i];
}

// ---- selection ------------------------------------------------------------------
__global__ void MaskToFlagsKernel(const uint8_t* __restrict__ mask, int64_t n,
                                  int32_t* __restrict__ flags) {
    O3DMI_GRID_STRIDE(i, n) flags[i] = mask[i] != 0;
}

__global__ void FlagsToMaskKernel(const int32_t* __restrict__ flags, int64_t n,
                                  uint8_t* __restrict__ mask) {
    O3DMI_GRID_STRIDE(i, n) mask[i] = flags[i] != 0;
}

__global__ void MarkTriangleVerticesKernel(const int32_t* __restrict__ tri,
                                           int64_t m,
                                           const int32_t* __restrict__ tflags,
                                           int32_t* __restrict__ vflags) {
    O3DMI_GRID_STRIDE(t, m) {
        if (tflags && !tflags[t]) continue;
        // every writer stores the same value
        vflags[tri[3 * t]] = 1;
        vflags[tri[3 * t + 1]] = 1;
        vflags[tri[3 * t + 2]] = 1;
    }
}

__global__ void MarkIndexedVerticesKernel(const int64_t* __restrict__ indices,
                                          int64_t k, int64_t v,
                                          int32_t* __restrict__ vflags,
                                          unsigned long long* ignored) {
    unsigned long long mine = 0;
    O3DMI_GRID_STRIDE(r, k) {
        const int64_t u = indices[r];
        if (u < 0 || u >= v) ++mine;
        else vflags[u] = 1;
    }
    if (mine) atomicAdd(ignored, mine);
}

__global__ void TrianglesOfVerticesKernel(const int32_t* __restrict__ tri,
                                          int64_t m,
                                          const int32_t* __restrict__ vflags,
                                          int32_t* __restrict__ tflags) {
    O3DMI_GRID_STRIDE(t, m)
        tflags[t] = vflags[tri[3 * t]] && vflags[tri[3 * t + 1]] &&
                    vflags[tri[3 * t + 2]];
}

template <typename I>
__global__ void RemapTrianglesKernel(const int32_t* __restrict__ tri, int64_t m,
                                     const int32_t* __restrict__ tflags,
                                     const int64_t* __restrict__ tpos,
                                     const int64_t* __restrict__ vnew,
                                     I* __restrict__ out) {
    O3DMI_GRID_STRIDE(t, m) {
        if (tflags && !tflags[t]) continue;
        const int64_t p = tpos ? tpos[t] : t;
        out[3 * p] = (I)vnew[tri[3 * t]];
        out[3 * p + 1] = (I)vnew[tri[3 * t + 1]];
        out[3 * p + 2] = (I)vnew[tri[3 * t + 2]];
    }
}

inline size_t Align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int CheckTrianglesAsync(const void* triangles_dev, int64_t m, int index_dtype,
                        int64_t v, int32_t* narrowed_dev, int* bad_dev,
                        hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(CheckTrianglesKernel<int64_t>, 3 * m,
                     (const int64_t*)triangles_dev, 3 * m, v, narrowed_dev,
                     bad_dev);
    else
        O3DMI_LAUNCH(CheckTrianglesKernel<int32_t>, 3 * m,
                     (const int32_t*)triangles_dev, 3 * m, v, narrowed_dev,
                     bad_dev);
    return O3DMI_OK;
}

int TriangleNormalsAsync(const void* positions_dev, int dtype,
                         const int32_t* tri, int64_t m, void* out_dev,
                         hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(TriangleNormalsKernel<double>, m,
                     (const double*)positions_dev, tri, m, (double*)out_dev);
    else
        O3DMI_LAUNCH(TriangleNormalsKernel<float>, m,
                     (const float*)positions_dev, tri, m, (float*)out_dev);
    return O3DMI_OK;
}

int TriangleAreasAsync(const void* positions_dev, int dtype,
                       const int32_t* tri, int64_t m, void* out_dev,
                       hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(TriangleAreasKernel<double>, m,
                     (const double*)positions_dev, tri, m, (double*)out_dev);
    else
        O3DMI_LAUNCH(TriangleAreasKernel<float>, m,
                     (const float*)positions_dev, tri, m, (float*)out_dev);
    return O3DMI_OK;
}

int TriangleAreasF64Async(const void* positions_dev, int dtype,
                          const int32_t* tri, int64_t m, double* out_dev,
                          hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(TriangleAreasF64Kernel<double>, m,
                     (const double*)positions_dev, tri, m, out_dev);
    else
        O3DMI_LAUNCH(TriangleAreasF64Kernel<float>, m,
                     (const float*)positions_dev, tri, m, out_dev);
    return O3DMI_OK;
}

int NormalizeMeshNormalsAsync(void* normals_dev, int64_t n, int dtype,
                              hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(NormalizeMeshNormalsKernel<double>, n,
                     (double*)normals_dev, n);
    else
        O3DMI_LAUNCH(NormalizeMeshNormalsKernel<float>, n, (float*)normals_dev,
                     n);
    return O3DMI_OK;
}

size_t RunSumScratchDoubles(int64_t n) {
    int64_t m = RunsOf(n > 0 ? n : 1);
    size_t total = (size_t)m;
    while (m > 1) {
        m = RunsOf(m);
        total += (size_t)m;
    }
    return total;
}

int RunSumTreeAsync(const void* values_dev, int64_t n, int dtype,
                    double* sums_dev, const double** total_dev,
                    hipStream_t s) {
    O3DMI_REQUIRE(values_dev && n > 0 && sums_dev && total_dev,
                  "null argument");
    int64_t m = RunsOf(n);
    const dim3 block(64);
    if (dtype == O3DMI_F64)
        hipLaunchKernelGGL(RunSumKernel<double>, dim3(GridFor(m, 64, 1 << 30)),
                           block, 0, s, (const double*)values_dev, n,
                           sums_dev);
    else
        hipLaunchKernelGGL(RunSumKernel<float>, dim3(GridFor(m, 64, 1 << 30)),
                           block, 0, s, (const float*)values_dev, n, sums_dev);
    double* level = sums_dev;
    while (m > 1) {
        const int64_t runs = RunsOf(m);
        hipLaunchKernelGGL(RunSumKernel<double>,
                           dim3(GridFor(runs, 64, 1 << 30)), block, 0, s,
                           level, m, level + m);
        level += m;
        m = runs;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    *total_dev = level;
    return O3DMI_OK;
}

size_t IncidenceScratchBytes(int64_t m, int64_t v) {
    const size_t sort = SortPairsScratchBytes(3 * m);
    const size_t scan = ScanScratchBytes(v > 3 * m ? v : 3 * m);
    return Align256(sort > scan ? sort : scan);
}

int BuildCornerTableAsync(const int32_t* tri, int64_t m, int64_t v,
                          const CornerTable& table, void* scratch_dev,
                          hipStream_t s) {
    O3DMI_HIP_CHECK(hipMemsetAsync(table.count, 0, sizeof(int32_t) * v, s));
    O3DMI_LAUNCH(CornerPairsKernel, 3 * m, tri, 3 * m, table.vertex,
                 table.corner, table.count);
    int st = SortPairsAsync(table.vertex, table.corner, 3 * m, BitsFor(v),
                            scratch_dev, s);
    if (st) return st;
    return PrefixSumAsync(table.count, v, false, table.start, nullptr,
                          scratch_dev, s);
}

int VertexNormalSumAsync(const CornerTable& table, int64_t v,
                         const void* triangle_normals_dev, int dtype,
                         void* out_dev, int32_t* long_list_dev,
                         hipStream_t s) {
    const dim3 waves = WaveGrid(v);
    if (dtype == O3DMI_F64) {
        O3DMI_LAUNCH(VertexNormalThreadKernel<double>, v, table, v,
                     (const double*)triangle_normals_dev, (double*)out_dev,
                     long_list_dev);
        hipLaunchKernelGGL(VertexNormalWaveKernel<double>, waves, dim3(kBlock),
                           0, s, table, v, (const double*)triangle_normals_dev,
                           (double*)out_dev, long_list_dev);
    } else {
        O3DMI_LAUNCH(VertexNormalThreadKernel<float>, v, table, v,
                     (const float*)triangle_normals_dev, (float*)out_dev,
                     long_list_dev);
        hipLaunchKernelGGL(VertexNormalWaveKernel<float>, waves, dim3(kBlock),
                           0, s, table, v, (const float*)triangle_normals_dev,
                           (float*)out_dev, long_list_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int BuildEdgeTableAsync(const int32_t* tri, int64_t m, int64_t v,
                        const EdgeTable& table, void* scratch_dev,
                        hipStream_t s) {
    const int bits = BitsFor(v);
    // by hi first, then stably by lo: ascending (lo, hi, slot)
    O3DMI_LAUNCH(SlotKeysKernel<0>, 3 * m, tri, 3 * m, table.hi, table.slot);
    int st = SortPairsAsync(table.hi, table.slot, 3 * m, bits, scratch_dev, s);
    if (st) return st;
    O3DMI_LAUNCH(SlotKeysKernel<1>, 3 * m, tri, 3 * m, table.lo, table.slot);
    st = SortPairsAsync(table.lo, table.slot, 3 * m, bits, scratch_dev, s);
    if (st) return st;
    O3DMI_LAUNCH(SlotKeysKernel<2>, 3 * m, tri, 3 * m, table.hi, table.slot);
    return O3DMI_OK;
}

int NonManifoldFlagsAsync(const EdgeTable& table, int64_t n_slots,
                          bool allow_boundary, int32_t* flags_dev,
                          hipStream_t s) {
    O3DMI_LAUNCH(NonManifoldFlagsKernel, n_slots, table, n_slots,
                 allow_boundary, flags_dev);
    return O3DMI_OK;
}

int EmitEdgesAsync(const EdgeTable& table, int64_t n_slots,
                   const int32_t* flags_dev, const int64_t* pos_dev,
                   int index_dtype, void* edges_out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(EmitEdgesKernel<int64_t>, n_slots, table, n_slots,
                     flags_dev, pos_dev, (int64_t*)edges_out_dev);
    else
        O3DMI_LAUNCH(EmitEdgesKernel<int32_t>, n_slots, table, n_slots,
                     flags_dev, pos_dev, (int32_t*)edges_out_dev);
    return O3DMI_OK;
}

int IotaAsync(int* p_dev, int64_t n, hipStream_t s) {
    O3DMI_LAUNCH(IotaKernel, n, p_dev, n);
    return O3DMI_OK;
}

int ClusterRootsAsync(const EdgeTable& table, int64_t m, int* parent_dev,
                      int* root_dev, int32_t* is_root_dev, hipStream_t s) {
    const int st = IotaAsync(parent_dev, m, s);
    if (st) return st;
    O3DMI_LAUNCH(EdgeUnionKernel, 3 * m, table, 3 * m, parent_dev);
    O3DMI_LAUNCH(FlattenKernel, m, parent_dev, m, root_dev, is_root_dev);
    return O3DMI_OK;
}

int ClusterLabelsAsync(const int* root_dev, const int64_t* rank_dev, int64_t m,
                       int32_t* labels_dev, int32_t* counts_dev,
                       hipStream_t s) {
    O3DMI_LAUNCH(ClusterLabelsKernel, m, root_dev, rank_dev, m, labels_dev,
                 counts_dev);
    return O3DMI_OK;
}

int LabelPairsAsync(const int32_t* labels_dev, int64_t m, uint32_t* keys_dev,
                    uint32_t* vals_dev, hipStream_t s) {
    O3DMI_LAUNCH(LabelPairsKernel, m, labels_dev, m, keys_dev, vals_dev);
    return O3DMI_OK;
}

int ClusterRunCountsAsync(const int32_t* counts_dev, int64_t n_clusters,
                          int32_t* runs_dev, hipStream_t s) {
    O3DMI_LAUNCH(ClusterRunCountsKernel, n_clusters, counts_dev, n_clusters,
                 runs_dev);
    return O3DMI_OK;
}

int ClusterAreaSumsAsync(const double* area_dev, const uint32_t* sorted_tri_dev,
                         const int32_t* counts_dev, const int64_t* start_dev,
                         const int64_t* run_start_dev, int64_t n_clusters,
                         int64_t max_runs, double* run_sums_dev,
                         double* area_out_dev, hipStream_t s) {
    O3DMI_REQUIRE(n_clusters > 0, "cluster areas: no cluster");
    hipLaunchKernelGGL(ClusterRunSumKernel,
                       dim3(GridFor(max_runs, 64, 1 << 30)), dim3(64), 0, s,
                       area_dev, sorted_tri_dev, counts_dev, start_dev,
                       run_start_dev, n_clusters, max_runs, run_sums_dev);
    O3DMI_LAUNCH(ClusterAreaKernel, n_clusters, run_sums_dev, counts_dev,
                 run_start_dev, n_clusters, area_out_dev);
    return O3DMI_OK;
}

int WidenCountsAsync(const int32_t* counts_dev, int64_t n, int64_t* out_dev,
                     hipStream_t s) {
    O3DMI_LAUNCH(WidenCountsKernel, n, counts_dev, n, out_dev);
    return O3DMI_OK;
}

int MaskToFlagsAsync(const uint8_t* mask_dev, int64_t n, int32_t* flags_dev,
                     hipStream_t s) {
    O3DMI_LAUNCH(MaskToFlagsKernel, n, mask_dev, n, flags_dev);
    return O3DMI_OK;
}

int FlagsToMaskAsync(const int32_t* flags_dev, int64_t n, uint8_t* mask_dev,
                     hipStream_t s) {
    O3DMI_LAUNCH(FlagsToMaskKernel, n, flags_dev, n, mask_dev);
    return O3DMI_OK;
}

int MarkTriangleVerticesAsync(const int32_t* tri, int64_t m,
                              const int32_t* tri_flags_dev,
                              int32_t* vertex_flags_dev, hipStream_t s) {
    O3DMI_LAUNCH(MarkTriangleVerticesKernel, m, tri, m, tri_flags_dev,
                 vertex_flags_dev);
    return O3DMI_OK;
}

int MarkIndexedVerticesAsync(const int64_t* indices_dev, int64_t k, int64_t v,
                             int32_t* vertex_flags_dev,
                             unsigned long long* ignored_dev, hipStream_t s) {
    O3DMI_LAUNCH(MarkIndexedVerticesKernel, k, indices_dev, k, v,
                 vertex_flags_dev, ignored_dev);
    return O3DMI_OK;
}

int TrianglesOfVerticesAsync(const int32_t* tri, int64_t m,
                             const int32_t* vertex_flags_dev,
                             int32_t* tri_flags_dev, hipStream_t s) {
    O3DMI_LAUNCH(TrianglesOfVerticesKernel, m, tri, m, vertex_flags_dev,
                 tri_flags_dev);
    return O3DMI_OK;
}

int RemapTrianglesAsync(const int32_t* tri, int64_t m,
                        const int32_t* tri_flags_dev,
                        const int64_t* tri_pos_dev,
                        const int64_t* vertex_new_dev, int index_dtype,
                        void* out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(RemapTrianglesKernel<int64_t>, m, tri, m, tri_flags_dev,
                     tri_pos_dev, vertex_new_dev, (int64_t*)out_dev);
    else
        O3DMI_LAUNCH(RemapTrianglesKernel<int32_t>, m, tri, m, tri_flags_dev,
                     tri_pos_dev, vertex_new_dev, (int32_t*)out_dev);
    return O3DMI_OK;
}

}  // namespace o3dmi
