// Rigid multiway fragment alignment, the device half
// (t/pipelines/kernel/FillInLinearSystemImpl.h:27-154 FillInRigidAlignmentTerm,
// t/pipelines/slac/FillInLinearSystemImpl.h:36-100 its per-edge caller,
// slac/SLACOptimizer.cpp:85-204 the correspondence set of an edge).
//
// The reference adds, per correspondence, a 12x12 block J J^T, 12 values J r
// and r r with float atomics, J = (J6, -J6). The block is [[A, -A], [-A, A]]
// and the rhs [b, -b] with A = sum J6 J6^T, b = sum J6 r: 21 + 6 + 1 sums and
// the pair count say everything. Per-pair terms are float32 in the
// reference's operation order, running sums float64 in a fixed tree
// (reduce_sums.h), no floating-point atomics.
//
// RigidTermsKernel serves ALL edges of an iteration in one launch: a work
// item is (edge, tile of 1024 of its correspondences); a lane reads 4 index
// pairs, gathers p_a, n_a from fragment i and q_b from fragment j through a
// device table of fragment pointers, applies the edge's poses (wave-uniform:
// scalar loads into SGPRs) and adds the widened products to 29 float64
// running sums. One partial row per tile, then one workgroup per edge adds
// the edge's rows in row order.
#include "common.h"
#include "reduce_sums.h"
#include "slac.h"
#include "slac_device.h"

namespace o3dmi {
namespace {

static_assert(kSlacBlock == kSumsBlock, "shared reduction geometry");

__global__ void __launch_bounds__(kSlacBlock)
RigidTermsKernel(const SlacFragment* __restrict__ frags,
                 const SlacEdge* __restrict__ edges, int n_edges,
                 float threshold, double* __restrict__ partials,
                 int* __restrict__ bad) {
    // the edge of this tile: the last one whose first tile is not behind it
    // (edges without correspondences own no tile). Wave-uniform.
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = n_edges - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (edges[mid].tile_first <= tile)
            lo = mid;
        else
            hi = mid - 1;
    }
    const SlacEdge& ed = edges[lo];
    const SlacFragment fi = frags[ed.i];
    const SlacFragment fj = frags[ed.j];
    const int64_t count = ed.count;
    // pointers that come out of a table in memory are generic (flat loads);
    // these are global
    using FloatG = const float __attribute__((address_space(1)));
    typedef long long Pair __attribute__((ext_vector_type(2)));
    using PairG = const Pair __attribute__((address_space(1)));
    FloatG* const pos_i = (FloatG*)fi.positions;
    FloatG* const nrm_i = (FloatG*)fi.normals;
    FloatG* const pos_j = (FloatG*)fj.positions;
    PairG* const corres = (PairG*)ed.corres;
    const int64_t base = (tile - ed.tile_first) * kSlacTile + threadIdx.x;

    // all index pairs, then all gathers, then the arithmetic: 4 x 3 rows in
    // flight per lane
    int64_t a[kSlacItems], b[kSlacItems];
    bool ok[kSlacItems];
    bool out_of_range = false;
#pragma unroll
    for (int k = 0; k < kSlacItems; ++k) {
        const int64_t c = base + (int64_t)k * kSlacBlock;
        ok[k] = c < count;
        a[k] = 0;
        b[k] = 0;
        if (ok[k]) {
            const Pair ab = corres[c];
            a[k] = ab.x;
            b[k] = ab.y;
        }
        if (a[k] < 0 || a[k] >= fi.n || b[k] < 0 || b[k] >= fj.n) {
            out_of_range = out_of_range || ok[k];
            ok[k] = false;
        }
    }
    float p[kSlacItems][3], q[kSlacItems][3], n[kSlacItems][3];
#pragma unroll
    for (int k = 0; k < kSlacItems; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[k][c] = ok[k] ? pos_i[3 * a[k] + c] : 0.f;
            n[k][c] = ok[k] ? nrm_i[3 * a[k] + c] : 0.f;
            q[k][c] = ok[k] ? pos_j[3 * b[k] + c] : 0.f;
        }
    }
    double A[kSlacSums];
#pragma unroll
    for (int k = 0; k < kSlacSums; ++k) A[k] = 0;
#pragma unroll
    for (int k = 0; k < kSlacItems; ++k) {
        const float px = Row(ed.Ti + 0, p[k][0], p[k][1], p[k][2]);
        const float py = Row(ed.Ti + 4, p[k][0], p[k][1], p[k][2]);
        const float pz = Row(ed.Ti + 8, p[k][0], p[k][1], p[k][2]);
        const float qx = Row(ed.Tj + 0, q[k][0], q[k][1], q[k][2]);
        const float qy = Row(ed.Tj + 4, q[k][0], q[k][1], q[k][2]);
        const float qz = Row(ed.Tj + 8, q[k][0], q[k][1], q[k][2]);
        const float nx = RotRow(ed.Ti + 0, n[k][0], n[k][1], n[k][2]);
        const float ny = RotRow(ed.Ti + 4, n[k][0], n[k][1], n[k][2]);
        const float nz = RotRow(ed.Ti + 8, n[k][0], n[k][1], n[k][2]);
        AccumulateRigidPair(A, ok[k], px, py, pz, qx, qy, qz, nx, ny, nz,
                            threshold);
    }
    if (out_of_range) atomicOr(bad, 1);
    BlockSumAndStore<kSlacSums>(A, partials);
}

__global__ void __launch_bounds__(kSlacBlock)
RigidTermsFinalKernel(const double* __restrict__ partials,
                      const SlacEdge* __restrict__ edges, int n_edges,
                      int64_t n_tiles, const int* __restrict__ bad,
                      double* __restrict__ sums) {
    __shared__ double lds[kSlacBlock / 32][32];
    if (*bad) return;
    const int e = blockIdx.x;
    const int64_t first = edges[e].tile_first;
    const int64_t last = e + 1 < n_edges ? edges[e + 1].tile_first : n_tiles;
    SumRows(partials, first, last, lds);
    if (threadIdx.x < kSlacSums)
        sums[(int64_t)e * kSlacSums + threadIdx.x] = lds[0][threadIdx.x];
}

// The reference's seam: the rows come gathered and transformed.
__global__ void __launch_bounds__(kSlacBlock)
RigidTermsSeamKernel(const float* __restrict__ Ti_ps,
                     const float* __restrict__ Tj_qs,
                     const float* __restrict__ Ri_normal_ps, int64_t count,
                     float threshold, double* __restrict__ partials) {
    const int64_t base = (int64_t)blockIdx.x * kSlacTile + threadIdx.x;
    float p[kSlacItems][3], q[kSlacItems][3], n[kSlacItems][3];
    bool ok[kSlacItems];
#pragma unroll
    for (int k = 0; k < kSlacItems; ++k) {
        const int64_t c = base + (int64_t)k * kSlacBlock;
        ok[k] = c < count;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            p[k][d] = ok[k] ? Ti_ps[3 * c + d] : 0.f;
            q[k][d] = ok[k] ? Tj_qs[3 * c + d] : 0.f;
            n[k][d] = ok[k] ? Ri_normal_ps[3 * c + d] : 0.f;
        }
    }
    double A[kSlacSums];
#pragma unroll
    for (int k = 0; k < kSlacSums; ++k) A[k] = 0;
#pragma unroll
    for (int k = 0; k < kSlacItems; ++k)
        AccumulateRigidPair(A, ok[k], p[k][0], p[k][1], p[k][2], q[k][0],
                            q[k][1], q[k][2], n[k][0], n[k][1], n[k][2],
                            threshold);
    BlockSumAndStore<kSlacSums>(A, partials);
}

// The tail of the seam, one workgroup: the 12x12 block [[A, -A], [-A, A]],
// the rhs [b, -b] and the residual go into the caller's float32 system at
// rows / columns 6i..6i+5, 6j..6j+5, every entry updated once
// (kernel/FillInLinearSystemImpl.h:129-153).
__global__ void __launch_bounds__(kSlacBlock)
RigidSeamScatterKernel(const double* __restrict__ partials, int64_t n_rows,
                       float* __restrict__ AtA, float* __restrict__ Atb,
                       float* __restrict__ residual, int64_t n_vars, int i,
                       int j) {
    __shared__ double lds[kSlacBlock / 32][32];
    SumRows(partials, 0, n_rows, lds);
    const int t = threadIdx.x;
    if (t < 144) {
        const int li = t / 12, lj = t % 12;
        const int u = li % 6, v = lj % 6;
        const int s = u >= v ? u * (u + 1) / 2 + v : v * (v + 1) / 2 + u;
        const double val = (li < 6) == (lj < 6) ? lds[0][s] : -lds[0][s];
        const int64_t row = (int64_t)(li < 6 ? i : j) * 6 + u;
        const int64_t col = (int64_t)(lj < 6 ? i : j) * 6 + v;
        AtA[row * n_vars + col] += (float)val;
    } else if (t < 156) {
        const int l = t - 144, u = l % 6;
        const double val = l < 6 ? lds[0][21 + u] : -lds[0][21 + u];
        Atb[(int64_t)(l < 6 ? i : j) * 6 + u] += (float)val;
    } else if (t == 156) {
        residual[0] += (float)lds[0][27];
    }
}

struct Pose12 {
    float t[12];
};

// ConvertCorrespondencesTargetIndexedToCx2Form and the inlier count of
// GetCorrespondenceSetForPointCloudPair (SLACOptimizer.cpp:85-118,170-186).
__global__ void __launch_bounds__(kBlock)
CorrespondenceSetKernel(const int32_t* __restrict__ idx,
                        const int64_t* __restrict__ position, int64_t n_i,
                        int64_t n_j, const float* __restrict__ pos_i,
                        const float* __restrict__ pos_j, Pose12 Ti, Pose12 Tj,
                        float d2, int64_t* __restrict__ corres,
                        unsigned long long* __restrict__ inliers,
                        int* __restrict__ bad) {
    // whole waves stay in the loop: the ballot below needs every lane
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (n_i + stride - 1) / stride;
    unsigned long long mine = 0;
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t a = it * stride + blockIdx.x * (int64_t)blockDim.x +
                          threadIdx.x;
        bool in = false;
        if (a < n_i) {
            const int64_t b = idx[a];
            if (b >= n_j) {
                atomicOr(bad, 1);
            } else if (b >= 0) {
                const int64_t o = position[a];
                corres[2 * o] = a;
                corres[2 * o + 1] = b;
                const float x = pos_i[3 * a], y = pos_i[3 * a + 1],
                            z = pos_i[3 * a + 2];
                const float u = pos_j[3 * b], v = pos_j[3 * b + 1],
                            w = pos_j[3 * b + 2];
                const float dx = Row(Ti.t + 0, x, y, z) - Row(Tj.t + 0, u, v, w);
                const float dy = Row(Ti.t + 4, x, y, z) - Row(Tj.t + 4, u, v, w);
                const float dz = Row(Ti.t + 8, x, y, z) - Row(Tj.t + 8, u, v, w);
                in = dx * dx + dy * dy + dz * dz <= d2;
            }
        }
        mine += (unsigned long long)__popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(inliers, mine);
}

}  // namespace

int64_t SlacLayoutTiles(SlacEdge* edges_host, int n_edges) {
    int64_t t = 0;
    for (int e = 0; e < n_edges; ++e) {
        edges_host[e].tile_first = t;
        t += SlacTiles(edges_host[e].count);
    }
    return t;
}

int SlacRigidTermsAsync(const SlacFragment* frags_dev,
                        const SlacEdge* edges_dev, int n_edges,
                        int64_t n_tiles, float threshold, double* partials_dev,
                        int* bad_dev, double* sums_dev, hipStream_t s) {
    if (n_edges <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n_tiles < (1ll << 31), "slac: too many correspondences");
    if (n_tiles > 0)
        hipLaunchKernelGGL(RigidTermsKernel, dim3((unsigned)n_tiles),
                           dim3(kSlacBlock), 0, s, frags_dev, edges_dev,
                           n_edges, threshold, partials_dev, bad_dev);
    return SlacEdgeSumsAsync(partials_dev, edges_dev, n_edges, n_tiles,
                             bad_dev, sums_dev, s);
}

int SlacEdgeSumsAsync(const double* partials_dev, const SlacEdge* edges_dev,
                      int n_edges, int64_t n_tiles, const int* bad_dev,
                      double* sums_dev, hipStream_t s) {
    if (n_edges <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(RigidTermsFinalKernel, dim3((unsigned)n_edges),
                       dim3(kSlacBlock), 0, s, partials_dev, edges_dev,
                       n_edges, n_tiles, bad_dev, sums_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacCorrespondenceSetAsync(const int32_t* idx_dev,
                               const int64_t* position_dev, int64_t n_i,
                               int64_t n_j, const float* positions_i_dev,
                               const float* positions_j_dev, const float* Ti,
                               const float* Tj, float d2, int64_t* corres_dev,
                               unsigned long long* inliers_dev, int* bad_dev,
                               hipStream_t s) {
    if (n_i <= 0) return O3DMI_OK;
    Pose12 ti, tj;
    for (int k = 0; k < 12; ++k) {
        ti.t[k] = Ti[k];
        tj.t[k] = Tj[k];
    }
    hipLaunchKernelGGL(CorrespondenceSetKernel, dim3(GridFor(n_i, kBlock)),
                       dim3(kBlock), 0, s, idx_dev, position_dev, n_i, n_j,
                       positions_i_dev, positions_j_dev, ti, tj, d2,
                       corres_dev, inliers_dev, bad_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi

using namespace o3dmi;

extern "C" {

int o3dmi_fill_in_rigid_alignment_term(float* AtA_dev, float* Atb_dev,
                                       float* residual_dev, int64_t n_vars,
                                       const float* Ti_ps_dev,
                                       const float* Tj_qs_dev,
                                       const float* Ri_normal_ps_dev,
                                       int64_t n, int i, int j,
                                       float threshold,
                                       o3dmi_stream_t stream) {
    O3DMI_REQUIRE(AtA_dev && Atb_dev && residual_dev, "null argument");
    O3DMI_REQUIRE(n >= 0 && (n == 0 || (Ti_ps_dev && Tj_qs_dev &&
                                        Ri_normal_ps_dev)),
                  "null argument");
    O3DMI_REQUIRE(n_vars > 0 && n_vars % 6 == 0,
                  "n_vars must be 6 x the number of nodes");
    O3DMI_REQUIRE(i >= 0 && j >= 0 && i < n_vars / 6 && j < n_vars / 6,
                  "node id out of range");
    O3DMI_REQUIRE(i != j, "an edge joins two different nodes");
    const int64_t tiles = SlacTiles(n);
    O3DMI_REQUIRE(tiles < (1ll << 31), "slac: too many correspondences");
    hipStream_t s = (hipStream_t)stream;
    double* partials = nullptr;
    O3DMI_HIP_CHECK(hipMallocAsync(
            (void**)&partials,
            sizeof(double) * kSlacSums * (size_t)(tiles > 0 ? tiles : 1), s));
    if (tiles > 0)
        hipLaunchKernelGGL(RigidTermsSeamKernel, dim3((unsigned)tiles),
                           dim3(kSlacBlock), 0, s, Ti_ps_dev, Tj_qs_dev,
                           Ri_normal_ps_dev, n, threshold, partials);
    hipLaunchKernelGGL(RigidSeamScatterKernel, dim3(1), dim3(kSlacBlock), 0,
                       s, partials, tiles, AtA_dev, Atb_dev, residual_dev,
                       n_vars, i, j);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(partials, s);
    O3DMI_HIP_CHECK(e);
    return O3DMI_OK;
}

int o3dmi_slac_rigid_terms(const void* const* positions_dev,
                           const void* const* normals_dev,
                           const int64_t* sizes, int n_fragments,
                           const int32_t* edges, const void* const* corres_dev,
                           const int64_t* corres_counts, int n_edges,
                           const double* poses, float threshold,
                           double* sums_dev, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(n_fragments > 0 && n_edges >= 0, "empty pose graph");
    O3DMI_REQUIRE(positions_dev && normals_dev && sizes && poses,
                  "null argument");
    if (n_edges == 0) return O3DMI_OK;
    O3DMI_REQUIRE(edges && corres_dev && corres_counts && sums_dev,
                  "null argument");
    std::vector<SlacFragment> frags((size_t)n_fragments);
    for (int k = 0; k < n_fragments; ++k) {
        O3DMI_REQUIRE(sizes[k] >= 0 && (sizes[k] == 0 || (positions_dev[k] &&
                                                          normals_dev[k])),
                      "fragment without positions or normals");
        frags[k] = {(const float*)positions_dev[k],
                    (const float*)normals_dev[k], sizes[k]};
    }
    std::vector<SlacEdge> ed((size_t)n_edges);
    for (int e = 0; e < n_edges; ++e) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        O3DMI_REQUIRE(i >= 0 && j >= 0 && i < n_fragments && j < n_fragments,
                      "node id out of range");
        O3DMI_REQUIRE(i != j, "an edge joins two different nodes");
        O3DMI_REQUIRE(corres_counts[e] >= 0 &&
                              (corres_counts[e] == 0 || corres_dev[e]),
                      "edge without correspondences buffer");
        // a lane reads its {a, b} pair as one 16-byte load
        O3DMI_REQUIRE(((uintptr_t)corres_dev[e] & 15) == 0,
                      "correspondence sets must be 16-byte aligned");
        ed[e].corres = (const int64_t*)corres_dev[e];
        ed[e].count = corres_counts[e];
        ed[e].i = i;
        ed[e].j = j;
        for (int k = 0; k < 12; ++k) {
            ed[e].Ti[k] = (float)poses[16 * i + k];
            ed[e].Tj[k] = (float)poses[16 * j + k];
        }
    }
    const int64_t n_tiles = SlacLayoutTiles(ed.data(), n_edges);
    hipStream_t s = (hipStream_t)stream;
    PoolScratch sc(s);
    SlacFragment* frags_dev = nullptr;
    SlacEdge* edges_dev = nullptr;
    double* partials = nullptr;
    int* bad = nullptr;
    int st;
    if ((st = sc.Alloc(&frags_dev, sizeof(SlacFragment) * frags.size())) ||
        (st = sc.Alloc(&edges_dev, sizeof(SlacEdge) * ed.size())) ||
        (st = sc.Alloc(&partials, sizeof(double) * kSlacSums *
                                          (size_t)(n_tiles > 0 ? n_tiles : 1))) ||
        (st = sc.Alloc(&bad, sizeof(int))))
        return st;
    O3DMI_HIP_CHECK(hipMemcpyAsync(frags_dev, frags.data(),
                                   sizeof(SlacFragment) * frags.size(),
                                   hipMemcpyHostToDevice, s));
    O3DMI_HIP_CHECK(hipMemcpyAsync(edges_dev, ed.data(),
                                   sizeof(SlacEdge) * ed.size(),
                                   hipMemcpyHostToDevice, s));
    O3DMI_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
    if ((st = SlacRigidTermsAsync(frags_dev, edges_dev, n_edges, n_tiles,
                                  threshold, partials, bad, sums_dev, s)))
        return st;
    int hbad = 0;
    O3DMI_HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int),
                                   hipMemcpyDeviceToHost, s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    O3DMI_REQUIRE(!hbad, "correspondence index out of range");
    return O3DMI_OK;
}

}  // extern "C"
