// The non-rigid SLAC optimizer, the device half
// (t/pipelines/kernel/FillInLinearSystemImpl.h:156-524 FillInSLACAlignmentTerm
// and FillInSLACRegularizerTerm, t/pipelines/slac/FillInLinearSystemImpl.h:
// 102-236 their host side, slac/SLACOptimizer.cpp:288-367 the driver's solve).
//
// The reference adds, per correspondence, a 60 x 60 block J J^T, 60 values
// J r and r r with float32 atomics into a dense float32 matrix and solves it
// with a vendor gesv. Here the system is float64 and only its lower triangle
// exists. Per-pair terms are float32 in the reference's expressions, every
// sum is float64:
//
//   pose-pose  [[A, -A], [-A, A]], [b, -b], sum r r, count: the 29 sums of the
//              rigid kernel, a fixed tree per (edge, tile), a fixed order per
//              edge, the edges added in edge order by one workgroup.
//   grid-grid  rank one per node pair, (rho_k rho_l) u v^T: a workgroup stages
//              256 pairs in LDS, lane (k, l) of 16 x 16 walks them and keeps
//              the 3 x 3 block of its node pair in registers for as long as
//              consecutive pairs name the same two nodes, then adds it to the
//              matrix with float64 atomics (lower triangle only).
//   pose-grid  J_pose (rho_k u) and the grid rhs, the same walk keyed on one
//              node.
//
// The SPD solve is a blocked right-looking Cholesky (panel kSlacCholPanel):
// diagonal block in one workgroup, panel triangular solve one lane per row,
// trailing update in kSlacCholTile^2 LDS tiles; the forward substitution of
// the right-hand side rides along, the backward one is two launches a panel.
#include "common.h"
#include "control_grid_device.h"
#include "kabsch.h"
#include "reduce_sums.h"
#include "slac.h"
#include "slac_device.h"

namespace o3dmi {
namespace {

static_assert(kSlacBlock == kSumsBlock, "shared reduction geometry");
static_assert(kSlacBlock == 256, "lane (k, l) of 16 x 16 node pairs");

// ---- staging of kSlacBlock pairs -------------------------------------------
// rho[0..7] = ratios of p's corners, rho[8..15] = -(ratios of q's corners);
// rank[.] = the corner's unknown is 6 n_frags + 3 rank; rank[0] = -1: the pair
// contributes nothing. uv[0..2] = Cnormal_p, uv[3..5] = RjT Ri Cnormal_p;
// jp[0..5] = J w.r.t. Ti, jp[6] = r.
struct Stage {
    float rho[kSlacBlock][17];
    int rank[kSlacBlock][17];
    float uv[kSlacBlock][7];
    float jp[kSlacBlock][7];
};

__device__ __forceinline__ void StagePair(Stage& st, bool take,
                                          const float (&rho)[16],
                                          const int (&rank)[16],
                                          const float (&u)[3],
                                          const float (&v)[3],
                                          const float (&jp)[6], float r) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        st.rho[t][k] = rho[k];
        st.rank[t][k] = take ? rank[k] : -1;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        st.uv[t][a] = u[a];
        st.uv[t][3 + a] = v[a];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) st.jp[t][k] = jp[k];
    st.jp[t][6] = r;
}

// The grid entries of the staged pairs. i / j: the edge's fragments.
__device__ __forceinline__ void ScatterStaged(const Stage& st,
                                              const SlacSystem& sys, int i,
                                              int j) {
    const int64_t n = sys.n;
    const int64_t base = 6 * (int64_t)sys.n_frags;
    {
        // grid-grid: lane (k, l)
        const int k = threadIdx.x >> 4, l = threadIdx.x & 15;
        const int ko = k < 8 ? 0 : 3, lo = l < 8 ? 0 : 3;
        double acc[9];
        int kr = -1, kc = -1;
        auto flush = [&]() {
            if (kr < 0) return;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int64_t row = base + 3 * (int64_t)kr + a;
                    const int64_t col = base + 3 * (int64_t)kc + c;
                    if (row >= col)
                        atomicAdd(&sys.AtA[row * n + col], acc[3 * a + c]);
                }
        };
        for (int p = 0; p < kSlacBlock; ++p) {
            if (st.rank[p][0] < 0) continue;
            const int rk = st.rank[p][k], rl = st.rank[p][l];
            if (rk < rl) continue;
            if (rk != kr || rl != kc) {
                flush();
                kr = rk;
                kc = rl;
#pragma unroll
                for (int e = 0; e < 9; ++e) acc[e] = 0;
            }
            const float fk = st.rho[p][k], fl = st.rho[p][l];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ja = fk * st.uv[p][ko + a];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float jc = fl * st.uv[p][lo + c];
                    acc[3 * a + c] += (double)(ja * jc);
                }
            }
        }
        flush();
    }
    // pose-grid and the grid rhs: item (node k, axis a, u), u < 6 a pose
    // column of i (j's is the negation), u = 6 the rhs
    for (int w = threadIdx.x; w < 16 * 21; w += kSlacBlock) {
        const int k = w / 21, a = (w % 21) / 7, u = w % 7;
        const int ko = k < 8 ? 0 : 3;
        double acc = 0;
        int kr = -1;
        auto flush = [&]() {
            if (kr < 0) return;
            const int64_t row = base + 3 * (int64_t)kr + a;
            if (u < 6) {
                atomicAdd(&sys.AtA[row * n + 6 * i + u], acc);
                atomicAdd(&sys.AtA[row * n + 6 * j + u], -acc);
            } else {
                atomicAdd(&sys.Atb[row], acc);
            }
        };
        for (int p = 0; p < kSlacBlock; ++p) {
            if (st.rank[p][0] < 0) continue;
            const int rk = st.rank[p][k];
            if (rk != kr) {
                flush();
                kr = rk;
                acc = 0;
            }
            const float jg = st.rho[p][k] * st.uv[p][ko + a];
            acc += (double)(jg * st.jp[p][u]);
        }
        flush();
    }
}

// r and the pose Jacobian of one pair from the transformed rows
// (kernel/FillInLinearSystemImpl.h:238-253).
__device__ __forceinline__ float PairResidual(const float (&p)[3],
                                              const float (&q)[3],
                                              const float (&n)[3],
                                              float (&jp)[6]) {
    jp[0] = -q[2] * n[1] + q[1] * n[2];
    jp[1] = q[2] * n[0] - q[0] * n[2];
    jp[2] = -q[1] * n[0] + q[0] * n[1];
    jp[3] = n[0];
    jp[4] = n[1];
    jp[5] = n[2];
    return (p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1] + (p[2] - q[2]) * n[2];
}

// The edge of a tile: the last one whose first tile is not behind it.
__device__ __forceinline__ int EdgeOfTile(const SlacEdge* __restrict__ edges,
                                          int n_edges, int64_t tile) {
    int lo = 0, hi = n_edges - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (edges[mid].tile_first <= tile)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kSlacBlock)
NonrigidTermsKernel(const SlacGridFragment* __restrict__ frags,
                    const SlacEdge* __restrict__ edges, int n_edges,
                    const float* __restrict__ curr,
                    const int32_t* __restrict__ rank_of, int capacity,
                    float grid_size, float threshold, SlacSystem sys,
                    double* __restrict__ partials) {
    __shared__ Stage st;
    const int64_t tile = blockIdx.x;
    const SlacEdge& ed = edges[EdgeOfTile(edges, n_edges, tile)];
    const SlacGridFragment fi = frags[ed.i];
    const SlacGridFragment fj = frags[ed.j];
    const int64_t count = ed.count;
    const int64_t base = (tile - ed.tile_first) * kSlacTile + threadIdx.x;

    double A[kSlacSums];
#pragma unroll
    for (int k = 0; k < kSlacSums; ++k) A[k] = 0;
    bool out_of_range = false;
    int skipped = 0;
    for (int item = 0; item < kSlacItems; ++item) {
        const int64_t c = base + (int64_t)item * kSlacBlock;
        bool ok = c < count;
        int64_t a = 0, b = 0;
        if (ok) {
            a = ed.corres[2 * c];
            b = ed.corres[2 * c + 1];
            if (a < 0 || a >= fi.n || b < 0 || b >= fj.n) {
                out_of_range = true;
                ok = false;
            }
        }
        int idx[16], rank[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) idx[k] = rank[k] = 0;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                idx[k] = fi.corners[8 * a + k];
                idx[8 + k] = fj.corners[8 * b + k];
            }
            if (idx[0] < 0 || idx[8] < 0) {
                ++skipped;
                ok = false;
            }
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const bool in = idx[k] >= 0 && idx[k] < capacity;
                rank[k] = in ? rank_of[idx[k]] : -1;
                if (rank[k] < 0 ||
                    6 * (int64_t)sys.n_frags + 3 * (int64_t)rank[k] + 2 >=
                            sys.n) {
                    out_of_range = true;
                    ok = false;
                }
            }
        }
        float rho[16], u[3] = {0, 0, 0}, v[3] = {0, 0, 0}, jp[6], r = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) rho[k] = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) jp[k] = 0;
        bool take = false;
        float tp[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, tn[3] = {0, 0, 0};
        if (ok) {
            float p[3], q[3], nm[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                p[d] = fi.positions[3 * a + d];
                nm[d] = fi.normals[3 * a + d];
                q[d] = fj.positions[3 * b + d];
            }
            // the embedding of Parameterize, kept in registers
            Cell cp, cq;
            Quantize(p, grid_size, cp);
            Quantize(q, grid_size, cq);
            int ip[8], iq[8];
            float rp[8], rn[8], rq[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ip[k] = idx[k];
                iq[k] = idx[8 + k];
                rp[k] = VertexRatio(cp, k);
                rn[k] = NormalRatio(cp, k, nm);
                rq[k] = VertexRatio(cq, k);
                rho[k] = rp[k];
                rho[8 + k] = -rq[k];
            }
            // Deform
            float Cp[3], Cq[3], Cn[3];
            Interpolate(curr, ip, rp, Cp);
            Interpolate(curr, ip, rn, Cn);
            Interpolate(curr, iq, rq, Cq);
            const float len =
                    sqrtf((Cn[0] * Cn[0] + Cn[1] * Cn[1]) + Cn[2] * Cn[2]);
#pragma unroll
            for (int d = 0; d < 3; ++d) u[d] = Cn[d] / len;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                tp[d] = Row(ed.Ti + 4 * d, Cp[0], Cp[1], Cp[2]);
                tq[d] = Row(ed.Tj + 4 * d, Cq[0], Cq[1], Cq[2]);
                tn[d] = RotRow(ed.Ti + 4 * d, u[0], u[1], u[2]);
            }
            // Rj^T (Ri Cnormal_p)
#pragma unroll
            for (int d = 0; d < 3; ++d)
                v[d] = ed.Tj[d] * tn[0] + ed.Tj[4 + d] * tn[1] +
                       ed.Tj[8 + d] * tn[2];
            r = PairResidual(tp, tq, tn, jp);
            take = !(fabsf(r) > threshold);
        }
        AccumulateRigidPair(A, ok, tp[0], tp[1], tp[2], tq[0], tq[1], tq[2],
                            tn[0], tn[1], tn[2], threshold);
        StagePair(st, take, rho, rank, u, v, jp, r);
        __syncthreads();
        ScatterStaged(st, sys, ed.i, ed.j);
        __syncthreads();
    }
    if (out_of_range) atomicOr(&sys.counters[0], 1);
    if (skipped) atomicAdd(&sys.counters[1], skipped);
    BlockSumAndStore<kSlacSums>(A, partials);
}

// A raw node index of the seam that leaves the system.
__global__ void __launch_bounds__(kBlock)
SeamIndexCheckKernel(const int32_t* __restrict__ idx, int64_t n_idx,
                     const uint8_t* __restrict__ mask, int n_frags,
                     int64_t n_vars, int* __restrict__ bad) {
    bool any = false;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_idx;
         t += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[t]) continue;
        const int64_t v = idx[t];
        any = any || v < 0 || 6 * (int64_t)n_frags + 3 * v + 2 >= n_vars;
    }
    if (any) atomicOr(bad, 1);
}

// The reference's seam: everything comes gathered, deformed and transformed.
__global__ void __launch_bounds__(kSlacBlock)
NonrigidSeamTermsKernel(const float* __restrict__ Ti_Cps,
                        const float* __restrict__ Tj_Cqs,
                        const float* __restrict__ Cnormal_ps,
                        const float* __restrict__ Ri_Cnormal_ps,
                        const float* __restrict__ RjT_Ri_Cnormal_ps,
                        const int32_t* __restrict__ idx_ps,
                        const int32_t* __restrict__ idx_qs,
                        const float* __restrict__ ratio_ps,
                        const float* __restrict__ ratio_qs, int64_t count,
                        float threshold, int i, int j, SlacSystem sys,
                        double* __restrict__ partials) {
    __shared__ Stage st;
    double A[kSlacSums];
#pragma unroll
    for (int k = 0; k < kSlacSums; ++k) A[k] = 0;
    // SeamIndexCheckKernel ran first
    const bool bad = sys.counters[0] != 0;
    const int64_t base = (int64_t)blockIdx.x * kSlacTile + threadIdx.x;
    for (int item = 0; item < kSlacItems; ++item) {
        const int64_t c = base + (int64_t)item * kSlacBlock;
        const bool ok = c < count && !bad;
        float rho[16], u[3], v[3], jp[6], tp[3], tq[3], tn[3];
        int rank[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            rho[k] = ok ? ratio_ps[8 * c + k] : 0.f;
            rho[8 + k] = ok ? -ratio_qs[8 * c + k] : 0.f;
            rank[k] = ok ? idx_ps[8 * c + k] : 0;
            rank[8 + k] = ok ? idx_qs[8 * c + k] : 0;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            tp[d] = ok ? Ti_Cps[3 * c + d] : 0.f;
            tq[d] = ok ? Tj_Cqs[3 * c + d] : 0.f;
            tn[d] = ok ? Ri_Cnormal_ps[3 * c + d] : 0.f;
            u[d] = ok ? Cnormal_ps[3 * c + d] : 0.f;
            v[d] = ok ? RjT_Ri_Cnormal_ps[3 * c + d] : 0.f;
        }
        const float r = PairResidual(tp, tq, tn, jp);
        const bool take = ok && !(fabsf(r) > threshold);
        AccumulateRigidPair(A, ok, tp[0], tp[1], tp[2], tq[0], tq[1], tq[2],
                            tn[0], tn[1], tn[2], threshold);
        StagePair(st, take, rho, rank, u, v, jp, r);
        __syncthreads();
        ScatterStaged(st, sys, i, j);
        __syncthreads();
    }
    BlockSumAndStore<kSlacSums>(A, partials);
}

// One workgroup, the edges in order: every pose entry is a fixed-order sum.
__global__ void __launch_bounds__(kSlacBlock)
PoseBlocksKernel(const double* __restrict__ sums,
                 const SlacEdge* __restrict__ edges, int n_edges,
                 SlacSystem sys) {
    if (sys.counters[0]) return;
    const int t = threadIdx.x;
    const int64_t n = sys.n;
    for (int e = 0; e < n_edges; ++e) {
        const double* S = sums + (int64_t)e * kSlacSums;
        const int i = edges[e].i, j = edges[e].j;
        if (t < 144) {
            const int li = t / 12, lj = t % 12;
            const int u = li % 6, v = lj % 6;
            const int s = u >= v ? u * (u + 1) / 2 + v : v * (v + 1) / 2 + u;
            const double val = (li < 6) == (lj < 6) ? S[s] : -S[s];
            const int64_t row = (int64_t)(li < 6 ? i : j) * 6 + u;
            const int64_t col = (int64_t)(lj < 6 ? i : j) * 6 + v;
            if (row >= col) sys.AtA[row * n + col] += val;
        } else if (t < 156) {
            const int l = t - 144, u = l % 6;
            const double val = l < 6 ? S[21 + u] : -S[21 + u];
            sys.Atb[(int64_t)(l < 6 ? i : j) * 6 + u] += val;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock)
RankTableKernel(const int32_t* __restrict__ active, int64_t G, int capacity,
                int32_t* __restrict__ rank) {
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < G;
         g += (int64_t)gridDim.x * blockDim.x) {
        const int idx = active[g];
        if (idx >= 0 && idx < capacity) rank[idx] = (int)g;
    }
}

__global__ void __launch_bounds__(kBlock)
GridCornersKernel(HashView hv, const float* __restrict__ points, int64_t n,
                  float grid_size, int32_t* __restrict__ corners) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        Cell c;
        int idx[8];
        const bool ok = Quantize(points + 3 * i, grid_size, c) &&
                        FindCorners(hv, c, idx);
#pragma unroll
        for (int k = 0; k < 8; ++k) corners[8 * i + k] = ok ? idx[k] : -1;
    }
}

// ---- regularizer -----------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
RegularizerKernel(const int32_t* __restrict__ active,
                  const int32_t* __restrict__ nb_idx,
                  const uint8_t* __restrict__ nb_mask, int64_t G,
                  const float* __restrict__ init,
                  const float* __restrict__ curr,
                  const int32_t* __restrict__ rank_of, int64_t n_rows,
                  float weight, int anchor_idx, SlacSystem sys,
                  double* __restrict__ node_residual) {
    const int64_t n = sys.n;
    const int64_t base = 6 * (int64_t)sys.n_frags;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < G;
         g += (int64_t)gridDim.x * blockDim.x) {
        node_residual[g] = 0;
        if (sys.counters[0]) continue;
        const int idx_i = active[g];
        bool bad = idx_i < 0 || idx_i >= n_rows;
        int idx_k[6];
        bool mask[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            mask[k] = nb_mask[6 * g + k] != 0;
            idx_k[k] = mask[k] ? nb_idx[6 * g + k] : 0;
            bad = bad || idx_k[k] < 0 || idx_k[k] >= n_rows;
        }
        int64_t off_i = -1, off_k[6];
        if (!bad) {
            const int ri = rank_of ? rank_of[idx_i] : idx_i;
            bad = ri < 0 || base + 3 * (int64_t)ri + 2 >= n;
            off_i = base + 3 * (int64_t)ri;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int rk = rank_of ? rank_of[idx_k[k]] : idx_k[k];
                if (mask[k])
                    bad = bad || rk < 0 || base + 3 * (int64_t)rk + 2 >= n;
                off_k[k] = base + 3 * (int64_t)rk;
            }
        }
        if (bad) {
            atomicOr(&sys.counters[0], 1);
            continue;
        }
        // cov = sum diff_init diff_curr^T over the masked neighbours
        float cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        float di[6][3], dc[6][3];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                di[k][a] = init[3 * (int64_t)idx_i + a] -
                           init[3 * (int64_t)idx_k[k] + a];
                dc[k][a] = curr[3 * (int64_t)idx_i + a] -
                           curr[3 * (int64_t)idx_k[k] + a];
            }
            if (!mask[k]) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) cov[a][b] += di[k][a] * dc[k][b];
            ++cnt;
        }
        if (cnt < 3) continue;
        // curr = R init: the fit's cross-covariance has the target (curr) in
        // its rows; det(R) = +1 is KabschJacobi's sign rule
        double Gm[3][3], R9[9], t3[3], s0, s1;
        const double zero[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Gm[a][b] = (double)cov[b][a];
        KabschJacobi(Gm, zero, zero, R9, t3, &s0, &s1);
        float R[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                R[a][b] = idx_i == anchor_idx ? (a == b ? 1.f : 0.f)
                                              : (float)R9[3 * a + b];
        double res = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (!mask[k]) continue;
            float lr[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                lr[a] = dc[k][a] - (R[a][0] * di[k][0] + R[a][1] * di[k][1] +
                                    R[a][2] * di[k][2]);
            res += (double)(weight *
                            (lr[0] * lr[0] + lr[1] * lr[1] + lr[2] * lr[2]));
            const int64_t oi = off_i, ok = off_k[k];
            const int64_t hi = oi > ok ? oi : ok, lo = oi > ok ? ok : oi;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicAdd(&sys.AtA[(oi + a) * n + oi + a], (double)weight);
                atomicAdd(&sys.AtA[(ok + a) * n + ok + a], (double)weight);
                // the reference writes (i, k) and (k, i); one is below the
                // diagonal
                atomicAdd(&sys.AtA[(hi + a) * n + lo + a], -(double)weight);
                const float wr = weight * lr[a];
                atomicAdd(&sys.Atb[oi + a], (double)wr);
                atomicAdd(&sys.Atb[ok + a], -(double)wr);
            }
        }
        node_residual[g] = res;
    }
}

// out[0] = sum of v[0..n) in a fixed order, one workgroup.
__global__ void __launch_bounds__(kSumsBlock)
FixedSumKernel(const double* __restrict__ v, int64_t n,
               double* __restrict__ out) {
    double A[1] = {0};
    for (int64_t i = threadIdx.x; i < n; i += kSumsBlock) A[0] += v[i];
    BlockSumAndStore<1>(A, out);
}

__global__ void __launch_bounds__(kBlock)
SeamFinishKernel(SlacSystem sys, const double* __restrict__ residual,
                 float* __restrict__ AtA_out, float* __restrict__ Atb_out,
                 float* __restrict__ residual_out) {
    if (sys.counters[0]) return;
    const int64_t n = sys.n;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n * n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n, c = t % n;
        const double v = r >= c ? sys.AtA[r * n + c] : sys.AtA[c * n + r];
        if (v != 0) AtA_out[t] += (float)v;
        if (t < n) {
            const double b = sys.Atb[t];
            if (b != 0) Atb_out[t] += (float)b;
        }
        if (t == 0 && residual[0] != 0) residual_out[0] += (float)residual[0];
    }
}

__global__ void __launch_bounds__(kBlock)
PrepareKernel(SlacSystem sys) {
    if (threadIdx.x < 6 && threadIdx.x < sys.n)
        sys.AtA[(int64_t)threadIdx.x * sys.n + threadIdx.x] = 1.0;
}

// Rows / columns row0 .. row0 + 2 of the lower triangle become the identity
// and their rhs 0: the node keeps its position.
__global__ void __launch_bounds__(kBlock)
PinNodeKernel(SlacSystem sys, int64_t row0) {
    const int64_t n = sys.n;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int64_t r = row0 + a;
            if (t <= r)
                sys.AtA[r * n + t] = t == r ? 1.0 : 0.0;
            else
                sys.AtA[t * n + r] = 0.0;
            if (t == 0) sys.Atb[r] = 0.0;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
NegateKernel(double* __restrict__ x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        x[i] = -x[i];
}

__global__ void __launch_bounds__(kBlock)
UpdateGridKernel(const int32_t* __restrict__ active, int64_t G,
                 const double* __restrict__ x, float* __restrict__ curr) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < 3 * G;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = t / 3;
        const int a = (int)(t % 3);
        const int64_t at = 3 * (int64_t)active[g] + a;
        curr[at] = curr[at] + (float)x[t];
    }
}

// ---- blocked Cholesky ------------------------------------------------------
constexpr int kNB = kSlacCholPanel;
constexpr int kTile = kSlacCholTile;
static_assert(kTile == 64 && kNB <= 64, "CholUpdateKernel's 4 x 4 micro tile");
// CholPanelKernel keeps a row per lane in LDS: kNB x kBlock doubles beside L
// and y, 74 KB at kNB = 32. gfx950 has 160 KB a CU, so two workgroups fit.
static_assert(sizeof(double) * (kNB * kBlock + kNB * (kNB + 1) + kNB) <=
                      80 * 1024,
              "CholPanelKernel: two workgroups a CU need <= 80 KB of LDS each");

// L11 L11^T = A[k0.., k0..] (nb x nb) in place, and y = L11^-1 b[k0..].
__global__ void __launch_bounds__(kBlock)
CholDiagKernel(double* __restrict__ A, double* __restrict__ b, int64_t n,
               int64_t k0, int nb, int* __restrict__ flag) {
    __shared__ double T[kNB][kNB + 1];
    __shared__ int fail;
    if (*flag) return;
    const int t = threadIdx.x;
    if (t == 0) fail = 0;
    for (int e = t; e < kNB * kNB; e += kBlock) {
        const int r = e / kNB, c = e % kNB;
        T[r][c] = (r < nb && c <= r) ? A[(k0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
        if (t == 0) {
            const double d = T[k][k];
            if (!(d > 0) || !isfinite(d))
                fail = 1;
            else
                T[k][k] = sqrt(d);
        }
        __syncthreads();
        if (fail) {
            if (t == 0) *flag = 1;
            return;
        }
        if (t > k && t < nb) T[t][k] /= T[k][k];
        __syncthreads();
        for (int e = t; e < kNB * kNB; e += kBlock) {
            const int r = e / kNB, c = e % kNB;
            if (c > k && c <= r && r < nb) T[r][c] -= T[r][k] * T[c][k];
        }
        __syncthreads();
    }
    for (int e = t; e < kNB * kNB; e += kBlock) {
        const int r = e / kNB, c = e % kNB;
        if (r < nb && c <= r) A[(k0 + r) * n + k0 + c] = T[r][c];
    }
    if (t == 0) {
        for (int k = 0; k < nb; ++k) {
            double v = b[k0 + k];
            for (int m = 0; m < k; ++m) v -= T[k][m] * b[k0 + m];
            b[k0 + k] = v / T[k][k];
        }
    }
}

// Rows r >= k0 + nb: L[r, k0..] = A[r, k0..] L11^-T and b[r] -= L[r, k0..] y.
__global__ void __launch_bounds__(kBlock)
CholPanelKernel(double* __restrict__ A, double* __restrict__ b, int64_t n,
                int64_t k0, int nb, const int* __restrict__ flag) {
    __shared__ double L[kNB][kNB + 1];
    __shared__ double y[kNB];
    __shared__ double xs[kNB][kBlock];
    if (*flag) return;
    for (int e = threadIdx.x; e < kNB * kNB; e += kBlock) {
        const int r = e / kNB, c = e % kNB;
        L[r][c] = (r < nb && c <= r) ? A[(k0 + r) * n + k0 + c]
                                     : (r == c ? 1.0 : 0.0);
    }
    if (threadIdx.x < kNB)
        y[threadIdx.x] = threadIdx.x < nb ? b[k0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int64_t r = k0 + nb + blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (r >= n) return;
    // the row lives in LDS (lane-contiguous): a register array would have to
    // be indexed by the loop counters
    const int t = threadIdx.x;
    for (int k = 0; k < nb; ++k) xs[k][t] = A[r * n + k0 + k];
    double dot = 0;
#pragma unroll 1
    for (int k = 0; k < nb; ++k) {
        double v = xs[k][t];
        for (int m = 0; m < k; ++m) v = fma(-xs[m][t], L[k][m], v);
        v = v / L[k][k];
        xs[k][t] = v;
        dot = fma(v, y[k], dot);
    }
    for (int k = 0; k < nb; ++k) A[r * n + k0 + k] = xs[k][t];
    b[r] -= dot;
}

// A[r][c] -= sum_k L[r][k0 + k] L[c][k0 + k] for t0 <= c <= r < n.
__global__ void __launch_bounds__(kBlock)
CholUpdateKernel(double* __restrict__ A, int64_t n, int64_t k0, int nb,
                 int64_t t0, const int* __restrict__ flag) {
    if (blockIdx.x > blockIdx.y) return;  // x: column tile, y: row tile
    __shared__ double Pr[kTile][kNB + 1];
    __shared__ double Pc[kTile][kNB + 1];
    if (*flag) return;
    const int64_t r0 = t0 + (int64_t)blockIdx.y * kTile;
    const int64_t c0 = t0 + (int64_t)blockIdx.x * kTile;
    for (int e = threadIdx.x; e < kTile * kNB; e += kBlock) {
        const int rr = e / kNB, k = e % kNB;
        Pr[rr][k] = (r0 + rr < n && k < nb) ? A[(r0 + rr) * n + k0 + k] : 0.0;
        Pc[rr][k] = (c0 + rr < n && k < nb) ? A[(c0 + rr) * n + k0 + k] : 0.0;
    }
    __syncthreads();
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0;
#pragma unroll 8
    for (int k = 0; k < kNB; ++k) {
        double pr[4], pc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            pr[a] = Pr[ty + 16 * a][k];
            pc[a] = Pc[tx + 16 * a][k];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = fma(pr[a], pc[c], acc[a][c]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t r = r0 + ty + 16 * a, cc = c0 + tx + 16 * c;
            if (r < n && cc <= r) A[r * n + cc] -= acc[a][c];
        }
}

// x[k0..] = L11^-T y[k0..], one workgroup.
__global__ void __launch_bounds__(kBlock)
CholBackDiagKernel(const double* __restrict__ A, double* __restrict__ b,
                   int64_t n, int64_t k0, int nb,
                   const int* __restrict__ flag) {
    __shared__ double L[kNB][kNB + 1];
    if (*flag) return;
    for (int e = threadIdx.x; e < kNB * kNB; e += kBlock) {
        const int r = e / kNB, c = e % kNB;
        L[r][c] = (r < nb && c <= r) ? A[(k0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = nb - 1; k >= 0; --k) {
            double v = b[k0 + k];
            for (int m = k + 1; m < nb; ++m) v -= L[m][k] * b[k0 + m];
            b[k0 + k] = v / L[k][k];
        }
    }
}

// y[r] -= sum_k L[k0 + k][r] x[k0 + k] for r < k0.
__global__ void __launch_bounds__(kBlock)
CholBackUpdateKernel(const double* __restrict__ A, double* __restrict__ b,
                     int64_t n, int64_t k0, int nb,
                     const int* __restrict__ flag) {
    __shared__ double x[kNB];
    if (*flag) return;
    if (threadIdx.x < kNB)
        x[threadIdx.x] = threadIdx.x < nb ? b[k0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (r >= k0) return;
    double dot = 0;
    for (int k = 0; k < nb; ++k) dot = fma(A[(k0 + k) * n + r], x[k], dot);
    b[r] -= dot;
}

}  // namespace

int SlacRankTableAsync(const int32_t* active_dev, int64_t G, int capacity,
                       int32_t* rank_dev, hipStream_t s) {
    O3DMI_HIP_CHECK(hipMemsetAsync(rank_dev, 0xFF,
                                   sizeof(int32_t) * (size_t)capacity, s));
    if (G <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(RankTableKernel, dim3(GridFor(G, kBlock)), dim3(kBlock),
                       0, s, active_dev, G, capacity, rank_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacGridCornersAsync(const HashView& hv, const float* points_dev,
                         int64_t n, float grid_size, int32_t* corners_dev,
                         hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(GridCornersKernel, dim3(GridFor(n, kBlock)),
                       dim3(kBlock), 0, s, hv, points_dev, n, grid_size,
                       corners_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacNonrigidTermsAsync(const SlacGridFragment* frags_dev,
                           const SlacEdge* edges_dev, int n_edges,
                           int64_t n_tiles, const float* curr_dev,
                           const int32_t* rank_dev, int capacity,
                           float grid_size, float threshold, SlacSystem sys,
                           double* partials_dev, hipStream_t s) {
    if (n_edges <= 0 || n_tiles <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(n_tiles < (1ll << 31), "slac: too many correspondences");
    hipLaunchKernelGGL(NonrigidTermsKernel, dim3((unsigned)n_tiles),
                       dim3(kSlacBlock), 0, s, frags_dev, edges_dev, n_edges,
                       curr_dev, rank_dev, capacity, grid_size, threshold, sys,
                       partials_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacPoseBlocksAsync(const double* sums_dev, const SlacEdge* edges_dev,
                        int n_edges, SlacSystem sys, hipStream_t s) {
    if (n_edges <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(PoseBlocksKernel, dim3(1), dim3(kSlacBlock), 0, s,
                       sums_dev, edges_dev, n_edges, sys);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacSeamIndexCheckAsync(const int32_t* idx_dev, int64_t n_idx,
                            const uint8_t* mask_dev, SlacSystem sys,
                            hipStream_t s) {
    if (n_idx <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(SeamIndexCheckKernel, dim3(GridFor(n_idx, kBlock)),
                       dim3(kBlock), 0, s, idx_dev, n_idx, mask_dev,
                       sys.n_frags, sys.n, sys.counters);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacNonrigidSeamTermsAsync(const float* Ti_Cps, const float* Tj_Cqs,
                               const float* Cnormal_ps,
                               const float* Ri_Cnormal_ps,
                               const float* RjT_Ri_Cnormal_ps,
                               const int32_t* idx_ps, const int32_t* idx_qs,
                               const float* ratio_ps, const float* ratio_qs,
                               int64_t count, float threshold, int i, int j,
                               SlacSystem sys, double* partials_dev,
                               hipStream_t s) {
    const int64_t tiles = SlacTiles(count);
    if (tiles <= 0) return O3DMI_OK;
    O3DMI_REQUIRE(tiles < (1ll << 31), "slac: too many correspondences");
    int st;
    if ((st = SlacSeamIndexCheckAsync(idx_ps, 8 * count, nullptr, sys, s)) ||
        (st = SlacSeamIndexCheckAsync(idx_qs, 8 * count, nullptr, sys, s)))
        return st;
    hipLaunchKernelGGL(NonrigidSeamTermsKernel, dim3((unsigned)tiles),
                       dim3(kSlacBlock), 0, s, Ti_Cps, Tj_Cqs, Cnormal_ps,
                       Ri_Cnormal_ps, RjT_Ri_Cnormal_ps, idx_ps, idx_qs,
                       ratio_ps, ratio_qs, count, threshold, i, j, sys,
                       partials_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacRegularizerAsync(const int32_t* active_dev, const int32_t* nb_idx_dev,
                         const uint8_t* nb_mask_dev, int64_t G,
                         const float* init_dev, const float* curr_dev,
                         const int32_t* rank_dev, int64_t n_rows, float weight,
                         int anchor_idx, SlacSystem sys,
                         double* node_residual_dev, double* residual_dev,
                         hipStream_t s) {
    if (G > 0)
        hipLaunchKernelGGL(RegularizerKernel, dim3(GridFor(G, kBlock)),
                           dim3(kBlock), 0, s, active_dev, nb_idx_dev,
                           nb_mask_dev, G, init_dev, curr_dev, rank_dev,
                           n_rows, weight, anchor_idx, sys, node_residual_dev);
    hipLaunchKernelGGL(FixedSumKernel, dim3(1), dim3(kSumsBlock), 0, s,
                       node_residual_dev, G > 0 ? G : 0, residual_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacSeamFinishAsync(SlacSystem sys, const double* residual_dev,
                        float* AtA_out, float* Atb_out, float* residual_out,
                        hipStream_t s) {
    hipLaunchKernelGGL(SeamFinishKernel, dim3(GridFor(sys.n * sys.n, kBlock)),
                       dim3(kBlock), 0, s, sys, residual_dev, AtA_out, Atb_out,
                       residual_out);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacPrepareSystemAsync(SlacSystem sys, hipStream_t s) {
    hipLaunchKernelGGL(PrepareKernel, dim3(1), dim3(kBlock), 0, s, sys);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacPinNodeAsync(SlacSystem sys, int64_t row0, hipStream_t s) {
    O3DMI_REQUIRE(row0 >= 0 && row0 + 2 < sys.n, "slac: pinned node outside");
    hipLaunchKernelGGL(PinNodeKernel, dim3(GridFor(sys.n, kBlock)),
                       dim3(kBlock), 0, s, sys, row0);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacNegateAsync(double* x_dev, int64_t n, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(NegateKernel, dim3(GridFor(n, kBlock)), dim3(kBlock), 0,
                       s, x_dev, n);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacUpdateGridAsync(const int32_t* active_dev, int64_t G,
                        const double* x_dev, float* curr_dev, hipStream_t s) {
    if (G <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(UpdateGridKernel, dim3(GridFor(3 * G, kBlock)),
                       dim3(kBlock), 0, s, active_dev, G, x_dev, curr_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int SlacSolveSpdAsync(double* A, double* b, int64_t n, int* flag,
                      hipStream_t s) {
    for (int64_t k0 = 0; k0 < n; k0 += kNB) {
        const int nb = (int)(n - k0 < kNB ? n - k0 : kNB);
        hipLaunchKernelGGL(CholDiagKernel, dim3(1), dim3(kBlock), 0, s, A, b,
                           n, k0, nb, flag);
        const int64_t t0 = k0 + nb;
        if (t0 >= n) break;
        const int64_t rest = n - t0;
        hipLaunchKernelGGL(CholPanelKernel,
                           dim3((unsigned)((rest + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, s, A, b, n, k0, nb, flag);
        const unsigned tiles = (unsigned)((rest + kTile - 1) / kTile);
        hipLaunchKernelGGL(CholUpdateKernel, dim3(tiles, tiles), dim3(kBlock),
                           0, s, A, n, k0, nb, t0, flag);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    const int64_t last = n > 0 ? ((n - 1) / kNB) * kNB : 0;
    for (int64_t k0 = last; k0 >= 0 && n > 0; k0 -= kNB) {
        const int nb = (int)(n - k0 < kNB ? n - k0 : kNB);
        hipLaunchKernelGGL(CholBackDiagKernel, dim3(1), dim3(kBlock), 0, s, A,
                           b, n, k0, nb, flag);
        if (k0 > 0)
            hipLaunchKernelGGL(CholBackUpdateKernel,
                               dim3((unsigned)((k0 + kBlock - 1) / kBlock)),
                               dim3(kBlock), 0, s, A, b, n, k0, nb, flag);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi
