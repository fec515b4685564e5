// Fast Global Registration (o3d_mi355x.h, "Fast Global Registration"):
//   FgrNormalizeAsync     rule 1: the fixed sum tree, max norms, the two
//                         normalised float64 clouds;
//   o3dmi_fgr_tuple_test  rule 3: one lane per trial, pass flags, the prefix
//                         sum of scan.h, a compaction that stops at the cap;
//   o3dmi_fgr_optimize    rule 4, two forms that return the same bits:
//                         resident  one workgroup of 512 threads runs every
//                                   iteration in ONE launch; p and q stay in
//                                   registers, the only traffic between
//                                   iterations is 2 KiB of LDS;
//                         streamed  per iteration a partial-sums launch (a
//                                   tile per wave) and a one-wave finish
//                                   launch, all queued without a host wait.
// Both forms run the same device functions on the same tile tree: per tile of
// 256 correspondences lane l adds l, l + 64, l + 128, l + 192 in that order,
// the xor butterfly (32, 16, .., 1) adds the lanes, the tile sums are added in
// tile order. All arithmetic is float64.
#include "fgr.h"

#include <algorithm>
#include <cmath>

#include "ransac.h"
#include "scan.h"

namespace o3dmi {
namespace {

constexpr int kFgrWaves = kFgrBlock / 64;
constexpr int kWaveTiles = 2;  // tiles a wave of the resident form owns
static_assert(kFgrResident == (int64_t)kFgrWaves * kWaveTiles * kFgrTile,
              "resident capacity");
constexpr int kStreamBlock = 256;  // 4 waves = 4 tiles per workgroup

// Device state of the streamed form: {trans 16, par, failed solves, delta R 9,
// delta t 3}; the first 18 are o3dmi_fgr_optimize's out_dev layout.
constexpr int kStateTrans = 0, kStatePar = 16, kStateFailed = 17,
              kStateDelta = 18, kStateDoubles = 32;

struct LoopArgs {
    double par;
    double division_factor;
    double max_distance;
    int decrease_mu;
    int iterations;
};

template <typename P>
__device__ __forceinline__ void Load3(const void* base, int64_t row,
                                      double* out) {
    const P* p = (const P*)base + 3 * row;
    out[0] = (double)p[0];
    out[1] = (double)p[1];
    out[2] = (double)p[2];
}

__device__ __forceinline__ double WaveSum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- rule 1 -----------------------------------------------------------------
// One wave per tile of 256 rows; out {tiles, 3}.
template <typename P>
__global__ void __launch_bounds__(kStreamBlock)
TileSum3Kernel(const P* __restrict__ in, int64_t n, double* __restrict__ out) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t tiles = (n + kFgrTile - 1) / kFgrTile;
    const int64_t wave0 =
            (int64_t)blockIdx.x * (kStreamBlock / 64) + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * (kStreamBlock / 64);
    for (int64_t tile = wave0; tile < tiles; tile += stride) {
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t r = tile * kFgrTile + lane + 64 * k;
            double c[3] = {0.0, 0.0, 0.0};
            if (r < n) {
                c[0] = (double)in[3 * r + 0];
                c[1] = (double)in[3 * r + 1];
                c[2] = (double)in[3 * r + 2];
            }
            v[0] += c[0];
            v[1] += c[1];
            v[2] += c[2];
        }
        v[0] = WaveSum(v[0]);
        v[1] = WaveSum(v[1]);
        v[2] = WaveSum(v[2]);
        if (lane == 0) {
            out[3 * tile + 0] = v[0];
            out[3 * tile + 1] = v[1];
            out[3 * tile + 2] = v[2];
        }
    }
}

__global__ void MeansKernel(const double* __restrict__ total_s, int64_t ns,
                            const double* __restrict__ total_t, int64_t nt,
                            FgrNormWords* __restrict__ w) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int a = 0; a < 3; ++a) {
        w->mean[a] = total_s[a] / (double)ns;
        w->mean[3 + a] = total_t[a] / (double)nt;
    }
}

template <typename P>
__global__ void __launch_bounds__(kBlock)
MaxNormKernel(const P* __restrict__ pts, int64_t n,
              const double* __restrict__ mean,
              unsigned long long* __restrict__ max_bits) {
    const double m0 = mean[0], m1 = mean[1], m2 = mean[2];
    double best = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double x = (double)pts[3 * i + 0] - m0;
        const double y = (double)pts[3 * i + 1] - m1;
        const double z = (double)pts[3 * i + 2] - m2;
        const double d = sqrt((x * x + y * y) + z * z);
        if (d > best) best = d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o, 64);
        if (other > best) best = other;
    }
    // non-negative doubles order like their bit patterns
    if ((threadIdx.x & 63) == 0)
        atomicMax(max_bits, (unsigned long long)__double_as_longlong(best));
}

__global__ void ScaleKernel(FgrNormWords* __restrict__ w,
                            int use_absolute_scale) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double scale = 0.0;
    if (w->max_scale[0] > scale) scale = w->max_scale[0];
    if (w->max_scale[1] > scale) scale = w->max_scale[1];
    w->scale_global = use_absolute_scale ? 1.0 : scale;
    // rule 4: the optimisation starts at scale_global, not at scale_start
    w->par_start = w->scale_global;
}

template <typename P>
__global__ void __launch_bounds__(kBlock)
NormalizeKernel(const P* __restrict__ pts, int64_t n,
                const double* __restrict__ mean,
                const double* __restrict__ scale_global,
                double* __restrict__ out) {
    const double sg = *scale_global;
    const int64_t total = 3 * n;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total;
         x += (int64_t)gridDim.x * blockDim.x)
        out[x] = ((double)pts[x] - mean[x % 3]) / sg;
}

__global__ void SwapPairsKernel(int64_t* __restrict__ corres, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = corres[2 * i];
        corres[2 * i] = corres[2 * i + 1];
        corres[2 * i + 1] = a;
    }
}

// ---- rule 3 -----------------------------------------------------------------
__device__ __forceinline__ double Edge(const double* a, const double* b) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt((x * x + y * y) + z * z);
}

template <typename P>
__global__ void __launch_bounds__(kBlock)
TupleTrialKernel(uint64_t seed, int64_t first, int64_t count,
                 const void* __restrict__ src, int64_t ns,
                 const void* __restrict__ tgt, int64_t nt,
                 const int64_t* __restrict__ corres, int64_t ncorr,
                 double scale, int32_t* __restrict__ pass) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count;
         i += (int64_t)gridDim.x * blockDim.x) {
        double pi[3][3], pj[3][3];
        bool ok = true;
        for (int j = 0; j < 3; ++j) {
            const int64_t r =
                    (int64_t)RansacDraw(seed, first + i, j, (uint64_t)ncorr);
            const int64_t si = corres[2 * r], ti = corres[2 * r + 1];
            if (si < 0 || si >= ns || ti < 0 || ti >= nt) {
                ok = false;  // never read
                break;
            }
            Load3<P>(src, si, pi[j]);
            Load3<P>(tgt, ti, pj[j]);
        }
        if (ok) {
            const double li0 = Edge(pi[0], pi[1]), li1 = Edge(pi[1], pi[2]),
                         li2 = Edge(pi[2], pi[0]);
            const double lj0 = Edge(pj[0], pj[1]), lj1 = Edge(pj[1], pj[2]),
                         lj2 = Edge(pj[2], pj[0]);
            ok = (li0 * scale < lj0) && (lj0 < li0 / scale) &&
                 (li1 * scale < lj1) && (lj1 < li1 / scale) &&
                 (li2 * scale < lj2) && (lj2 < li2 / scale);
        }
        pass[i] = ok ? 1 : 0;
    }
}

// Passing trial i of the batch is tuple base + position[i]; tuples below the
// cap write their three pairs, the one that fills the cap also its trial count.
__global__ void __launch_bounds__(kBlock)
TupleCompactKernel(const int32_t* __restrict__ pass,
                   const int64_t* __restrict__ position, int64_t count,
                   uint64_t seed, int64_t first, int64_t base, int64_t cap,
                   const int64_t* __restrict__ corres, int64_t ncorr,
                   int64_t* __restrict__ tuples,
                   int64_t* __restrict__ trials_at_cap) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (!pass[i]) continue;
        const int64_t k = base + position[i];
        if (k >= cap) continue;
        for (int j = 0; j < 3; ++j) {
            const int64_t r =
                    (int64_t)RansacDraw(seed, first + i, j, (uint64_t)ncorr);
            tuples[2 * (3 * k + j)] = corres[2 * r];
            tuples[2 * (3 * k + j) + 1] = corres[2 * r + 1];
        }
        if (k == cap - 1) *trials_at_cap = first + i + 1;
    }
}

// ---- rule 4 -----------------------------------------------------------------
// The 16 sums. JTJ (symmetric) and JTr of the rule are
//   [ v0   v1   v2   0   -v8   v7 ]        [ v10 ]
//   [ v1   v3   v4   v8   0   -v6 ]        [ v11 ]
//   [ v2   v4   v5  -v7   v6   0  ]        [ v12 ]
//   [ 0    v8  -v7   v9   0    0  ]        [ v13 ]
//   [-v8   0    v6   0    v9   0  ]        [ v14 ]
//   [ v7  -v6   0    0    0    v9 ]        [ v15 ]
// (a sum of negated terms is the negated sum, bit for bit; a term that is zero
// in every row is left out, as adding +0.0 changes nothing).
// v += the terms of one correspondence. One that is not live has p = q = 0
// and s forced to 0: every term is then +-0.0, and adding it leaves v (never
// -0.0, as it starts at +0.0) as it is, like the +0.0 of the rule.
__device__ __forceinline__ void Accumulate(const double* p, const double* q,
                                           double par, bool live, double* v) {
    const double r0 = p[0] - q[0], r1 = p[1] - q[1], r2 = p[2] - q[2];
    const double temp = par / (((r0 * r0 + r1 * r1) + r2 * r2) + par);
    const double s = live ? temp * temp : 0.0;
    const double x = q[0], y = q[1], z = q[2];
    v[0] += (z * z) * s + (y * y) * s;
    v[1] += ((-y) * x) * s;
    v[2] += (z * (-x)) * s;
    v[3] += (z * z) * s + (x * x) * s;
    v[4] += ((-z) * y) * s;
    v[5] += (y * y) * s + (x * x) * s;
    v[6] += x * s;
    v[7] += y * s;
    v[8] += z * s;
    v[9] += s;
    v[10] += (z * r1) * s + ((-y) * r2) * s;
    v[11] += ((-z) * r0) * s + (x * r2) * s;
    v[12] += (y * r0) * s + ((-x) * r1) * s;
    v[13] += (-r0) * s;
    v[14] += (-r1) * s;
    v[15] += (-r2) * s;
}

__device__ __forceinline__ void MovePoint(const double* R, const double* t,
                                          double* q) {
    const double x = q[0], y = q[1], z = q[2];
    q[0] = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
    q[1] = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
    q[2] = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
}

// Lane c < 16 adds column c of tiles {n_tiles, 16} in tile order; every lane
// of the wave receives all 16 totals.
__device__ __forceinline__ void ColumnTotals(const double* tiles,
                                             int64_t n_tiles, int lane,
                                             double* tot) {
    double acc = 0.0;
    if (lane < kFgrSums)
        for (int64_t t = 0; t < n_tiles; ++t) acc += tiles[t * kFgrSums + lane];
#pragma unroll
    for (int c = 0; c < kFgrSums; ++c) tot[c] = __shfl(acc, c, 64);
}

// Solves -JTJ x = JTr by the Cholesky factor of JTJ (JTJ y = JTr, x = -y) and
// forms delta = Rz(x2) Ry(x1) Rx(x0), translation x[3..5]. false: a pivot was
// not positive and finite, or x is not finite; delta is then the identity.
__device__ __forceinline__ bool SolveStep(const double* v, double* R,
                                          double* t) {
    double A[6][6] = {{v[0], v[1], v[2], 0.0, -v[8], v[7]},
                      {v[1], v[3], v[4], v[8], 0.0, -v[6]},
                      {v[2], v[4], v[5], -v[7], v[6], 0.0},
                      {0.0, v[8], -v[7], v[9], 0.0, 0.0},
                      {-v[8], 0.0, v[6], 0.0, v[9], 0.0},
                      {v[7], -v[6], 0.0, 0.0, 0.0, v[9]}};
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !(d < INFINITY)) ok = false;
        const double l = sqrt(d);
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double a = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
            L[i][j] = a / l;
        }
    }
    double y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double a = v[10 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) a -= L[i][k] * y[k];
        y[i] = a / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double a = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) a -= L[k][i] * x[k];
        x[i] = a / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = -x[i];
        if (!(fabs(x[i]) < INFINITY)) ok = false;
    }
    if (!ok) {
        R[0] = 1; R[1] = 0; R[2] = 0;
        R[3] = 0; R[4] = 1; R[5] = 0;
        R[6] = 0; R[7] = 0; R[8] = 1;
        t[0] = 0; t[1] = 0; t[2] = 0;
        return false;
    }
    double sa, ca, sb, cb, sc, cc;
    sincos(x[0], &sa, &ca);
    sincos(x[1], &sb, &cb);
    sincos(x[2], &sc, &cc);
    R[0] = cc * cb;
    R[1] = (cc * sb) * sa - sc * ca;
    R[2] = (cc * sb) * ca + sc * sa;
    R[3] = sc * cb;
    R[4] = (sc * sb) * sa + cc * ca;
    R[5] = (sc * sb) * ca - cc * sa;
    R[6] = -sb;
    R[7] = cb * sa;
    R[8] = cb * ca;
    t[0] = x[3];
    t[1] = x[4];
    t[2] = x[5];
    return true;
}

// trans = delta * trans on the 3x4 part of the row-major 4x4 (the last row
// stays 0 0 0 1).
__device__ __forceinline__ void ComposeTrans(const double* R, const double* t,
                                             double* T) {
    double N[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            N[4 * i + j] = (R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j]) +
                           R[3 * i + 2] * T[8 + j];
        N[4 * i + 3] = ((R[3 * i] * T[3] + R[3 * i + 1] * T[7]) +
                        R[3 * i + 2] * T[11]) + t[i];
    }
    for (int e = 0; e < 12; ++e) T[e] = N[e];
}

__device__ __forceinline__ double NextPar(const LoopArgs& a, int itr,
                                          double par) {
    if (a.decrease_mu && itr % 4 == 0 && par > a.max_distance)
        par /= a.division_factor;
    return par;
}

// A pair outside [0, ns) x [0, nt) is never read and adds zeros.
__device__ __forceinline__ bool GatherPair(const double* __restrict__ src,
                                           int64_t ns,
                                           const double* __restrict__ tgt,
                                           int64_t nt,
                                           const int64_t* __restrict__ corres,
                                           int64_t n, int64_t c, double* p,
                                           double* q) {
    p[0] = p[1] = p[2] = 0.0;
    q[0] = q[1] = q[2] = 0.0;
    if (c >= n) return false;
    const int64_t si = corres[2 * c], ti = corres[2 * c + 1];
    if (si < 0 || si >= ns || ti < 0 || ti >= nt) return false;
    Load3<double>(src, si, p);
    Load3<double>(tgt, ti, q);
    return true;
}

// The resident form: wave w owns tiles w and w + 8 (n <= kFgrResident), lane l
// their correspondences l + 64 k. Every wave forms the totals and solves the
// step itself (the values are wave-uniform), so an iteration has ONE workgroup
// barrier and no broadcast; the tile sums alternate between two LDS buffers,
// which makes that barrier enough.
__global__ void __launch_bounds__(kFgrBlock)
ResidentKernel(const double* __restrict__ src, int64_t ns,
               const double* __restrict__ tgt, int64_t nt,
               const int64_t* __restrict__ corres, int64_t n, LoopArgs a,
               double* __restrict__ out) {
    __shared__ double s_tiles[2][kFgrWaves * kWaveTiles * kFgrSums];
    __shared__ double s_trans[12];  // thread 0's alone until the end
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int n_tiles = (int)((n + kFgrTile - 1) / kFgrTile);
    double p[kWaveTiles][4][3], q[kWaveTiles][4][3];
    bool live[kWaveTiles][4];
#pragma unroll
    for (int j = 0; j < kWaveTiles; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            live[j][k] = GatherPair(
                    src, ns, tgt, nt, corres, n,
                    (int64_t)(wave + kFgrWaves * j) * kFgrTile + lane + 64 * k,
                    p[j][k], q[j][k]);
    if (threadIdx.x == 0)
        for (int e = 0; e < 12; ++e) s_trans[e] = (e % 5 == 0) ? 1.0 : 0.0;
    double par = a.par;
    int failed = 0;
    for (int itr = 0; itr < a.iterations; ++itr) {
        double* tiles = s_tiles[itr & 1];
#pragma unroll
        for (int j = 0; j < kWaveTiles; ++j) {
            const int tile = wave + kFgrWaves * j;
            if (tile >= n_tiles) break;  // uniform over the wave
            double v[kFgrSums];
#pragma unroll
            for (int i = 0; i < kFgrSums; ++i) v[i] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Accumulate(p[j][k], q[j][k], par, live[j][k], v);
                // one correspondence at a time: the scheduler otherwise
                // interleaves all of them and runs out of registers
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < kFgrSums; ++i) v[i] = WaveSum(v[i]);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kFgrSums; ++i)
                    tiles[tile * kFgrSums + i] = v[i];
            }
        }
        __syncthreads();
        double tot[kFgrSums], R[9], t[3];
        ColumnTotals(tiles, n_tiles, lane, tot);
        if (!SolveStep(tot, R, t)) ++failed;
        if (threadIdx.x == 0) ComposeTrans(R, t, s_trans);
#pragma unroll
        for (int j = 0; j < kWaveTiles; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (live[j][k]) MovePoint(R, t, q[j][k]);
        par = NextPar(a, itr, par);
    }
    if (threadIdx.x == 0) {
        for (int e = 0; e < 12; ++e) out[e] = s_trans[e];
        out[12] = 0;
        out[13] = 0;
        out[14] = 0;
        out[15] = 1;
        out[kStatePar] = par;
        out[kStateFailed] = (double)failed;
    }
}

// ---- the streamed form ------------------------------------------------------
// pq {n, 6}: p and the current q of every correspondence; live {n}.
__global__ void __launch_bounds__(kBlock)
StreamGatherKernel(const double* __restrict__ src, int64_t ns,
                   const double* __restrict__ tgt, int64_t nt,
                   const int64_t* __restrict__ corres, int64_t n,
                   double par, double* __restrict__ pq,
                   uint8_t* __restrict__ live, double* __restrict__ state) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n;
         c += (int64_t)gridDim.x * blockDim.x) {
        double p[3], q[3];
        live[c] = GatherPair(src, ns, tgt, nt, corres, n, c, p, q) ? 1 : 0;
        for (int a = 0; a < 3; ++a) {
            pq[6 * c + a] = p[a];
            pq[6 * c + 3 + a] = q[a];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int e = 0; e < kStateDoubles; ++e) state[e] = 0.0;
        state[0] = state[5] = state[10] = state[15] = 1.0;
        state[kStatePar] = par;
    }
}

// Iteration itr: q is first moved by the delta of iteration itr - 1 (the move
// the resident form makes at the end of that iteration), then a wave adds
// its tile.
__global__ void __launch_bounds__(kStreamBlock)
StreamPartialKernel(double* __restrict__ pq, const uint8_t* __restrict__ live,
                    int64_t n, int itr, const double* __restrict__ state,
                    double* __restrict__ partials) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t tiles = (n + kFgrTile - 1) / kFgrTile;
    const int64_t wave0 =
            (int64_t)blockIdx.x * (kStreamBlock / 64) + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * (kStreamBlock / 64);
    const double par = state[kStatePar];
    double R[9], t[3];
    for (int e = 0; e < 9; ++e) R[e] = state[kStateDelta + e];
    for (int e = 0; e < 3; ++e) t[e] = state[kStateDelta + 9 + e];
    for (int64_t tile = wave0; tile < tiles; tile += stride) {
        double v[kFgrSums];
#pragma unroll
        for (int i = 0; i < kFgrSums; ++i) v[i] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = tile * kFgrTile + lane + 64 * k;
            double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
            const bool alive = c < n && live[c];
            if (alive) {
                for (int e = 0; e < 3; ++e) {
                    p[e] = pq[6 * c + e];
                    q[e] = pq[6 * c + 3 + e];
                }
                if (itr > 0) {
                    MovePoint(R, t, q);
                    for (int e = 0; e < 3; ++e) pq[6 * c + 3 + e] = q[e];
                }
            }
            Accumulate(p, q, par, alive, v);
        }
#pragma unroll
        for (int i = 0; i < kFgrSums; ++i) v[i] = WaveSum(v[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < kFgrSums; ++i)
                partials[tile * kFgrSums + i] = v[i];
        }
    }
}

// One wave: totals in tile order, the step, the state for the next launch.
__global__ void __launch_bounds__(64)
StreamFinishKernel(const double* __restrict__ partials, int64_t n_tiles,
                   int itr, LoopArgs a, double* __restrict__ state,
                   double* __restrict__ out) {
    const int lane = (int)threadIdx.x;
    double tot[kFgrSums], R[9], t[3];
    ColumnTotals(partials, n_tiles, lane, tot);
    const bool ok = SolveStep(tot, R, t);
    if (lane != 0) return;
    double T[12];
    for (int e = 0; e < 12; ++e) T[e] = state[kStateTrans + e];
    ComposeTrans(R, t, T);
    const double par = NextPar(a, itr, state[kStatePar]);
    const double failed = state[kStateFailed] + (ok ? 0.0 : 1.0);
    for (int e = 0; e < 12; ++e) state[kStateTrans + e] = T[e];
    state[kStatePar] = par;
    state[kStateFailed] = failed;
    for (int e = 0; e < 9; ++e) state[kStateDelta + e] = R[e];
    for (int e = 0; e < 3; ++e) state[kStateDelta + 9 + e] = t[e];
    if (itr == a.iterations - 1) {
        for (int e = 0; e < 12; ++e) out[e] = T[e];
        out[12] = 0;
        out[13] = 0;
        out[14] = 0;
        out[15] = 1;
        out[kStatePar] = par;
        out[kStateFailed] = failed;
    }
}

int64_t Tiles(int64_t n) { return (n + kFgrTile - 1) / kFgrTile; }

// Streamed scratch: state | partials {tiles, 16} | pq {n, 6} | live {n}.
size_t StreamScratchBytes(int64_t n) {
    return 8 * ((size_t)kStateDoubles + (size_t)Tiles(n) * kFgrSums +
                6 * (size_t)n) +
           (size_t)n;
}

template <typename P>
int SumTree(const P* in, int64_t n, double* levels, const double** total,
            hipStream_t s) {
    // first level from the point dtype, the rest over the tile sums
    int64_t tiles = Tiles(n);
    hipLaunchKernelGGL(TileSum3Kernel<P>,
                       dim3(GridFor(tiles, kStreamBlock / 64)),
                       dim3(kStreamBlock), 0, s, in, n, levels);
    const double* cur = levels;
    int64_t count = tiles;
    while (count > 1) {
        double* next = (double*)cur + 3 * count;
        tiles = Tiles(count);
        hipLaunchKernelGGL(TileSum3Kernel<double>,
                           dim3(GridFor(tiles, kStreamBlock / 64)),
                           dim3(kStreamBlock), 0, s, cur, count, next);
        cur = next;
        count = tiles;
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    *total = cur;
    return O3DMI_OK;
}

size_t TreeDoubles(int64_t n) {
    size_t d = 0;
    int64_t count = n;
    do {
        count = Tiles(count);
        d += 3 * (size_t)count;
    } while (count > 1);
    return d;
}

}  // namespace

size_t FgrNormScratchDoubles(int64_t ns, int64_t nt) {
    return TreeDoubles(ns) + TreeDoubles(nt);
}

int FgrNormalizeAsync(const void* source_dev, int64_t ns,
                      const void* target_dev, int64_t nt, int dtype,
                      int use_absolute_scale, double* scratch_dev,
                      FgrNormWords* w, double* source_out_dev,
                      double* target_out_dev, hipStream_t s) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(scratch_dev && w && source_out_dev && target_out_dev,
                  "null argument");
    const bool f64 = dtype == O3DMI_F64;
    const double* tot_s = nullptr;
    const double* tot_t = nullptr;
    double* lev_t = scratch_dev + TreeDoubles(ns);
    int st;
    if (f64) {
        if ((st = SumTree((const double*)source_dev, ns, scratch_dev, &tot_s,
                          s)) ||
            (st = SumTree((const double*)target_dev, nt, lev_t, &tot_t, s)))
            return st;
    } else {
        if ((st = SumTree((const float*)source_dev, ns, scratch_dev, &tot_s,
                          s)) ||
            (st = SumTree((const float*)target_dev, nt, lev_t, &tot_t, s)))
            return st;
    }
    hipLaunchKernelGGL(MeansKernel, dim3(1), dim3(64), 0, s, tot_s, ns, tot_t,
                       nt, w);
    unsigned long long* mx = (unsigned long long*)w->max_scale;
    const dim3 gs(GridFor(ns, kBlock)), gt(GridFor(nt, kBlock)), b(kBlock);
    if (f64) {
        hipLaunchKernelGGL(MaxNormKernel<double>, gs, b, 0, s,
                           (const double*)source_dev, ns, w->mean, mx);
        hipLaunchKernelGGL(MaxNormKernel<double>, gt, b, 0, s,
                           (const double*)target_dev, nt, w->mean + 3, mx + 1);
    } else {
        hipLaunchKernelGGL(MaxNormKernel<float>, gs, b, 0, s,
                           (const float*)source_dev, ns, w->mean, mx);
        hipLaunchKernelGGL(MaxNormKernel<float>, gt, b, 0, s,
                           (const float*)target_dev, nt, w->mean + 3, mx + 1);
    }
    hipLaunchKernelGGL(ScaleKernel, dim3(1), dim3(64), 0, s, w,
                       use_absolute_scale ? 1 : 0);
    const dim3 g3s(GridFor(3 * ns, kBlock)), g3t(GridFor(3 * nt, kBlock));
    if (f64) {
        hipLaunchKernelGGL(NormalizeKernel<double>, g3s, b, 0, s,
                           (const double*)source_dev, ns, w->mean,
                           &w->scale_global, source_out_dev);
        hipLaunchKernelGGL(NormalizeKernel<double>, g3t, b, 0, s,
                           (const double*)target_dev, nt, w->mean + 3,
                           &w->scale_global, target_out_dev);
    } else {
        hipLaunchKernelGGL(NormalizeKernel<float>, g3s, b, 0, s,
                           (const float*)source_dev, ns, w->mean,
                           &w->scale_global, source_out_dev);
        hipLaunchKernelGGL(NormalizeKernel<float>, g3t, b, 0, s,
                           (const float*)target_dev, nt, w->mean + 3,
                           &w->scale_global, target_out_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int FgrSwapPairsAsync(int64_t* corres_dev, int64_t n, hipStream_t s) {
    if (n <= 0) return O3DMI_OK;
    hipLaunchKernelGGL(SwapPairsKernel, dim3(GridFor(n, kBlock)), dim3(kBlock),
                       0, s, corres_dev, n);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

}  // namespace o3dmi

using namespace o3dmi;

extern "C" {

int o3dmi_internal_fgr_tuple_test(uint64_t seed, const void* source_dev,
                                  int64_t ns, const void* target_dev,
                                  int64_t nt, int dtype,
                                  const int64_t* corres_dev, int64_t n_corres,
                                  double tuple_scale,
                                  int64_t maximum_tuple_count,
                                  int64_t first_batch, int64_t* tuples_dev,
                                  int64_t* n_tuples, int64_t* n_trials,
                                  int64_t* n_batches, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "Only Float32 and Float64 point clouds are supported.");
    O3DMI_REQUIRE(n_tuples && n_trials, "null argument");
    O3DMI_REQUIRE(n_corres >= 0 && n_corres < (1ll << 56),
                  "correspondence count out of range");
    O3DMI_REQUIRE(maximum_tuple_count > 0, "maximum_tuple_count must be > 0");
    O3DMI_REQUIRE(std::isfinite(tuple_scale) && tuple_scale > 0,
                  "tuple_scale must be finite and > 0");
    O3DMI_REQUIRE(first_batch >= 1, "first_batch must be >= 1");
    *n_tuples = 0;
    *n_trials = 0;
    if (n_batches) *n_batches = 0;
    if (n_corres <= 2) return O3DMI_OK;  // FastGlobalRegistration.cpp:92-98
    O3DMI_REQUIRE(source_dev && target_dev && ns > 0 && nt > 0,
                  "Source and/or Target pointcloud is empty.");
    O3DMI_REQUIRE(corres_dev && tuples_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = 100 * n_corres;
    const int64_t cap = maximum_tuple_count;
    const int64_t bmax = std::min(total, kFgrMaxBatch);
    PoolScratch sc(s);
    int32_t* pass = nullptr;
    int64_t* position = nullptr;
    void* scan_tmp = nullptr;
    int64_t* words = nullptr;  // {passing trials of the batch, trials at cap}
    int st;
    if ((st = sc.Alloc(&pass, 4 * (size_t)bmax)) ||
        (st = sc.Alloc(&position, 8 * (size_t)bmax)) ||
        (st = sc.Alloc(&scan_tmp, ScanScratchBytes(bmax))) ||
        (st = sc.Alloc(&words, 16)))
        return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(words, 0, 16, s));
    int64_t batch = std::min(first_batch, bmax);
    int64_t kept = 0, batches = 0;
    int64_t h[2] = {0, 0};
    for (int64_t first = 0; first < total && kept < cap;) {
        const int64_t count = std::min(batch, total - first);
        const dim3 g(GridFor(count, kBlock)), b(kBlock);
        if (dtype == O3DMI_F64)
            hipLaunchKernelGGL(TupleTrialKernel<double>, g, b, 0, s, seed,
                               first, count, source_dev, ns, target_dev, nt,
                               corres_dev, n_corres, tuple_scale, pass);
        else
            hipLaunchKernelGGL(TupleTrialKernel<float>, g, b, 0, s, seed,
                               first, count, source_dev, ns, target_dev, nt,
                               corres_dev, n_corres, tuple_scale, pass);
        O3DMI_HIP_CHECK(hipGetLastError());
        if ((st = PrefixSumAsync(pass, count, false, position, words, scan_tmp,
                                 s)))
            return st;
        hipLaunchKernelGGL(TupleCompactKernel, g, b, 0, s, pass, position,
                           count, seed, first, kept, cap, corres_dev, n_corres,
                           tuples_dev, words + 1);
        O3DMI_HIP_CHECK(hipGetLastError());
        O3DMI_HIP_CHECK(hipMemcpyAsync(h, words, 16, hipMemcpyDeviceToHost, s));
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        ++batches;
        if (h[0] < 0 || h[0] > count) {
            SetLastError("fgr: passing-trial count out of range");
            return O3DMI_ERR_INTERNAL;
        }
        kept = std::min(cap, kept + h[0]);
        first += count;
        batch = std::min(2 * batch, bmax);
    }
    *n_tuples = kept;
    *n_trials = kept >= cap ? h[1] : total;
    if (n_batches) *n_batches = batches;
    return O3DMI_OK;
}

int o3dmi_fgr_tuple_test(uint64_t seed, const void* source_dev, int64_t ns,
                         const void* target_dev, int64_t nt, int dtype,
                         const int64_t* corres_dev, int64_t n_corres,
                         double tuple_scale, int64_t maximum_tuple_count,
                         int64_t* tuples_dev, int64_t* n_tuples,
                         int64_t* n_trials, o3dmi_stream_t stream) {
    return o3dmi_internal_fgr_tuple_test(
            seed, source_dev, ns, target_dev, nt, dtype, corres_dev, n_corres,
            tuple_scale, maximum_tuple_count, kFgrFirstBatch, tuples_dev,
            n_tuples, n_trials, nullptr, stream);
}

size_t o3dmi_fgr_optimize_scratch_bytes(int64_t n_corres) {
    if (n_corres <= kFgrResident) return 0;
    return StreamScratchBytes(n_corres);
}

int o3dmi_internal_fgr_optimize(const double* source_dev, int64_t ns,
                                const double* target_dev, int64_t nt,
                                const int64_t* corres_dev, int64_t n_corres,
                                double par, double division_factor,
                                int decrease_mu,
                                double maximum_correspondence_distance,
                                int iteration_number, int form,
                                void* scratch_dev, double* out_dev,
                                int* form_out, o3dmi_stream_t stream) {
    O3DMI_REQUIRE(out_dev != nullptr, "out is null");
    O3DMI_REQUIRE(n_corres >= 0 && iteration_number >= 0, "negative count");
    O3DMI_REQUIRE(std::isfinite(division_factor) && division_factor > 0 &&
                          std::isfinite(maximum_correspondence_distance) &&
                          maximum_correspondence_distance > 0,
                  "division_factor and maximum_correspondence_distance must "
                  "be finite and > 0");
    O3DMI_REQUIRE(form >= kFgrFormAuto && form <= kFgrFormStreamed,
                  "unknown form");
    O3DMI_REQUIRE(form != kFgrFormResident || n_corres <= kFgrResident,
                  "too many correspondences for the resident form");
    hipStream_t s = (hipStream_t)stream;
    LoopArgs a;
    a.par = par;
    a.division_factor = division_factor;
    a.max_distance = maximum_correspondence_distance;
    a.decrease_mu = decrease_mu ? 1 : 0;
    a.iterations = iteration_number;
    // FastGlobalRegistration.cpp:213; no iteration: the identity as well
    const bool none = n_corres < 10 || iteration_number == 0;
    if (none) {
        a.iterations = 0;
        hipLaunchKernelGGL(ResidentKernel, dim3(1), dim3(kFgrBlock), 0, s,
                           (const double*)nullptr, (int64_t)0,
                           (const double*)nullptr, (int64_t)0,
                           (const int64_t*)nullptr, (int64_t)0, a, out_dev);
        O3DMI_HIP_CHECK(hipGetLastError());
        if (form_out) *form_out = 0;
        return O3DMI_OK;
    }
    O3DMI_REQUIRE(source_dev && target_dev && corres_dev && ns > 0 && nt > 0,
                  "null argument");
    if (form == kFgrFormAuto)
        form = n_corres <= kFgrResident ? kFgrFormResident : kFgrFormStreamed;
    if (form_out) *form_out = form;
    if (form == kFgrFormResident) {
        hipLaunchKernelGGL(ResidentKernel, dim3(1), dim3(kFgrBlock), 0, s,
                           source_dev, ns, target_dev, nt, corres_dev,
                           n_corres, a, out_dev);
        O3DMI_HIP_CHECK(hipGetLastError());
        return O3DMI_OK;
    }
    O3DMI_REQUIRE(scratch_dev != nullptr, "scratch is null");
    const int64_t tiles = Tiles(n_corres);
    double* state = (double*)scratch_dev;
    double* partials = state + kStateDoubles;
    double* pq = partials + tiles * kFgrSums;
    uint8_t* live = (uint8_t*)(pq + 6 * n_corres);
    hipLaunchKernelGGL(StreamGatherKernel, dim3(GridFor(n_corres, kBlock)),
                       dim3(kBlock), 0, s, source_dev, ns, target_dev, nt,
                       corres_dev, n_corres, par, pq, live, state);
    const dim3 grid(GridFor(tiles, kStreamBlock / 64));
    for (int itr = 0; itr < iteration_number; ++itr) {
        hipLaunchKernelGGL(StreamPartialKernel, grid, dim3(kStreamBlock), 0, s,
                           pq, live, n_corres, itr, state, partials);
        hipLaunchKernelGGL(StreamFinishKernel, dim3(1), dim3(64), 0, s,
                           partials, tiles, itr, a, state, out_dev);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

size_t o3dmi_internal_fgr_stream_scratch_bytes(int64_t n_corres) {
    return n_corres > 0 ? StreamScratchBytes(n_corres) : 0;
}

int o3dmi_fgr_optimize(const double* source_dev, int64_t ns,
                       const double* target_dev, int64_t nt,
                       const int64_t* corres_dev, int64_t n_corres, double par,
                       double division_factor, int decrease_mu,
                       double maximum_correspondence_distance,
                       int iteration_number, void* scratch_dev,
                       double* out_dev, o3dmi_stream_t stream) {
    return o3dmi_internal_fgr_optimize(
            source_dev, ns, target_dev, nt, corres_dev, n_corres, par,
            division_factor, decrease_mu, maximum_correspondence_distance,
            iteration_number, kFgrFormAuto, scratch_dev, out_dev, nullptr,
            stream);
}

int64_t o3dmi_internal_fgr_resident_capacity(void) { return kFgrResident; }

}  // extern "C"
