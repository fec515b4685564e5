// The wave-per-query neighbour search as a device header: GatherCells plus a
// Sink, WaveTopK, and the Out policy of KnnSearchKernel / HybridSearchKernel,
// with the host steps of a KNN search (KnnSearchRun). Included by .hip files
// only: nns.hip for the public searches, and every operator that does
// something with each point's neighbour list (pointcloud_segment.hip,
// pointcloud_smooth.hip, pointcloud_filter.hip, pointcloud_metrics.hip) for
// its own sinks, output policies and launchers. Kernels and device code sit in
// an unnamed namespace: every unit gets its own copy. The index itself and
// what the host drivers need are in nns.h.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "nns.h"

namespace o3dmi {

// ---- host steps of a KNN search, defined in nns.hip --------------------------
// Everything a KnnSearch call owns; released on every exit path (the index
// destructor drains the device first, so the pooled scratch is idle by then).
struct KnnResources {
    unsigned long long* box = nullptr;  // [0..2] min keys, [3..5] max, [6] count
    int* retry = nullptr;               // [0] = count, [1..q] = query ids
    std::vector<o3dmi_nns*> levels;     // finest first
    ~KnnResources();
    int AddLevel(const void* points, int64_t n, int dtype, double cell,
                 hipStream_t s);
    void DropLevels();
};

// What steps 1 and 2 of a KNN search leave behind: the dataset's bounding box
// and the cell size of the finest level (res.levels[0]).
struct KnnPlan {
    double lo[3], ext[3];
    double emax;    // largest extent (1 for a cloud of no extent)
    double h;       // cell edge of the finest level
    double target;  // points per occupied cell aimed at
    bool single;    // one level already spans the cloud
};

// Steps 1 and 2 of KnnSearchRun for rows of k neighbours.
int KnnPlanFinest(const void* points_dev, int64_t n, int dtype, int k,
                  KnnResources& res, KnnPlan& plan, hipStream_t s);

// The retry list of the first pass ([0] = count, [1..q] = ids); none when one
// level spans the cloud.
int KnnAllocRetry(KnnResources& res, const KnnPlan& plan, int64_t q,
                  hipStream_t s);

// Occupied cell box of level `lv` from the dataset's bounding box.
void KnnCellBox(const o3dmi_nns* lv, const KnnPlan& plan, long long* cmin,
                long long* cmax);

// Length of the retry list once the first pass has run.
int KnnRetryCount(const KnnResources& res, const KnnPlan& plan, int* n_retry,
                  hipStream_t s);

namespace {

constexpr int kMaxKnn = 64;  // general-k searches: k <= one wave

// ---- general-k searches: one wave per query --------------------------------
// A lane-per-query search keeps a sorted k-list per lane and pays a dependent
// chain of ~2 loads per neighbour cell plus an insertion shift per candidate,
// with the 64 lanes of a wave diverging on every one of them (2.7 ms for
// 100 k queries at k = 30 even with the lists in LDS). Here a wave serves one
// query:
//   * lane c looks up neighbour cell c (bucket bounds), a wave prefix sum
//     turns the per-cell counts into one candidate range, and lane t fetches
//     candidate t (owner cell found by a 6-step search over the prefix) --
//     two memory round trips for any number of cells. A record is accepted
//     only if its own cell is the cell it was fetched for, so records that
//     merely share the bucket (hash collisions) never show up twice;
//   * accepted candidates are compacted into an LDS buffer of the wave;
//   * the k best are found by rank counting: candidate p reads every buffered
//     candidate q (a broadcast LDS read) and counts those that sort before it
//     by (d2, index); rank < k means "rank-th neighbour". No dependent chain,
//     no divergence, ties impossible because indices are unique.
constexpr int kCoopCap = 512;    // buffered candidates per wave before a merge
constexpr int kCoopBlock = 256;  // 4 waves = 4 queries in flight per workgroup
constexpr int kNoIndex = 0x7fffffff;

template <typename T>
__device__ __forceinline__ T InfOf() { return (T)INFINITY; }

template <typename T>
__device__ __forceinline__ bool PairLess(T ad, int ai, T bd, int bi) {
    return ad < bd || (ad == bd && ai < bi);
}

__device__ __forceinline__ void WaveLdsSync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// v = the sum / the minimum of v over the 64 lanes, on every lane (butterfly
// over lane distances 32, 16, ..., 1). Statements, not functions, like
// O3DMI_GATHER_BALL below and for its reason.
#define O3DMI_WAVE_SUM(v) \
    _Pragma("unroll") for (int m_ = 32; m_ > 0; m_ >>= 1) v += __shfl_xor(v, m_)
#define O3DMI_WAVE_MIN(v)                                 \
    _Pragma("unroll") for (int m_ = 32; m_ > 0; m_ >>= 1) { \
        const auto o_ = __shfl_xor(v, m_);                \
        v = o_ < v ? o_ : v;                              \
    }

// Buffer rows: kCoopCap, + one more batch of 64 (the merge is triggered after
// the batch that crosses kCoopCap), + the current list of <= 64 entries that
// competes again in a merge; then the 64 ranked rows.
constexpr int kCoopRows = kCoopCap + 128;

template <typename T>
constexpr size_t CoopLdsBytesPerWave() {
    return (sizeof(T) + sizeof(int)) * (size_t)(kCoopRows + 64);
}

template <typename T> struct Quad;
template <> struct Quad<float> { using type = float4; };
template <> struct Quad<double> { using type = double4; };

template <typename T>
struct WaveTopK {
    T* cd;       // LDS: candidates [kCoopRows], then ranked list [64]
    int* ci;
    T* rd;
    int* ri;
    int m;       // buffered candidates (wave-uniform)
    T best_d;    // rank = lane, valid for lane < nbest
    int best_i;
    int nbest;   // wave-uniform
    int knn;
    T kth_d;     // the k-th entry once nbest == knn (wave-uniform)
    int kth_i;

    __device__ __forceinline__ void Init(char* lds) {
        char* base = lds + CoopLdsBytesPerWave<T>() * (threadIdx.x >> 6);
        cd = (T*)base;
        rd = cd + kCoopRows;
        ci = (int*)(rd + 64);
        ri = ci + kCoopRows;
    }

    __device__ __forceinline__ void Reset(int k) {
        m = 0;
        best_d = InfOf<T>();
        best_i = kNoIndex;
        nbest = 0;
        knn = k;
        kth_d = InfOf<T>();
        kth_i = kNoIndex;
    }

    // Candidate of this lane (kNoIndex = none).
    __device__ __forceinline__ void Push(T d, int i, T, T, T) { Push(d, i); }
    __device__ __forceinline__ void Push(T d, int i) {
        // what cannot make the list any more is dropped here
        bool valid = i != kNoIndex;
        if (valid && nbest == knn && !PairLess(d, i, kth_d, kth_i)) valid = false;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(valid);
        if (mask == 0) return;
        const int lane = threadIdx.x & 63;
        const int at = m + __popcll(mask & ((1ull << lane) - 1ull));
        if (valid) {
            cd[at] = d;
            ci[at] = i;
        }
        m += __popcll(mask);
        if (m > kCoopCap) Select();  // room for one more batch of 64 is kept
    }

    __device__ __forceinline__ void Flush() {
        if (m > 0) Select();
    }

    // Merge the buffer into the ranked list.
    __device__ __forceinline__ void Select() {
        const int lane = threadIdx.x & 63;
        // the current list competes again
        int total = m;
        if (lane < nbest) {
            cd[total + lane] = best_d;
            ci[total + lane] = best_i;
        }
        total += nbest;
        // pad to whole quads with entries that sort after everything
        const int padded = (total + 3) & ~3;
        if (lane < padded - total) {
            cd[total + lane] = InfOf<T>();
            ci[total + lane] = kNoIndex;
        }
        WaveLdsSync();
        using Q = typename Quad<T>::type;
        // two candidates per lane per pass over the buffer (quad LDS reads,
        // every lane reads the same address: broadcast)
        for (int p0 = 0; p0 < total; p0 += 128) {
            const int pa = p0 + lane, pb = p0 + 64 + lane;
            const bool ha = pa < total, hb = pb < total;
            const T a_d = ha ? cd[pa] : InfOf<T>();
            const int a_i = ha ? ci[pa] : kNoIndex;
            const T b_d = hb ? cd[pb] : InfOf<T>();
            const int b_i = hb ? ci[pb] : kNoIndex;
            int ra = 0, rb = 0;
#pragma unroll 2
            for (int qi = 0; qi < padded; qi += 4) {
                const Q d4 = *(const Q*)(cd + qi);
                const int4 i4 = *(const int4*)(ci + qi);
                ra += (PairLess(d4.x, i4.x, a_d, a_i) ? 1 : 0) +
                      (PairLess(d4.y, i4.y, a_d, a_i) ? 1 : 0) +
                      (PairLess(d4.z, i4.z, a_d, a_i) ? 1 : 0) +
                      (PairLess(d4.w, i4.w, a_d, a_i) ? 1 : 0);
                rb += (PairLess(d4.x, i4.x, b_d, b_i) ? 1 : 0) +
                      (PairLess(d4.y, i4.y, b_d, b_i) ? 1 : 0) +
                      (PairLess(d4.z, i4.z, b_d, b_i) ? 1 : 0) +
                      (PairLess(d4.w, i4.w, b_d, b_i) ? 1 : 0);
            }
            if (ha && ra < knn) {
                rd[ra] = a_d;
                ri[ra] = a_i;
            }
            if (hb && rb < knn) {
                rd[rb] = b_d;
                ri[rb] = b_i;
            }
        }
        WaveLdsSync();
        nbest = total < knn ? total : knn;
        best_d = lane < nbest ? rd[lane] : InfOf<T>();
        best_i = lane < nbest ? ri[lane] : kNoIndex;
        if (nbest == knn) {
            kth_d = rd[knn - 1];
            kth_i = ri[knn - 1];
        }
        WaveLdsSync();
        m = 0;
    }
};

// Candidates of the cells [x0..x1] x [y0..y1] x [z0..z1] whose Chebyshev cell
// distance to (cx, cy, cz) is >= r_skip. RADIUS: keep d2 < nv.radius_squared.
// Sink::Push(d2, index, x, y, z) receives every lane's candidate of a batch
// (index == kNoIndex: none).
template <typename T, bool RADIUS, typename Sink>
__device__ __forceinline__ void GatherCells(const NnsView<T>& nv, const T* qq,
                                            long long cx, long long cy,
                                            long long cz, long long x0,
                                            long long x1, long long y0,
                                            long long y1, long long z0,
                                            long long z1, long long r_skip,
                                            Sink& list) {
    if (x1 < x0 || y1 < y0 || z1 < z0) return;
    const int lane = threadIdx.x & 63;
    const int nx = (int)(x1 - x0 + 1), ny = (int)(y1 - y0 + 1);
    const int nz = (int)(z1 - z0 + 1);
    const int ncell = nx * ny * nz;
    for (int base = 0; base < ncell; base += 64) {
        const int ci = base + lane;
        unsigned s0 = 0, cnt = 0;
        if (ci < ncell) {
            const long long x = x0 + ci % nx, y = y0 + (ci / nx) % ny,
                            z = z0 + ci / (nx * ny);
            long long ax = x - cx, ay = y - cy, az = z - cz;
            ax = ax < 0 ? -ax : ax;
            ay = ay < 0 ? -ay : ay;
            az = az < 0 ? -az : az;
            const long long cheb = max(ax, max(ay, az));
            if (cheb >= r_skip) {
                const unsigned b = HashCell(x, y, z) & nv.mask;
                unsigned e0;
                BucketRange(nv, b, s0, e0);
                cnt = e0 - s0;
            }
        }
        unsigned incl = cnt;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned o = __shfl_up(incl, m);
            if (lane >= m) incl += o;
        }
        const unsigned total = __shfl(incl, 63);
        const unsigned excl = incl - cnt;
        for (unsigned t0 = 0; t0 < total; t0 += 64) {
            const unsigned t = t0 + lane;
            const unsigned tc = t < total ? t : total - 1;
            // owner cell: number of lanes whose inclusive prefix is <= t
            int pos = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const unsigned v = __shfl(incl, pos + step - 1);
                if (v <= tc) pos += step;
            }
            const unsigned oe = __shfl(excl, pos);
            const unsigned os = __shfl(s0, pos);
            T d = InfOf<T>();
            int pi = kNoIndex;
            T px = T(0), py = T(0), pz = T(0);
            if (t < total) {
                const Rec4<T> p = nv.sorted[os + (t - oe)];
                px = p.x;
                py = p.y;
                pz = p.z;
                // the record's own cell must be the cell it was fetched for
                const T pp[3] = {p.x, p.y, p.z};
                long long rx, ry, rz;
                CellOf(pp, nv.inv_cell, rx, ry, rz);
                const bool own = rx >= x0 && rx <= x1 && ry >= y0 && ry <= y1 &&
                                 rz >= z0 && rz <= z1 &&
                                 (int)(rx - x0) + nx * ((int)(ry - y0) +
                                                        ny * (int)(rz - z0)) ==
                                         base + pos;
                T result = T(0);
                const T d0 = qq[0] - p.x;
                result += d0 * d0;
                const T d1 = qq[1] - p.y;
                result += d1 * d1;
                const T dd = qq[2] - p.z;
                result += dd * dd;
                if (own && (!RADIUS || result < nv.radius_squared)) {
                    d = result;
                    pi = RecIndex(p);
                }
            }
            list.Push(d, pi, px, py, pz);
        }
    }
}

// The radius-limited gather over the 27 cells around the query's cell
// (cx, cy, cz) = CellOf(qq). A statement, not a function: the compiler
// optimises a function once on its own before it inlines it, and even one
// that only forwards to GatherCells leaves every kernel that calls it with
// other code than the call written out (profiles/nns_split_kernels.json).
#define O3DMI_GATHER_BALL(T, nv, qq, cx, cy, cz, sink)                        \
    GatherCells<T, true>(nv, qq, cx, cy, cz, cx - 1, cx + 1, cy - 1, cy + 1, \
                         cz - 1, cz + 1, 0, sink)

template <typename T>
__device__ __forceinline__ void WriteTopK(const WaveTopK<T>& list, int64_t i,
                                          int* __restrict__ idx_out,
                                          T* __restrict__ d2_out,
                                          int* __restrict__ cnt_out) {
    const int lane = threadIdx.x & 63;
    if (lane < list.knn) {
        const bool ok = lane < list.nbest;
        if (idx_out) idx_out[i * list.knn + lane] = ok ? list.best_i : -1;
        if (d2_out) d2_out[i * list.knn + lane] = ok ? list.best_d : T(0);
    }
    if (cnt_out && lane == 0) cnt_out[i] = list.nbest;
}

// The finished list as a neighbour source of per-point bodies that also read
// neighbour tables (`Nb`: int count; void Load(int base, int& idx, T& d2)):
// lane j holds entry j.
template <typename T>
struct ListNb {
    int count;
    int idx;
    T d2;
    __device__ __forceinline__ void Load(int, int& i, T& d) const {
        i = idx;
        d = d2;
    }
};

template <typename T>
__device__ __forceinline__ ListNb<T> ListOf(const WaveTopK<T>& list) {
    const bool ok = (int)(threadIdx.x & 63) < list.nbest;
    return {list.nbest, ok ? list.best_i : -1, ok ? list.best_d : T(0)};
}

// HybridSearch for general max_knn (core/nns/NanoFlannImpl.h:305-370 semantics:
// neighbours with d2 < r2, ascending by (d2, index), the first max_knn kept;
// idx padded with -1, dist with 0, count = min(found, max_knn)). `out` is the
// output policy, as in KnnSearchKernel.
template <typename T, typename Out>
__global__ void __launch_bounds__(kCoopBlock)
HybridSearchKernel(NnsView<T> nv, const T* __restrict__ q, int64_t nq,
                   int max_knn, Out out) {
    extern __shared__ __align__(16) char coop_lds[];
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    WaveTopK<T> list;
    list.Init(coop_lds);
    for (int64_t i = wave; i < nq; i += n_waves) {
        const T qq[3] = {q[3 * i + 0], q[3 * i + 1], q[3 * i + 2]};
        list.Reset(max_knn);
        long long cx, cy, cz;
        CellOf(qq, nv.inv_cell, cx, cy, cz);
        O3DMI_GATHER_BALL(T, nv, qq, cx, cy, cz, list);
        list.Flush();
        out.Write(list, i);
    }
}

// Candidates at or below the floor pair were emitted in an earlier round.
template <typename T>
struct FloorSink {
    WaveTopK<T>* list;
    T floor_d;
    int floor_i;
    bool has_floor;
    __device__ __forceinline__ void Push(T d, int i, T, T, T) {
        if (has_floor && i != kNoIndex && !PairLess(floor_d, floor_i, d, i))
            i = kNoIndex;
        list->Push(d, i);
    }
};

// ---- k nearest neighbours without a radius (KnnIndex / KnnSearch) ----------
// NearestNeighborSearch::KnnSearch semantics (core/nns/NanoFlannImpl.h:
// _KnnSearchCPU, nanoflann KNNResultSet): the min(knn, N) nearest points,
// ascending by distance (ties by lower index here; nanoflann's tie order
// depends on its tree traversal). The reference's GPU path is a brute-force
// distance matrix + block select (core/nns/KnnSearchOps.cu); points in 3-D do
// better on the same bucketed grid as the radius index, searched in growing
// cubic shells: after shell r every unvisited point is farther than
// r * cell + (distance from the query to the nearest face of its own cell),
// so the walk stops as soon as the k-th distance is below that bound. The
// cell size is chosen by the host so that an occupied cell holds ~knn / 2
// points (shells 0 and 1 then usually suffice).
// A query in a sparse region would walk thousands of empty shells on a single
// fine grid, so the index is a pyramid: level l has cells 4^l times the finest;
// a level is searched for at most kKnnShells shells, then the walk restarts on
// the next coarser level (the list starts over there). The
// coarsest level spans the whole cloud in a handful of cells and is searched
// exhaustively.
// (KnnGrid and kKnnShells: nns.h.)
constexpr int kKnnMaxLevels = 12;

template <typename T>
struct KnnPyramid {
    int n_levels;
    int first_radius;  // cube radius of the first step on a level
    int first_level;   // levels [first_level, n_levels) are walked
    int exhaustive_last;  // the last level covers the cloud: search all of it
    int brute;            // scan all n_points records instead of walking cells
    int64_t n_points;
    KnnGrid<T> level[kKnnMaxLevels];
};

// Waves per SIMD the register budget of KnnSearchKernel is sized for; an
// output policy that needs more registers than four waves leave specialises
// this before the kernel is instantiated.
template <typename Out> struct KnnWaves { static constexpr int value = 4; };

template <typename T, typename Out>
__global__ void __launch_bounds__(kCoopBlock)
__attribute__((amdgpu_waves_per_eu(KnnWaves<Out>::value)))
KnnSearchKernel(KnnPyramid<T> pyr, const T* __restrict__ q, int64_t nq, int knn,
                const int* __restrict__ query_ids, int* __restrict__ retry_ids,
                int* __restrict__ retry_count, Out out) {
    extern __shared__ __align__(16) char coop_lds[];
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    WaveTopK<T> list;
    list.Init(coop_lds);
    for (int64_t w = wave; w < nq; w += n_waves) {
        // second pass: only the queries the finest level could not finish
        const int64_t i = query_ids ? (int64_t)query_ids[w] : w;
        const T qq[3] = {q[3 * i + 0], q[3 * i + 1], q[3 * i + 2]};
        bool done = false;
        if (pyr.brute) {
            // few leftover queries: one coalesced sweep over the records, the
            // k-th distance prunes almost every batch after the first merges
            list.Reset(knn);
            const Rec4<T>* rec = pyr.level[0].nv.sorted;
            const int lane = threadIdx.x & 63;
            constexpr int kAhead = 8;  // record loads in flight per lane
            for (int64_t t0 = 0; t0 < pyr.n_points; t0 += 64 * kAhead) {
                Rec4<T> p[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const int64_t t = t0 + 64 * u + lane;
                    p[u] = rec[t < pyr.n_points ? t : pyr.n_points - 1];
                }
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const int64_t t = t0 + 64 * u + lane;
                    T result = T(0);
                    const T d0 = qq[0] - p[u].x;
                    result += d0 * d0;
                    const T d1 = qq[1] - p[u].y;
                    result += d1 * d1;
                    const T dd = qq[2] - p[u].z;
                    result += dd * dd;
                    const bool in = t < pyr.n_points;
                    list.Push(in ? result : InfOf<T>(),
                              in ? RecIndex(p[u]) : kNoIndex);
                }
            }
            list.Flush();
            done = true;
        }
        for (int l = pyr.first_level; l < pyr.n_levels && !done; ++l) {
            // a coarser level covers the finer one's cells again: start over
            list.Reset(knn);
            const KnnGrid<T>& g = pyr.level[l];
            const bool last = pyr.exhaustive_last && l == pyr.n_levels - 1;
            long long c[3];
            CellOf(qq, g.nv.inv_cell, c[0], c[1], c[2]);
            // distance to the nearest face of the query's own cell
            double margin = g.cell;
            long long r0 = 0, rmax = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double lo = (double)qq[a] - (double)c[a] * g.cell;
                const double hi = (double)(c[a] + 1) * g.cell - (double)qq[a];
                margin = fmin(margin, fmin(lo, hi));
                const long long below = g.cmin[a] - c[a];
                const long long above = c[a] - g.cmax[a];
                r0 = max(r0, max(below, above));        // shells before the box
                rmax = max(rmax, max(-below, -above));  // shell covering the box
            }
            // cell assignment rounds in float64: keep a small absolute slack
            margin -= 1e-7 * g.cell;
            if (!(margin > 0)) margin = 0;
            if (last) {
                // the whole occupied box in one step
                GatherCells<T, false>(g.nv, qq, c[0], c[1], c[2], g.cmin[0],
                                      g.cmax[0], g.cmin[1], g.cmax[1],
                                      g.cmin[2], g.cmax[2], 0, list);
                list.Flush();
                done = true;
                break;
            }
            if (r0 > kKnnShells) continue;  // the box is out of reach here
            bool first = true;
            for (long long r = r0 > pyr.first_radius ? r0 : pyr.first_radius;
                 r <= kKnnShells; ++r) {
                // first step: the whole cube of radius r (shells 0..r); then
                // one shell at a time
                GatherCells<T, false>(
                        g.nv, qq, c[0], c[1], c[2], max(c[0] - r, g.cmin[0]),
                        min(c[0] + r, g.cmax[0]), max(c[1] - r, g.cmin[1]),
                        min(c[1] + r, g.cmax[1]), max(c[2] - r, g.cmin[2]),
                        min(c[2] + r, g.cmax[2]), first ? 0 : r, list);
                first = false;
                list.Flush();
                if (list.nbest == knn) {
                    const double bound = (double)r * g.cell + margin;
                    if ((double)list.kth_d < bound * bound * (1.0 - 1e-6)) {
                        done = true;
                        break;
                    }
                }
                if (r >= rmax) {  // nothing of the box lies beyond: complete
                    done = true;
                    break;
                }
            }
        }
        if (!done) {
            // first pass on the finest level only: leave it to the second
            if (retry_ids && (threadIdx.x & 63) == 0)
                retry_ids[atomicAdd(retry_count, 1)] = (int)i;
            continue;
        }
        out.Write(list, i);
    }
}

template <typename T>
KnnPyramid<T> MakePyramid(const KnnResources& res, const KnnPlan& plan,
                          int64_t n, int first_level, bool exhaustive,
                          bool brute) {
    KnnPyramid<T> pyr;
    pyr.n_levels = (int)res.levels.size();
    pyr.first_radius = 1;
    pyr.first_level = first_level;
    pyr.exhaustive_last = exhaustive ? 1 : 0;
    pyr.brute = brute ? 1 : 0;
    pyr.n_points = n;
    for (int l = 0; l < pyr.n_levels; ++l) {
        const o3dmi_nns* lv = res.levels[l];
        long long cmin[3], cmax[3];
        KnnCellBox(lv, plan, cmin, cmax);
        pyr.level[l] = MakeKnnGrid<T>(lv, cmin, cmax);
    }
    return pyr;
}

// 4. Second pass: a coalesced sweep over all records when the leftovers
// are few, else a pyramid of 4x coarser levels (built only now) whose
// last level spans the cloud in <= 4 cells per axis and is searched
// exhaustively. launch(first_level, exhaustive, brute, ids, count, retry_ids,
// retry_count) is the caller's KnnSearchKernel launch.
template <typename Launch>
int KnnSecondPass(const void* points_dev, int64_t n, int dtype, int k,
                  KnnResources& res, const KnnPlan& plan, int n_retry,
                  Launch&& launch, hipStream_t s) {
    int st;
    double sweep_limit = 2e9;  // leftover queries x points
    if (const char* e_ = std::getenv("O3DMI_KNN_SWEEP_LIMIT"))
        sweep_limit = std::atof(e_);
    const bool brute = (double)n_retry * (double)n <= sweep_limit;
    if (n_retry > 0 && brute) {
        if ((st = launch(0, false, true, res.retry + 1, n_retry, nullptr,
                         nullptr)))
            return st;
    } else if (n_retry > 0) {
        while ((int)res.levels.size() < kKnnMaxLevels &&
               plan.emax / res.levels.back()->radius > 3.0) {
            if ((st = res.AddLevel(points_dev, n, dtype,
                                   res.levels.back()->radius * 4.0, s)))
                return st;
        }
        if ((st = launch(1, true, false, res.retry + 1, n_retry, nullptr,
                         nullptr)))
            return st;
    }
    if (std::getenv("O3DMI_VERBOSE"))
        std::fprintf(stderr,
                     "[o3dmi] knn: n=%lld k=%d cell=%g levels=%d target=%g "
                     "second-pass queries=%d (%s)\n",
                     (long long)n, k, plan.h, (int)res.levels.size(),
                     plan.target, n_retry, brute ? "sweep" : "pyramid");
    return O3DMI_OK;
}

// What a first pass of the caller's own gets: the finest level of the KNN
// index and its occupied cell box. With `exhaustive` that level spans the
// whole cloud and its box is searched in one step (no retry list then); else
// a query the level cannot finish appends its id to retry_ids and is answered
// by the second pass.
struct KnnFirstPass {
    const o3dmi_nns* finest;
    long long cmin[3], cmax[3];
    int first_radius;
    int exhaustive;
    int* retry_ids;
    int* retry_count;
};

// The KNN search of q queries among n points, k = min(n, knn) <= 64. The
// finished list of query i goes through the output policy make_out(T()) of
// the point type T (TopKOut, ...): see KnnSearchKernel. `first_pass`, when
// given, is called as first_pass(const KnnFirstPass&) -> int in place of the
// first KnnSearchKernel launch. Waits for the stream (twice at least);
// *second_pass_queries (optional) = the length of the retry list.
template <typename MakeOut, typename FirstPass = std::nullptr_t>
int KnnSearchRun(const void* points_dev, int64_t n, const void* queries_dev,
                 int64_t q, int dtype, int knn, MakeOut make_out, hipStream_t s,
                 FirstPass first_pass = nullptr,
                 int64_t* second_pass_queries = nullptr) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "points must be Float32 or Float64");
    O3DMI_REQUIRE(knn > 0, "knn should be larger than 0.");
    O3DMI_REQUIRE(n > 0 && n < (1ll << 31) && points_dev, "empty dataset");
    O3DMI_REQUIRE(q >= 0 && q < (1ll << 31) - 1, "q out of range");
    const int k = (int)(n < (int64_t)knn ? n : (int64_t)knn);
    O3DMI_REQUIRE(k <= kMaxKnn, "knn > 64 is not supported");
    if (second_pass_queries) *second_pass_queries = 0;
    if (q == 0) return O3DMI_OK;
    O3DMI_REQUIRE(queries_dev, "null argument");
    KnnResources res;
    KnnPlan plan;
    int st;
    if ((st = KnnPlanFinest(points_dev, n, dtype, k, res, plan, s))) return st;

    // 3. First pass on the finest level alone; the queries it cannot finish
    // (too few points within kKnnShells shells: sparse regions, outliers,
    // queries away from the cloud) are collected for a second pass.
    if ((st = KnnAllocRetry(res, plan, q, s))) return st;
    auto launch = [&](int first_level, bool exhaustive, bool brute,
                      const int* ids, int64_t count, int* retry_ids,
                      int* retry_count) -> int {
        const dim3 grid(GridFor(count, kCoopBlock / 64, kCUs * 16)),
                block(kCoopBlock);
        auto run = [&](auto t) {
            using T = decltype(t);
            auto out = make_out(t);
            hipLaunchKernelGGL((KnnSearchKernel<T, decltype(out)>), grid, block,
                               CoopLdsBytesPerWave<T>() * (kCoopBlock / 64), s,
                               MakePyramid<T>(res, plan, n, first_level,
                                              exhaustive, brute),
                               (const T*)queries_dev, count, k, ids, retry_ids,
                               retry_count, out);
        };
        if (dtype == O3DMI_F64) run(double());
        else run(float());
        O3DMI_HIP_CHECK(hipGetLastError());
        return O3DMI_OK;
    };
    int* const retry_ids = res.retry ? res.retry + 1 : nullptr;
    if constexpr (std::is_same_v<FirstPass, std::nullptr_t>) {
        st = launch(0, plan.single, false, nullptr, q, retry_ids, res.retry);
    } else {
        KnnFirstPass fp = {res.levels[0], {}, {}, 1, plan.single ? 1 : 0,
                           retry_ids, res.retry};
        KnnCellBox(fp.finest, plan, fp.cmin, fp.cmax);
        st = first_pass(fp);
    }
    if (st) return st;
    int n_retry = 0;
    if ((st = KnnRetryCount(res, plan, &n_retry, s))) return st;
    if ((st = KnnSecondPass(points_dev, n, dtype, k, res, plan, n_retry, launch,
                            s)))
        return st;
    if (second_pass_queries) *second_pass_queries = n_retry;
    return O3DMI_OK;  // (KnnResources waits before the pool gets its blocks)
}

}  // namespace
}  // namespace o3dmi
