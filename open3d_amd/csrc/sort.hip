// Stable least-significant-digit radix sort of (key, value) pairs of uint32
// (sort.h), and its C entry o3dmi_sort_pairs_u32.
//
// One pass sorts by one digit of <= kPairSortBits bits in three launches:
//   1. PairHistKernel: a block owns kPairSortTile consecutive elements and
//      counts its digits; hist is tile-major, hist[tile * bins + digit].
//   2. PairScanKernel: one block turns the table into output offsets, walking
//      it in (digit, tile) order: offset = all elements with a smaller digit +
//      the same digit in the tiles before.
//   3. PairScatterKernel: wave w of a block owns the elements [w * 512,
//      (w + 1) * 512) of the tile, visited in 8 rounds of 64 (element = tile +
//      w * 512 + round * 64 + lane), so (tile, wave, round, lane) is index
//      order; an element's rank among the equal digits of its tile is the
//      count in the waves before + in the rounds before + in the lower lanes.
// Nothing depends on the order in which blocks or waves run: the only atomics
// are integer counts, and every output position is a function of the input.
// The tile and wave layout is VoxelDownSample's (pointcloud.hip), which keeps
// its own sort: that one builds its keys and ranks its voxels inside the
// passes.
#include "sort.h"

#include "common.h"

namespace o3dmi {
namespace {

constexpr int kWaves = kPairSortBlock / 64;
constexpr int kBins = 1 << kPairSortBits;
constexpr int kScanSegs = kPairSortBlock / kBins;  // tile ranges per column

static_assert(kBins * kScanSegs == kPairSortBlock, "scan block layout");

struct PairSortPlan {
    int passes, bits;  // bits per digit
};
inline PairSortPlan PlanPairSort(int key_bits) {
    PairSortPlan p;
    p.passes = (key_bits + kPairSortBits - 1) / kPairSortBits;
    p.bits = p.passes ? (key_bits + p.passes - 1) / p.passes : 0;
    return p;
}

inline int64_t TilesOf(int64_t n) {
    return (n + kPairSortTile - 1) / kPairSortTile;
}

__global__ void __launch_bounds__(kPairSortBlock)
PairHistKernel(const unsigned* __restrict__ keys, int64_t n, int shift,
               int bits, int* __restrict__ hist) {
    __shared__ int h[kBins];
    const int bins = 1 << bits;
    const int64_t base = (int64_t)blockIdx.x * kPairSortTile;
    for (int b = threadIdx.x; b < bins; b += kPairSortBlock) h[b] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPairSortItems; ++k) {
        const int64_t e = base + k * kPairSortBlock + threadIdx.x;
        if (e < n) atomicAdd(&h[(keys[e] >> shift) & (bins - 1)], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kPairSortBlock)
        hist[(int64_t)blockIdx.x * bins + b] = h[b];
}

// One block. Thread (seg, d) owns the tiles [seg * chunk, (seg + 1) * chunk)
// of column d: it adds them up, learns where its range starts from the sums
// of the others, then walks the range again and leaves the offsets.
__global__ void __launch_bounds__(kPairSortBlock)
PairScanKernel(int* __restrict__ hist, int n_tiles, int bits) {
    __shared__ int seg_sum[kScanSegs][kBins];
    __shared__ int dbase[kBins];
    const int bins = 1 << bits;
    const int d = threadIdx.x & (kBins - 1), seg = threadIdx.x / kBins;
    const int chunk = (n_tiles + kScanSegs - 1) / kScanSegs;
    const int t_begin = seg * chunk;
    const int t_end = t_begin + chunk < n_tiles ? t_begin + chunk : n_tiles;
    int* col = hist + d;
    int sum = 0;
    if (d < bins) {
        for (int t0 = t_begin; t0 < t_end; t0 += 16) {
            int c[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                c[u] = t0 + u < t_end ? col[(int64_t)(t0 + u) * bins] : 0;
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += c[u];
        }
    }
    seg_sum[seg][d] = sum;
    __syncthreads();
    // exclusive prefix of the column totals: the first wave, 4 digits a lane
    if (threadIdx.x < 64) {
        constexpr int kPer = kBins / 64;
        int tot[kPer], mine = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int dd = threadIdx.x * kPer + j;
            tot[j] = 0;
            if (dd < bins)
                for (int sg = 0; sg < kScanSegs; ++sg) tot[j] += seg_sum[sg][dd];
            mine += tot[j];
        }
        int incl = mine;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const int t = __shfl_up(incl, k);
            if ((int)threadIdx.x >= k) incl += t;
        }
        int run = incl - mine;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            dbase[threadIdx.x * kPer + j] = run;
            run += tot[j];
        }
    }
    __syncthreads();
    if (d >= bins) return;
    int run = dbase[d];
    for (int sg = 0; sg < seg; ++sg) run += seg_sum[sg][d];
    for (int t0 = t_begin; t0 < t_end; t0 += 16) {
        int c[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            c[u] = t0 + u < t_end ? col[(int64_t)(t0 + u) * bins] : 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (t0 + u < t_end) col[(int64_t)(t0 + u) * bins] = run;
            run += c[u];
        }
    }
}

__global__ void __launch_bounds__(kPairSortBlock)
PairScatterKernel(const unsigned* __restrict__ keys_in,
                  const unsigned* __restrict__ vals_in,
                  unsigned* __restrict__ keys_out,
                  unsigned* __restrict__ vals_out, int64_t n, int shift,
                  int bits, const int* __restrict__ offsets) {
    __shared__ int wh[kWaves][kBins];  // 16 KiB
    const int bins = 1 << bits;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wbase = (int64_t)blockIdx.x * kPairSortTile +
                          wave * (kPairSortItems * 64);
    unsigned key[kPairSortItems], val[kPairSortItems];
#pragma unroll
    for (int r = 0; r < kPairSortItems; ++r) {
        const int64_t e = wbase + r * 64 + lane;
        key[r] = 0;
        val[r] = 0;
        if (e < n) {
            key[r] = keys_in[e];
            val[r] = vals_in[e];
        }
    }
    for (int b = threadIdx.x; b < kBins * kWaves; b += kPairSortBlock)
        (&wh[0][0])[b] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPairSortItems; ++r)
        if (wbase + r * 64 + lane < n)
            atomicAdd(&wh[wave][(key[r] >> shift) & (bins - 1)], 1);
    __syncthreads();
    // per digit: where each wave's run starts in the output
    for (int b = threadIdx.x; b < bins; b += kPairSortBlock) {
        int off = offsets[(int64_t)blockIdx.x * bins + b];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int c = wh[w][b];
            wh[w][b] = off;
            off += c;
        }
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < kPairSortItems; ++r) {
        const bool valid = wbase + r * 64 + lane < n;
        const unsigned d = (key[r] >> shift) & (bins - 1);
        // lanes of this round holding the same digit
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < bits; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        int pos = 0;
        if (valid) pos = wh[wave][d] + __popcll(same & lt);
        // every lane has read its start; the first lane of each digit group
        // moves the start past the group (only this wave touches wh[wave])
        if (valid && (same & lt) == 0ull) wh[wave][d] += __popcll(same);
        if (valid) {
            keys_out[pos] = key[r];
            vals_out[pos] = val[r];
        }
    }
}

inline size_t Padded(int64_t n) { return ((size_t)n + 63) & ~(size_t)63; }

}  // namespace

size_t SortPairsScratchBytes(int64_t n) {
    if (n < 1) n = 1;
    return Padded(n) * 8 + (size_t)TilesOf(n) * kBins * sizeof(int);
}

int SortPairsAsync(uint32_t* keys_dev, uint32_t* vals_dev, int64_t n,
                   int key_bits, void* scratch_dev, hipStream_t s) {
    O3DMI_REQUIRE(n >= 0 && n < (1ll << 31), "sort: n out of range (< 2^31)");
    O3DMI_REQUIRE(key_bits >= 0 && key_bits <= 32,
                  "sort: key_bits must be in [0, 32]");
    if (n <= 1 || key_bits == 0) return O3DMI_OK;
    O3DMI_REQUIRE(keys_dev && vals_dev && scratch_dev, "null argument");
    const PairSortPlan plan = PlanPairSort(key_bits);
    unsigned* k[2] = {keys_dev, (unsigned*)scratch_dev};
    unsigned* v[2] = {vals_dev, k[1] + Padded(n)};
    int* hist = (int*)(v[1] + Padded(n));
    const int n_tiles = (int)TilesOf(n);
    const dim3 grid((unsigned)n_tiles), block(kPairSortBlock);
    for (int p = 0; p < plan.passes; ++p) {
        const int shift = p * plan.bits;
        const int bits = key_bits - shift < plan.bits ? key_bits - shift
                                                      : plan.bits;
        const int a = p & 1, b = a ^ 1;
        hipLaunchKernelGGL(PairHistKernel, grid, block, 0, s, k[a], n, shift,
                           bits, hist);
        hipLaunchKernelGGL(PairScanKernel, dim3(1), block, 0, s, hist, n_tiles,
                           bits);
        hipLaunchKernelGGL(PairScatterKernel, grid, block, 0, s, k[a], v[a],
                           k[b], v[b], n, shift, bits, hist);
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    if (plan.passes & 1) {
        O3DMI_HIP_CHECK(hipMemcpyAsync(keys_dev, k[1], sizeof(unsigned) * n,
                                       hipMemcpyDeviceToDevice, s));
        O3DMI_HIP_CHECK(hipMemcpyAsync(vals_dev, v[1], sizeof(unsigned) * n,
                                       hipMemcpyDeviceToDevice, s));
    }
    return O3DMI_OK;
}

}  // namespace o3dmi

extern "C" int o3dmi_sort_pairs_u32(uint32_t* keys_dev, uint32_t* vals_dev,
                                    int64_t n, int key_bits,
                                    o3dmi_stream_t stream) {
    using namespace o3dmi;
    O3DMI_REQUIRE(n >= 0 && n < (1ll << 31), "sort: n out of range (< 2^31)");
    O3DMI_REQUIRE(key_bits >= 0 && key_bits <= 32,
                  "sort: key_bits must be in [0, 32]");
    if (n <= 1 || key_bits == 0) return O3DMI_OK;
    O3DMI_REQUIRE(keys_dev && vals_dev, "null argument");
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(s);
    void* scratch = nullptr;
    int st = pool.Alloc(&scratch, SortPairsScratchBytes(n));
    if (st) return st;
    st = SortPairsAsync(keys_dev, vals_dev, n, key_bits, scratch, s);
    if (st) return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}
