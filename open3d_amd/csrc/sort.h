// Device-wide stable sort of (key, value) pairs of uint32 (sort.hip): a
// least-significant-digit radix sort on the caller's stream, no host wait.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace o3dmi {

constexpr int kPairSortBits = 8;     // digit width, at most (PairSortPlan)
constexpr int kPairSortBlock = 1024; // 16 waves
constexpr int kPairSortItems = 8;    // elements per thread
constexpr int kPairSortTile = kPairSortBlock * kPairSortItems;  // 8192

// ceil(log2(n)): the bits that tell the values of [0, n) apart (0 for n <= 1).
inline int BitsFor(int64_t n) {
    int bits = 0;
    while (bits < 63 && (1ll << bits) < n) ++bits;
    return bits;
}

// Bytes of scratch SortPairsAsync needs for n pairs (the second pair of
// arrays and the tile histograms).
size_t SortPairsScratchBytes(int64_t n);

// Sorts the n pairs (keys[i], vals[i]) ascending by the low key_bits bits of
// the key; pairs whose keys agree there keep their input order (stable, the
// same result on every run). The sorted pairs end up in keys_dev / vals_dev.
// n < 2^31, key_bits in [0, 32]; ceil(key_bits / kPairSortBits) passes of
// equal digit width. n <= 1 or key_bits == 0 launches nothing.
int SortPairsAsync(uint32_t* keys_dev, uint32_t* vals_dev, int64_t n,
                   int key_bits, void* scratch_dev, hipStream_t s);

}  // namespace o3dmi
