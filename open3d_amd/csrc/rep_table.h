// The lowest-index-wins table behind RemoveDuplicatedPoints
// (pointcloud_filter.hip) and the mesh de-duplications
// (trianglemesh_clean.hip): an open-addressing table of row INDICES keyed by
// three 32- or 64-bit words that a functor makes of a row. Equal keys meet in
// one slot and keep the lowest index with atomicMin, so the representative of
// a key does not depend on which thread came first. Device code only; include
// from a .hip file.
//
// A key functor K has `using Word = uint32_t / uint64_t` and
//   __device__ int operator()(int64_t i, Word k[3]) const
// which fills k and answers kKeyed, or answers that row i has no key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace o3dmi {

constexpr int kKeyed = 0;  // k[] is the key of the row
constexpr int kAlone = 1;  // the row equals nothing, itself included: kept
constexpr int kNoKey = 2;  // not a row of the set: not kept

__device__ __forceinline__ uint32_t Fold(uint32_t w) { return w; }
__device__ __forceinline__ uint32_t Fold(uint64_t w) {
    return (uint32_t)w ^ ((uint32_t)(w >> 32) * 0x9E3779B1u);
}

template <typename W>
__device__ __forceinline__ uint32_t HashWords(const W k[3]) {
    uint32_t h = Fold(k[0]) * 0x9E3779B1u;
    h ^= (Fold(k[1]) * 0x85EBCA77u) + (h >> 15);
    h ^= (Fold(k[2]) * 0xC2B2AE3Du) + (h << 11);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// Inserts every keyed row of [0, n) into table (a power of two >= 2 n slots,
// all -1). A slot's key never changes once it is claimed (atomicMin only swaps
// in another row of the same key), so a probe sequence means the same on
// every thread and in the look-up that follows.
template <typename K>
__global__ void RepInsertKernel(K keys, int64_t n, int32_t* __restrict__ table,
                                uint32_t slot_mask) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        typename K::Word k[3], q[3];
        if (keys(i, k) != kKeyed) continue;
        uint32_t h = HashWords(k) & slot_mask;
        for (;;) {
            const int32_t prev = atomicCAS(&table[h], -1, (int32_t)i);
            if (prev == -1) break;
            keys(prev, q);
            if (q[0] == k[0] && q[1] == k[1] && q[2] == k[2]) {
                atomicMin(&table[h], (int32_t)i);
                break;
            }
            h = (h + 1) & slot_mask;
        }
    }
}

// The lowest row whose key equals k, the key of the inserted row i.
template <typename K>
__device__ __forceinline__ int32_t RepFind(const K& keys, int64_t i,
                                           const typename K::Word k[3],
                                           const int32_t* __restrict__ table,
                                           uint32_t slot_mask) {
    typename K::Word q[3];
    uint32_t h = HashWords(k) & slot_mask;
    for (;;) {
        const int32_t res = table[h];
        if (res < 0) return (int32_t)i;  // unreachable: i was inserted
        keys(res, q);
        if (q[0] == k[0] && q[1] == k[1] && q[2] == k[2]) return res;
        h = (h + 1) & slot_mask;
    }
}

}  // namespace o3dmi
