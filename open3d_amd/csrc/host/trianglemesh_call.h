// The call scaffold the TriangleMesh drivers (trianglemesh.cpp, mesh_bvh.cpp,
// trianglemesh_clean.cpp, trianglemesh_filter.cpp, trianglemesh_topology.cpp,
// trianglemesh_subdivide.cpp, trianglemesh_clip.cpp) share: the size and dtype
// checks, the checked int32 triangle list, the capacity refusal of the count /
// fill protocol, and the allocation of the incidence tables and the long
// lists. Download is pointcloud_call.h's.
#pragma once

#include "../trianglemesh.h"
#include "pointcloud_call.h"

namespace o3dmi {
namespace {  // every driver gets its own copy: the library exports none of it

inline int CheckSizes(int64_t v, int64_t m, int index_dtype) {
    O3DMI_REQUIRE(index_dtype == O3DMI_I32 || index_dtype == O3DMI_I64,
                  "triangles must be Int32 or Int64");
    O3DMI_REQUIRE(v >= 0 && v < (1ll << 31), "v out of range (< 2^31)");
    O3DMI_REQUIRE(m >= 0 && m <= kMeshMaxTriangles,
                  "m out of range (<= 2^29 triangles)");
    return O3DMI_OK;
}

inline int CheckFloat(int dtype) {
    O3DMI_REQUIRE(dtype == O3DMI_F32 || dtype == O3DMI_F64,
                  "positions and normals must be Float32 or Float64");
    return O3DMI_OK;
}

// The triangle list as checked int32: the caller's array, or its narrowed
// copy. One launch, one download.
inline int LoadTriangles(PoolScratch& pool, Words* w, const void* triangles_dev,
                         int64_t m, int index_dtype, int64_t v,
                         const int32_t** tri) {
    int32_t* narrowed = nullptr;
    int st = O3DMI_OK;
    if (index_dtype == O3DMI_I64 &&
        (st = pool.Alloc(&narrowed, sizeof(int32_t) * 3 * (size_t)m)))
        return st;
    st = CheckTrianglesAsync(triangles_dev, m, index_dtype, v, narrowed,
                             &w->bad, pool.s);
    if (st) return st;
    int bad = 0;
    if ((st = Download(&w->bad, &bad, sizeof(bad), pool.s))) return st;
    O3DMI_REQUIRE(!bad, "triangle index outside [0, v)");
    *tri = narrowed ? narrowed : (const int32_t*)triangles_dev;
    return O3DMI_OK;
}

// The optional {v,3} attributes of the filters and the clustering.
inline int CheckVertexAttrs(int dtype, int attr_dtype, const void* normals_dev,
                     const void* colors_dev, const void* normals_out_dev,
                     const void* colors_out_dev) {
    if ((normals_dev || colors_dev) && attr_dtype != dtype)
        return Unsupported(
                "vertex normals and colours must have the position dtype");
    O3DMI_REQUIRE(!normals_dev || normals_out_dev,
                  "null argument: normals given, no output for them");
    O3DMI_REQUIRE(!colors_dev || colors_out_dev,
                  "null argument: colours given, no output for them");
    return O3DMI_OK;
}

// The refusal of a fill call whose capacity is below the count.
inline int CapacityError(const char* what) {
    SetLastError(what);
    return O3DMI_ERR_CAPACITY;
}

// The three arrays of an edge table of n_slots slots (3 m for a mesh's own).
// The scratch of its build (IncidenceScratchBytes) stays with the caller, who
// may share it with other steps.
inline int AllocEdgeTable(PoolScratch& pool, int64_t n_slots, EdgeTable* tb) {
    const size_t bytes = sizeof(uint32_t) * (size_t)n_slots;
    int st = pool.Alloc(&tb->lo, bytes);
    if (!st) st = pool.Alloc(&tb->hi, bytes);
    if (!st) st = pool.Alloc(&tb->slot, bytes);
    return st;
}

// The four arrays of the corner table of m triangles on v vertices.
inline int AllocCornerTable(PoolScratch& pool, int64_t m, int64_t v,
                            CornerTable* tb) {
    const size_t corner_bytes = sizeof(uint32_t) * 3 * (size_t)m;
    int st = pool.Alloc(&tb->vertex, corner_bytes);
    if (!st) st = pool.Alloc(&tb->corner, corner_bytes);
    if (!st) st = pool.Alloc(&tb->count, sizeof(int32_t) * (size_t)v);
    if (!st) st = pool.Alloc(&tb->start, sizeof(int64_t) * (size_t)v);
    return st;
}

// A long list over n items: n + 1 ints, the last one the counter, zeroed on
// the pool's stream.
inline int AllocLongList(PoolScratch& pool, int64_t n, int32_t** list) {
    const int st = pool.Alloc(list, sizeof(int32_t) * ((size_t)n + 1));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(*list + n, 0, sizeof(int32_t), pool.s));
    return O3DMI_OK;
}

}  // namespace
}  // namespace o3dmi
