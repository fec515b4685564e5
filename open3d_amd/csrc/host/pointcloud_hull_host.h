// Private host seam of the convex hull: the driver's hull routine, for the
// other drivers that start from a hull on the device
// (host/bounding_volume.cpp). Defined in host/pointcloud_hull.cpp.
#pragma once

#include <cstdint>

#include "../common.h"

namespace o3dmi {

// Where a hull goes, by the count / capacity protocol of
// o3dmi_pointcloud_convex_hull: device buffers and host counts.
struct HullOutput {
    void* positions;
    void* point_indices;
    int64_t vertex_capacity;
    void* triangles;
    int64_t triangle_capacity;
    int index_dtype;
    int64_t* n_vertices;
    int64_t* n_triangles;
};

// The hull of the m widened points P_dev, written by the count / capacity
// protocol. points_dev: the rows the output positions are copied from.
// drop_last: point m - 1 and every triangle that names it are left out.
// Scratch comes from `pool`; the waits are the hull's (one for the simplex,
// one per round, one for the counts) and the call returns with pool.s drained.
int HullOf(PoolScratch& pool, const double* P_dev, int64_t m, bool drop_last,
           const void* points_dev, int dtype, const HullOutput& o);

}  // namespace o3dmi
