// Lock-free union-find over an int parent[] array, shared by ClusterDBSCAN's
// union sweep (pointcloud_segment.hip) and ClusterConnectedTriangles
// (trianglemesh.hip). parent[] is a forest in which a non-root's parent is always a SMALLER
// index: a root is only ever hooked under a smaller root, with one CAS, so
// trees cannot form cycles and the root of a finished tree is the lowest
// index of its component whatever order the waves ran in.
#pragma once

#include <hip/hip_runtime.h>

namespace o3dmi {

// Follows parent[] to a root. The reads are relaxed agent-scope atomic loads:
// other waves hook roots while this one walks, and a plain load may be served
// from a line another XCD has since changed. What is read may still be out of
// date (a root that has been hooked meanwhile); the CAS in DbscanUnite decides.
__device__ __forceinline__ int DbscanFind(int* parent, int x) {
    while (true) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;  // p < x: the walk ends
    }
}

// Unites the trees of a and b. Nothing here waits for another wave: the loop
// repeats only after a failed CAS, which means some other hook of that root
// succeeded (at most n - 1 hooks exist), and it continues from the value the
// CAS returned.
__device__ __forceinline__ void DbscanUnite(int* parent, int a, int b) {
    while (true) {
        a = DbscanFind(parent, a);
        b = DbscanFind(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return;
        a = old;  // hi was hooked under `old` < hi by somebody else
        b = lo;
    }
}

}  // namespace o3dmi
