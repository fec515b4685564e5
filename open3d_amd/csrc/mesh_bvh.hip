// A linear BVH over the triangles of one mesh and its closest-point query
// (mesh_bvh.h). Build: the scene box, a 30-bit Morton code per triangle, the
// stable pair sort (sort.h), a Karras radix tree over (code, sorted position)
// and a bottom-up refit with one arrival counter per inner node. Query: one
// lane per query, near child first, the far child on a stack in LDS. Ray
// queries: the same walk with slab intervals for box distances, one template
// with a policy per kind (closest, any, next above a given t; count, list
// and vote iterate the last). No result depends on the tree: see the header.
#include "mesh_bvh.h"

#include "mesh_launch.h"
#include "sort.h"

namespace o3dmi {
namespace {

inline size_t Align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the per-pair function ------------------------------------------------------
__device__ __forceinline__ float Dot3(const float x[3], const float y[3]) {
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// ((gx gx) + gy gy) + gz gz of the gap between q and the box [lo, hi].
__device__ __forceinline__ float BoxDist2(const float q[3], const float lo[3],
                                          const float hi[3]) {
    const float gx = fmaxf(fmaxf(lo[0] - q[0], q[0] - hi[0]), 0.0f);
    const float gy = fmaxf(fmaxf(lo[1] - q[1], q[1] - hi[1]), 0.0f);
    const float gz = fmaxf(fmaxf(lo[2] - q[2], q[2] - hi[2]), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// RaycastingScene.cpp:206-274, branch for branch.
__device__ __forceinline__ void ClosestPointTriangle(
        const float p[3], const float a[3], const float b[3], const float c[3],
        float out[3], float* tex_u, float* tex_v) {
    float ab[3], ac[3], ap[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
    }
    const float d1 = Dot3(ab, ap);
    const float d2 = Dot3(ac, ap);
    if (d1 <= 0.f && d2 <= 0.f) {
        *tex_u = 0;
        *tex_v = 0;
        for (int k = 0; k < 3; ++k) out[k] = a[k];
        return;
    }
    float bp[3];
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const float d3 = Dot3(ab, bp);
    const float d4 = Dot3(ac, bp);
    if (d3 >= 0.f && d4 <= d3) {
        *tex_u = 1;
        *tex_v = 0;
        for (int k = 0; k < 3; ++k) out[k] = b[k];
        return;
    }
    float cp[3];
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const float d5 = Dot3(ab, cp);
    const float d6 = Dot3(ac, cp);
    if (d6 >= 0.f && d5 <= d6) {
        *tex_u = 0;
        *tex_v = 1;
        for (int k = 0; k < 3; ++k) out[k] = c[k];
        return;
    }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float v = d1 / (d1 - d3);
        *tex_u = v;
        *tex_v = 0;
        for (int k = 0; k < 3; ++k) out[k] = a[k] + v * ab[k];
        return;
    }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float v = d2 / (d2 - d6);
        *tex_u = 0;
        *tex_v = v;
        for (int k = 0; k < 3; ++k) out[k] = a[k] + v * ac[k];
        return;
    }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        const float v = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        *tex_u = 1 - v;
        *tex_v = v;
        for (int k = 0; k < 3; ++k) out[k] = b[k] + v * (c[k] - b[k]);
        return;
    }
    const float denom = 1.f / ((va + vb) + vc);
    const float v = vb * denom;
    const float w = vc * denom;
    *tex_u = v;
    *tex_v = w;
    for (int k = 0; k < 3; ++k) out[k] = (a[k] + v * ab[k]) + w * ac[k];
}

struct Tri {
    float a[3], b[3], c[3];
    uint32_t id;
};

__device__ __forceinline__ Tri LoadLeaf(const BvhLeaf* __restrict__ leaves,
                                        int64_t pos) {
    const float4* w = (const float4*)(leaves + pos);
    const float4 w0 = w[0], w1 = w[1], w2 = w[2];
    Tri t;
    t.a[0] = w0.x; t.a[1] = w0.y; t.a[2] = w0.z;
    t.b[0] = w0.w; t.b[1] = w1.x; t.b[2] = w1.y;
    t.c[0] = w1.z; t.c[1] = w1.w; t.c[2] = w2.x;
    t.id = __float_as_uint(w2.y);
    return t;
}

__device__ __forceinline__ void TriBox(const Tri& t, float lo[3],
                                       float hi[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(fminf(t.a[k], t.b[k]), t.c[k]);
        hi[k] = fmaxf(fmaxf(t.a[k], t.b[k]), t.c[k]);
    }
}

// d2(q, t) of the header, with the closest point and its coordinates.
__device__ __forceinline__ float PairD2(const float q[3], const Tri& t,
                                        float p[3], float* u, float* v) {
    ClosestPointTriangle(q, t.a, t.b, t.c, p, u, v);
    const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    const float e2 = (dx * dx + dy * dy) + dz * dz;
    float lo[3], hi[3];
    TriBox(t, lo, hi);
    const float b2 = BoxDist2(q, lo, hi);
    // not fmaxf: a NaN e2 stays NaN
    return e2 != e2 ? e2 : (e2 > b2 ? e2 : b2);
}

// ---- build --------------------------------------------------------------------
// Floats as unsigned words that order like the values.
__device__ __forceinline__ uint32_t OrderedBits(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float FromOrderedBits(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// scene[0..2] = min, scene[3..5] = max over the vertices the triangles name,
// as ordered words (0xFFFFFFFF / 0 beforehand).
__global__ void SceneBoxKernel(const float* __restrict__ pos,
                               const int32_t* __restrict__ tri, int64_t m,
                               uint32_t* __restrict__ scene) {
    float lo[3] = {INFINITY, INFINITY, INFINITY};
    float hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    O3DMI_GRID_STRIDE(t, m) {
        for (int c = 0; c < 3; ++c) {
            const int64_t u = tri[3 * t + c];
            for (int k = 0; k < 3; ++k) {
                const float x = pos[3 * u + k];
                lo[k] = fminf(lo[k], x);
                hi[k] = fmaxf(hi[k], x);
            }
        }
    }
    for (int k = 0; k < 3; ++k) {
        for (int w = 32; w > 0; w >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], w));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], w));
        }
    }
    // one set of atomics per workgroup: every wave of the launch adding its
    // own to the same six words took 565 us at 2 M triangles
    __shared__ float part[kBlock / 64][6];
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 3; ++k) {
            part[threadIdx.x >> 6][k] = lo[k];
            part[threadIdx.x >> 6][3 + k] = hi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        float l = part[0][k], h = part[0][3 + k];
        for (int w = 1; w < kBlock / 64; ++w) {
            l = fminf(l, part[w][k]);
            h = fmaxf(h, part[w][3 + k]);
        }
        if (l <= h) {  // the workgroup saw a triangle
            atomicMin(&scene[k], OrderedBits(l));
            atomicMax(&scene[3 + k], OrderedBits(h));
        }
    }
}

__global__ void SceneBoxDecodeKernel(const uint32_t* __restrict__ scene,
                                     float* __restrict__ out) {
    if (threadIdx.x < 6) out[threadIdx.x] = FromOrderedBits(scene[threadIdx.x]);
}

// The 10-bit cell of x in [lo, hi]; an axis of zero extent is cell 0.
__device__ __forceinline__ uint32_t Cell10(float x, float lo, float hi) {
    const float extent = hi - lo;
    if (!(extent > 0.0f)) return 0u;
    // fmaxf / fminf drop a NaN (an extent past FLT_MAX)
    const float f = fminf(fmaxf((x - lo) / extent * 1024.0f, 0.0f), 1023.0f);
    return (uint32_t)f;
}

__device__ __forceinline__ uint32_t Spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ uint32_t Morton30(const float p[3],
                                             const float* __restrict__ scene) {
    return (Spread10(Cell10(p[0], scene[0], scene[3])) << 2) |
           (Spread10(Cell10(p[1], scene[1], scene[4])) << 1) |
           Spread10(Cell10(p[2], scene[2], scene[5]));
}

__global__ void TriangleCodesKernel(const float* __restrict__ pos,
                                    const int32_t* __restrict__ tri, int64_t m,
                                    const float* __restrict__ scene,
                                    uint32_t* __restrict__ keys,
                                    uint32_t* __restrict__ vals) {
    O3DMI_GRID_STRIDE(t, m) {
        float centre[3];
        for (int k = 0; k < 3; ++k) {
            const float a = pos[3 * (int64_t)tri[3 * t] + k];
            const float b = pos[3 * (int64_t)tri[3 * t + 1] + k];
            const float c = pos[3 * (int64_t)tri[3 * t + 2] + k];
            centre[k] = 0.5f * fminf(fminf(a, b), c) +
                        0.5f * fmaxf(fmaxf(a, b), c);
        }
        keys[t] = Morton30(centre, scene);
        vals[t] = (uint32_t)t;
    }
}

__global__ void LeavesKernel(const float* __restrict__ pos,
                             const int32_t* __restrict__ tri, int64_t m,
                             const uint32_t* __restrict__ sorted_tri,
                             BvhLeaf* __restrict__ leaves) {
    O3DMI_GRID_STRIDE(i, m) {
        const uint32_t t = sorted_tri[i];
        BvhLeaf leaf;
        for (int k = 0; k < 3; ++k) {
            leaf.a[k] = pos[3 * (int64_t)tri[3 * (int64_t)t] + k];
            leaf.b[k] = pos[3 * (int64_t)tri[3 * (int64_t)t + 1] + k];
            leaf.c[k] = pos[3 * (int64_t)tri[3 * (int64_t)t + 2] + k];
        }
        leaf.id = t;
        leaf.parent = -1;  // m == 1; RadixTreeKernel sets the others after
        leaf.pad = 0;
        leaves[i] = leaf;
    }
}

// The length of the common prefix of keys i and j, a key being (code, sorted
// position); -1 outside [0, m).
__device__ __forceinline__ int Delta(const uint32_t* __restrict__ codes,
                                     int64_t m, int64_t i, int64_t j) {
    if (j < 0 || j >= m) return -1;
    const uint32_t x = codes[i] ^ codes[j];
    if (x) return __clz((int)x);
    return 32 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// Karras, "Maximizing parallelism in the construction of BVHs, octrees and
// k-d trees" (2012), section 3: inner node i of m - 1.
__global__ void RadixTreeKernel(const uint32_t* __restrict__ codes, int64_t m,
                                BvhNode* __restrict__ nodes,
                                BvhLeaf* __restrict__ leaves) {
    O3DMI_GRID_STRIDE(i, m - 1) {
        const int d =
                Delta(codes, m, i, i + 1) - Delta(codes, m, i, i - 1) < 0 ? -1
                                                                           : 1;
        const int dmin = Delta(codes, m, i, i - d);
        int64_t lmax = 2;
        while (Delta(codes, m, i, i + lmax * d) > dmin) lmax *= 2;
        int64_t l = 0;
        for (int64_t t = lmax / 2; t >= 1; t /= 2)
            if (Delta(codes, m, i, i + (l + t) * d) > dmin) l += t;
        const int64_t j = i + l * d;
        const int dnode = Delta(codes, m, i, j);
        int64_t split = 0;
        int64_t t = l;
        do {
            t = (t + 1) >> 1;
            if (Delta(codes, m, i, i + (split + t) * d) > dnode) split += t;
        } while (t > 1);
        const int64_t gamma = i + split * d + (d < 0 ? -1 : 0);
        const int64_t first = i < j ? i : j, last = i < j ? j : i;
        const int32_t me = (int32_t)i << 1;
        if (first == gamma) {
            nodes[i].child[0] = ~(int32_t)gamma;
            leaves[gamma].parent = me;
        } else {
            nodes[i].child[0] = (int32_t)gamma;
            nodes[gamma].parent = me;
        }
        if (last == gamma + 1) {
            nodes[i].child[1] = ~(int32_t)(gamma + 1);
            leaves[gamma + 1].parent = me | 1;
        } else {
            nodes[i].child[1] = (int32_t)(gamma + 1);
            nodes[gamma + 1].parent = me | 1;
        }
        nodes[i].arrivals = 0;
        if (i == 0) nodes[0].parent = -1;
    }
}

// One thread per leaf climbs: it leaves its box in its parent's slot, and the
// second child to arrive at a node goes on with the union. The boxes are
// handed over inside the launch, between workgroups: write-through stores,
// drained before the relaxed agent-scope ticket, and agent-scope loads in the
// thread that reads them (the LastArrival pattern of common.h).
__global__ void RefitKernel(BvhNode* __restrict__ nodes,
                            const BvhLeaf* __restrict__ leaves, int64_t m) {
    O3DMI_GRID_STRIDE(i, m) {
        const Tri t = LoadLeaf(leaves, i);
        float box[6];
        TriBox(t, box, box + 3);
        int32_t up = leaves[i].parent;
        // at most one climb per level; the bound only guards a broken tree
        for (int step = 0; up >= 0 && step < 2 * kBvhStack; ++step) {
            BvhNode* node = nodes + (up >> 1);
            const int side = up & 1;
            for (int k = 0; k < 6; ++k)
                __hip_atomic_store(&node->box[side][k], box[k],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (__hip_atomic_fetch_add(&node->arrivals, 1, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT) == 0)
                break;  // the sibling's thread goes on
            for (int k = 0; k < 3; ++k) {
                const float lo = __hip_atomic_load(&node->box[side ^ 1][k],
                                                   __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                const float hi = __hip_atomic_load(&node->box[side ^ 1][3 + k],
                                                   __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                box[k] = fminf(box[k], lo);
                box[3 + k] = fmaxf(box[3 + k], hi);
            }
            up = node->parent;
        }
    }
}

// ---- query --------------------------------------------------------------------
constexpr int kQueryBlock = 128;

__global__ void QueryCodesKernel(const float* __restrict__ queries, int64_t q,
                                 MeshBvhView bvh, uint32_t* __restrict__ keys,
                                 uint32_t* __restrict__ vals) {
    float scene[6];
    for (int k = 0; k < 3; ++k) {
        scene[k] = bvh.scene_lo[k];
        scene[3 + k] = bvh.scene_hi[k];
    }
    O3DMI_GRID_STRIDE(i, q) {
        const float p[3] = {queries[3 * i], queries[3 * i + 1],
                            queries[3 * i + 2]};
        keys[i] = Morton30(p, scene);
        vals[i] = (uint32_t)i;
    }
}

template <bool COUNT>
__global__ void __launch_bounds__(kQueryBlock)
ClosestPointKernel(MeshBvhView bvh, const float* __restrict__ queries,
                   const uint32_t* __restrict__ order, int64_t nq,
                   MeshQueryOut out, int* __restrict__ status,
                   unsigned long long* __restrict__ visits) {
    // entry e of this lane's stack: stack[e * kQueryBlock + threadIdx.x]
    __shared__ int32_t stack[kBvhStack * kQueryBlock];
    unsigned long long opened = 0, tested = 0;
    bool overflow = false;
    O3DMI_GRID_STRIDE(slot, nq) {
        const int64_t i = order ? (int64_t)order[slot] : slot;
        const float q[3] = {queries[3 * i], queries[3 * i + 1],
                            queries[3 * i + 2]};
        float best = INFINITY;
        uint32_t best_id = kBvhNoTriangle;
        int32_t best_pos = -1;
        int sp = 0;
        int32_t node = bvh.m == 1 ? ~0 : 0;
        for (;;) {
            bool pop = true;
            if (node < 0) {
                const int32_t pos = ~node;
                const Tri t = LoadLeaf(bvh.leaves, pos);
                float p[3], u, v;
                const float d2 = PairD2(q, t, p, &u, &v);
                if (COUNT) ++tested;
                if (d2 < best || (d2 == best && t.id < best_id)) {
                    best = d2;
                    best_id = t.id;
                    best_pos = pos;
                }
            } else {
                const float4* w = (const float4*)(bvh.nodes + node);
                const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                const int32_t c0 = (int32_t)__float_as_uint(w0.x);
                const int32_t c1 = (int32_t)__float_as_uint(w0.y);
                const float lo0[3] = {w1.x, w1.y, w1.z};
                const float hi0[3] = {w1.w, w2.x, w2.y};
                const float lo1[3] = {w2.z, w2.w, w3.x};
                const float hi1[3] = {w3.y, w3.z, w3.w};
                const float b0 = BoxDist2(q, lo0, hi0);
                const float b1 = BoxDist2(q, lo1, hi1);
                if (COUNT) ++opened;
                // skipped only when strictly farther than the best: a node
                // at the best's distance may hold a lower index
                const bool go0 = !(b0 > best), go1 = !(b1 > best);
                if (go0 && go1) {
                    const bool near0 = b0 <= b1;
                    if (sp < kBvhStack) {
                        stack[sp * kQueryBlock + threadIdx.x] =
                                near0 ? c1 : c0;
                        ++sp;
                    } else {
                        overflow = true;  // never, by the bound in mesh_bvh.h
                    }
                    node = near0 ? c0 : c1;
                    pop = false;
                } else if (go0 || go1) {
                    node = go0 ? c0 : c1;
                    pop = false;
                }
            }
            if (pop) {
                if (sp == 0) break;
                --sp;
                node = stack[sp * kQueryBlock + threadIdx.x];
            }
        }
        float p[3] = {0, 0, 0}, n[3] = {0, 0, 0}, u = 0, v = 0;
        if (best_pos >= 0) {
            const Tri t = LoadLeaf(bvh.leaves, best_pos);
            PairD2(q, t, p, &u, &v);
            if (out.normals) {
                // cross_3x1(b - a, c - a), then the mesh rule of
                // NormalizeNormals
                float e1[3], e2[3];
                for (int k = 0; k < 3; ++k) {
                    e1[k] = t.b[k] - t.a[k];
                    e2[k] = t.c[k] - t.a[k];
                }
                n[0] = e1[1] * e2[2] - e1[2] * e2[1];
                n[1] = e1[2] * e2[0] - e1[0] * e2[2];
                n[2] = e1[0] * e2[1] - e1[1] * e2[0];
                const float norm = sqrtf((n[0] * n[0] + n[1] * n[1]) +
                                         n[2] * n[2]);
                if (norm > 0) {
                    n[0] /= norm;
                    n[1] /= norm;
                    n[2] /= norm;
                }
            }
        }
        if (out.points)
            for (int k = 0; k < 3; ++k) out.points[3 * i + k] = p[k];
        if (out.ids) out.ids[i] = best_id;
        if (out.uvs) {
            out.uvs[2 * i] = u;
            out.uvs[2 * i + 1] = v;
        }
        if (out.normals)
            for (int k = 0; k < 3; ++k) out.normals[3 * i + k] = n[k];
        if (out.distance) out.distance[i] = sqrtf(best);
        if (out.d2) out.d2[i] = best;
    }
    if (overflow) atomicOr(status, 1);
    if (COUNT) {
        for (int w = 32; w > 0; w >>= 1) {
            opened += __shfl_xor(opened, w);
            tested += __shfl_xor(tested, w);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&visits[0], opened);
            atomicAdd(&visits[1], tested);
        }
    }
}

// ---- ray queries ----------------------------------------------------------------
struct Ray {
    float o[3], d[3];
};

__device__ __forceinline__ Ray LoadRay(const float* __restrict__ rays,
                                       int64_t i) {
    Ray r;
    for (int k = 0; k < 3; ++k) {
        r.o[k] = rays[6 * i + k];
        r.d[k] = rays[6 * i + 3 + k];
    }
    return r;
}

// The slab interval [T0, T1] of the header; false when it is empty.
__device__ __forceinline__ bool Slab(const Ray& r, const float lo[3],
                                     const float hi[3], float tnear,
                                     float tfar, float* T0, float* T1) {
    float t0 = tnear, t1 = tfar;
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
        if (r.d[k] != 0.0f) {
            const float a = (lo[k] - r.o[k]) / r.d[k];
            const float b = (hi[k] - r.o[k]) / r.d[k];
            t0 = fmaxf(t0, fminf(a, b));
            t1 = fminf(t1, fmaxf(a, b));
        } else if (r.o[k] < lo[k] || r.o[k] > hi[k]) {
            inside = false;
        }
    }
    *T0 = t0;
    *T1 = t1;
    return inside && t0 <= t1;
}

__device__ __forceinline__ void Cross3(const float x[3], const float y[3],
                                       float out[3]) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

// The pair of the header: whether it hits, and then t, u, v.
__device__ __forceinline__ bool PairRay(const Ray& r, const Tri& tr,
                                        float tnear, float tfar, float* t,
                                        float* u, float* v) {
    float e1[3], e2[3], s[3], p[3], q[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = tr.b[k] - tr.a[k];
        e2[k] = tr.c[k] - tr.a[k];
        s[k] = r.o[k] - tr.a[k];
    }
    Cross3(r.d, e2, p);
    const float det = Dot3(e1, p);
    if (det == 0.0f || det != det) return false;
    const float inv = 1.0f / det;
    *u = Dot3(s, p) * inv;
    Cross3(s, e1, q);
    *v = Dot3(r.d, q) * inv;
    const float te = Dot3(e2, q) * inv;
    if (!(*u >= 0.0f && *v >= 0.0f && *u + *v <= 1.0f)) return false;
    float lo[3], hi[3], T0, T1;
    TriBox(tr, lo, hi);
    if (!Slab(r, lo, hi, tnear, tfar, &T0, &T1)) return false;
    if (!(te > tnear && te <= tfar)) return false;
    *t = fminf(fmaxf(te, T0), T1) + 0.0f;
    return true;
}

enum RayPolicy { kPolicyClosest, kPolicyAny, kPolicyNext };

struct RayBest {
    float t;
    uint32_t id;
    int32_t pos;  // the winner's leaf, -1: none
};

struct RayVisits {
    unsigned long long opened, tested;
    bool overflow;
};

// One traversal of the tree for one ray, near child first (by T0), the far
// child on this lane's stack (entry e at stack[e * kQueryBlock]).
// kPolicyClosest: *best = the minimum (t, id) over the hitting pairs.
// kPolicyNext: the same over the pairs with t > prev. kPolicyAny: returns at
// the first hit, best->pos >= 0 then. *best comes in as {+inf, none, -1}.
template <int POLICY, bool COUNT>
__device__ __forceinline__ void TraverseRay(const MeshBvhView& bvh,
                                            const Ray& r, float tnear,
                                            float tfar, float prev,
                                            int32_t* __restrict__ stack,
                                            RayBest* best, RayVisits* vis) {
    int sp = 0;
    int32_t node = bvh.m == 1 ? ~0 : 0;
    for (;;) {
        bool pop = true;
        if (node < 0) {
            const int32_t pos = ~node;
            const Tri tr = LoadLeaf(bvh.leaves, pos);
            float t, u, v;
            const bool hit = PairRay(r, tr, tnear, tfar, &t, &u, &v);
            if (COUNT) ++vis->tested;
            if (hit && (POLICY != kPolicyNext || t > prev)) {
                if (POLICY == kPolicyAny) {
                    best->pos = pos;
                    return;
                }
                if (t < best->t || (t == best->t && tr.id < best->id)) {
                    best->t = t;
                    best->id = tr.id;
                    best->pos = pos;
                }
            }
        } else {
            const float4* w = (const float4*)(bvh.nodes + node);
            const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            const int32_t c0 = (int32_t)__float_as_uint(w0.x);
            const int32_t c1 = (int32_t)__float_as_uint(w0.y);
            const float lo0[3] = {w1.x, w1.y, w1.z};
            const float hi0[3] = {w1.w, w2.x, w2.y};
            const float lo1[3] = {w2.z, w2.w, w3.x};
            const float hi1[3] = {w3.y, w3.z, w3.w};
            float a0, a1, b0, b1;
            bool go0 = Slab(r, lo0, hi0, tnear, tfar, &a0, &b0);
            bool go1 = Slab(r, lo1, hi1, tnear, tfar, &a1, &b1);
            if (COUNT) ++vis->opened;
            if (POLICY != kPolicyAny) {
                // skipped only when strictly farther than the best: a node
                // at the best's t may hold a lower index
                go0 = go0 && !(a0 > best->t);
                go1 = go1 && !(a1 > best->t);
            }
            if (POLICY == kPolicyNext) {
                go0 = go0 && b0 > prev;
                go1 = go1 && b1 > prev;
            }
            if (go0 && go1) {
                const bool near0 = a0 <= a1;
                if (sp < kBvhStack) {
                    stack[sp * kQueryBlock] = near0 ? c1 : c0;
                    ++sp;
                } else {
                    vis->overflow = true;  // never, by the bound in mesh_bvh.h
                }
                node = near0 ? c0 : c1;
                pop = false;
            } else if (go0 || go1) {
                node = go0 ? c0 : c1;
                pop = false;
            }
        }
        if (pop) {
            if (sp == 0) return;
            --sp;
            node = stack[sp * kQueryBlock];
        }
    }
}

// The number of distinct t among the hitting pairs of r on (0, +inf].
template <bool COUNT>
__device__ __forceinline__ int CountRay(const MeshBvhView& bvh, const Ray& r,
                                        int32_t* __restrict__ stack,
                                        RayVisits* vis) {
    int count = 0;
    float prev = -INFINITY;
    for (;;) {
        RayBest best = {INFINITY, kBvhNoTriangle, -1};
        TraverseRay<kPolicyNext, COUNT>(bvh, r, 0.0f, INFINITY, prev, stack,
                                        &best, vis);
        if (best.pos < 0) return count;
        ++count;
        prev = best.t;  // strictly above the last one: the loop ends
    }
}

template <bool COUNT>
__device__ __forceinline__ void FlushRayVisits(
        const RayVisits& vis, int* __restrict__ status,
        unsigned long long* __restrict__ visits) {
    if (vis.overflow) atomicOr(status, 1);
    if (COUNT) {
        unsigned long long opened = vis.opened, tested = vis.tested;
        for (int w = 32; w > 0; w >>= 1) {
            opened += __shfl_xor(opened, w);
            tested += __shfl_xor(tested, w);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&visits[0], opened);
            atomicAdd(&visits[1], tested);
        }
    }
}

__global__ void OriginCodesKernel(const float* __restrict__ rows, int stride,
                                  int64_t q, MeshBvhView bvh,
                                  uint32_t* __restrict__ keys,
                                  uint32_t* __restrict__ vals) {
    float scene[6];
    for (int k = 0; k < 3; ++k) {
        scene[k] = bvh.scene_lo[k];
        scene[3 + k] = bvh.scene_hi[k];
    }
    O3DMI_GRID_STRIDE(i, q) {
        const float p[3] = {rows[stride * i], rows[stride * i + 1],
                            rows[stride * i + 2]};
        keys[i] = Morton30(p, scene);
        vals[i] = (uint32_t)i;
    }
}

template <int KIND, bool COUNT>
__global__ void __launch_bounds__(kQueryBlock)
RayQueryKernel(MeshBvhView bvh, const float* __restrict__ rays,
               const uint32_t* __restrict__ order, int64_t nq, float tnear,
               float tfar, RayQueryOut out, int* __restrict__ status,
               unsigned long long* __restrict__ visits) {
    __shared__ int32_t stack_all[kBvhStack * kQueryBlock];
    int32_t* stack = stack_all + threadIdx.x;
    RayVisits vis = {0, 0, false};
    O3DMI_GRID_STRIDE(slot, nq) {
        const int64_t i = order ? (int64_t)order[slot] : slot;
        const Ray r = LoadRay(rays, i);
        if (KIND == kRayCount) {
            const int count = CountRay<COUNT>(bvh, r, stack, &vis);
            if (out.counts) out.counts[i] = count;
            continue;
        }
        RayBest best = {INFINITY, kBvhNoTriangle, -1};
        if (KIND == kRayAny) {
            TraverseRay<kPolicyAny, COUNT>(bvh, r, tnear, tfar, 0.0f, stack,
                                           &best, &vis);
            if (out.occluded) out.occluded[i] = best.pos >= 0 ? 1 : 0;
            continue;
        }
        TraverseRay<kPolicyClosest, COUNT>(bvh, r, tnear, tfar, 0.0f, stack,
                                           &best, &vis);
        float t = INFINITY, n[3] = {0, 0, 0}, u = 0, v = 0;
        if (best.pos >= 0) {
            const Tri tr = LoadLeaf(bvh.leaves, best.pos);
            PairRay(r, tr, tnear, tfar, &t, &u, &v);
            if (out.normals) {
                // as ClosestPointKernel's
                float e1[3], e2[3];
                for (int k = 0; k < 3; ++k) {
                    e1[k] = tr.b[k] - tr.a[k];
                    e2[k] = tr.c[k] - tr.a[k];
                }
                Cross3(e1, e2, n);
                const float norm = sqrtf((n[0] * n[0] + n[1] * n[1]) +
                                         n[2] * n[2]);
                if (norm > 0) {
                    n[0] /= norm;
                    n[1] /= norm;
                    n[2] /= norm;
                }
            }
        }
        if (out.t_hit) out.t_hit[i] = t;
        if (out.geometry_ids)
            out.geometry_ids[i] = best.pos >= 0 ? 0u : kBvhNoTriangle;
        if (out.primitive_ids) out.primitive_ids[i] = best.id;
        if (out.uvs) {
            out.uvs[2 * i] = u;
            out.uvs[2 * i + 1] = v;
        }
        if (out.normals)
            for (int k = 0; k < 3; ++k) out.normals[3 * i + k] = n[k];
    }
    FlushRayVisits<COUNT>(vis, status, visits);
}

__global__ void __launch_bounds__(kQueryBlock)
RayListKernel(MeshBvhView bvh, const float* __restrict__ rays, int64_t nq,
              const int64_t* __restrict__ splits, RayListOut out,
              int* __restrict__ status) {
    __shared__ int32_t stack_all[kBvhStack * kQueryBlock];
    int32_t* stack = stack_all + threadIdx.x;
    RayVisits vis = {0, 0, false};
    O3DMI_GRID_STRIDE(i, nq) {
        const Ray r = LoadRay(rays, i);
        int64_t at = splits[i];
        float prev = -INFINITY;
        for (;;) {
            RayBest best = {INFINITY, kBvhNoTriangle, -1};
            TraverseRay<kPolicyNext, false>(bvh, r, 0.0f, INFINITY, prev,
                                            stack, &best, &vis);
            if (best.pos < 0) break;
            if (out.ray_ids) out.ray_ids[at] = i;
            if (out.t_hit) out.t_hit[at] = best.t;
            if (out.geometry_ids) out.geometry_ids[at] = 0u;
            if (out.primitive_ids) out.primitive_ids[at] = best.id;
            if (out.uvs) {
                const Tri tr = LoadLeaf(bvh.leaves, best.pos);
                float t, u = 0, v = 0;
                PairRay(r, tr, 0.0f, INFINITY, &t, &u, &v);
                out.uvs[2 * at] = u;
                out.uvs[2 * at + 1] = v;
            }
            ++at;
            prev = best.t;
        }
    }
    FlushRayVisits<false>(vis, status, nullptr);
}

// A point's rays go to `lanes` = min(nsamples, kVoteLanes) neighbouring lanes
// of one wave (lane k of them takes the directions k, k + lanes, ...), and
// the first of them adds up their odd counts by shuffles. The rays of a point
// share their origin and nearly their direction, so the lanes walk the tree
// together; one lane running them in turn took twice as long as a count
// query over the {nsamples q, 6} ray tensor.
constexpr int kVoteLanes = 8;
constexpr int kVoteWaves = kQueryBlock / 64;

// How many points one workgroup takes in a pass.
inline __host__ __device__ int VotePointsPerBlock(int lanes) {
    return kVoteWaves * (64 / lanes);
}

__global__ void __launch_bounds__(kQueryBlock)
RayVoteKernel(MeshBvhView bvh, const float* __restrict__ points, int64_t nq,
              const float* __restrict__ dirs, int nsamples, int lanes,
              float* __restrict__ occupancy, float* __restrict__ distance,
              int* __restrict__ status) {
    __shared__ int32_t stack_all[kBvhStack * kQueryBlock];
    int32_t* stack = stack_all + threadIdx.x;
    RayVisits vis = {0, 0, false};
    const int per_wave = 64 / lanes, per_block = VotePointsPerBlock(lanes);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = lane / lanes, first = lane % lanes;
    // every lane of a wave makes the same number of passes: the shuffles
    // below see all of them
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < nq;
         base += (int64_t)gridDim.x * per_block) {
        const int64_t i = base + wave * per_wave + slot;
        const bool mine = slot < per_wave && i < nq;
        int odd = 0;
        if (mine) {
            Ray r;
            for (int k = 0; k < 3; ++k) r.o[k] = points[3 * i + k];
            for (int j = first; j < nsamples; j += lanes) {
                for (int k = 0; k < 3; ++k) r.d[k] = dirs[3 * j + k];
                odd += CountRay<false>(bvh, r, stack, &vis) & 1;
            }
        }
        int votes = odd;
        for (int k = 1; k < lanes; ++k) votes += __shfl_down(odd, k);
        if (mine && first == 0) {
            const bool inside = votes > nsamples / 2;
            if (occupancy) occupancy[i] = inside ? 1.0f : 0.0f;
            if (distance) distance[i] = distance[i] * (inside ? -1.0f : 1.0f);
        }
    }
    FlushRayVisits<false>(vis, status, nullptr);
}

__global__ void PinholeRaysKernel(PinholeFrame f, int width, int64_t n,
                                  float* __restrict__ rays) {
    O3DMI_GRID_STRIDE(i, n) {
        const float px = (float)(int)(i % width) + 0.5f;
        const float py = (float)(int)(i / width) + 0.5f;
        for (int k = 0; k < 3; ++k) {
            rays[6 * i + k] = f.centre[k];
            rays[6 * i + 3 + k] =
                    (f.dir[3 * k] * px + f.dir[3 * k + 1] * py) +
                    f.dir[3 * k + 2];
        }
    }
}

}  // namespace

size_t MeshBvhBuildScratchBytes(int64_t m) {
    // the scene words, keys, values, then the sort's
    return 256 + 2 * Align256(sizeof(uint32_t) * (size_t)m) +
           Align256(SortPairsScratchBytes(m));
}

int BuildMeshBvhAsync(const float* positions_dev, const int32_t* tri,
                      int64_t m, BvhNode* nodes_dev, BvhLeaf* leaves_dev,
                      float* scene_dev, void* scratch_dev, hipStream_t s) {
    O3DMI_REQUIRE(positions_dev && tri && m > 0 && leaves_dev && scene_dev &&
                          scratch_dev && (m == 1 || nodes_dev),
                  "null argument");
    char* base = (char*)scratch_dev;
    uint32_t* scene_words = (uint32_t*)base;
    uint32_t* keys = (uint32_t*)(base + 256);
    uint32_t* vals =
            (uint32_t*)(base + 256 + Align256(sizeof(uint32_t) * (size_t)m));
    void* sort_scratch = base + 256 + 2 * Align256(sizeof(uint32_t) * (size_t)m);
    O3DMI_HIP_CHECK(hipMemsetAsync(scene_words, 0xFF, 3 * sizeof(uint32_t), s));
    O3DMI_HIP_CHECK(hipMemsetAsync(scene_words + 3, 0, 3 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(SceneBoxKernel, dim3(GridFor(m, kBlock, kCUs)),
                       dim3(kBlock), 0, s, positions_dev, tri, m, scene_words);
    hipLaunchKernelGGL(SceneBoxDecodeKernel, dim3(1), dim3(64), 0, s,
                       scene_words, scene_dev);
    O3DMI_LAUNCH(TriangleCodesKernel, m, positions_dev, tri, m, scene_dev,
                 keys, vals);
    int st = SortPairsAsync(keys, vals, m, kBvhMortonBits, sort_scratch, s);
    if (st) return st;
    O3DMI_LAUNCH(LeavesKernel, m, positions_dev, tri, m, vals, leaves_dev);
    if (m > 1) {
        O3DMI_LAUNCH(RadixTreeKernel, m - 1, keys, m, nodes_dev, leaves_dev);
        O3DMI_LAUNCH(RefitKernel, m, nodes_dev, leaves_dev, m);
    }
    return O3DMI_OK;
}

size_t MeshBvhQueryScratchBytes(int64_t q) {
    return 2 * Align256(sizeof(uint32_t) * (size_t)q) +
           Align256(SortPairsScratchBytes(q));
}

int MeshBvhQueryAsync(const MeshBvhView& bvh, const float* queries_dev,
                      int64_t q, const MeshQueryOut& out, bool sort_queries,
                      void* scratch_dev, int* status_dev,
                      unsigned long long* visits_dev, hipStream_t s) {
    O3DMI_REQUIRE(bvh.leaves && bvh.m > 0 && (bvh.m == 1 || bvh.nodes) &&
                          queries_dev && q > 0 && status_dev,
                  "null argument");
    O3DMI_REQUIRE(!sort_queries || scratch_dev, "null argument");
    const uint32_t* order = nullptr;
    if (sort_queries) {
        char* base = (char*)scratch_dev;
        uint32_t* keys = (uint32_t*)base;
        uint32_t* vals =
                (uint32_t*)(base + Align256(sizeof(uint32_t) * (size_t)q));
        void* sort_scratch =
                base + 2 * Align256(sizeof(uint32_t) * (size_t)q);
        O3DMI_LAUNCH(QueryCodesKernel, q, queries_dev, q, bvh, keys, vals);
        const int st =
                SortPairsAsync(keys, vals, q, kBvhMortonBits, sort_scratch, s);
        if (st) return st;
        order = vals;
    }
    const dim3 grid((unsigned)GridFor(q, kQueryBlock, kCUs * 16)),
            block(kQueryBlock);
    if (visits_dev)
        hipLaunchKernelGGL(ClosestPointKernel<true>, grid, block, 0, s, bvh,
                           queries_dev, order, q, out, status_dev, visits_dev);
    else
        hipLaunchKernelGGL(ClosestPointKernel<false>, grid, block, 0, s, bvh,
                           queries_dev, order, q, out, status_dev, visits_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

namespace {

inline dim3 RayGrid(int64_t q) {
    return dim3((unsigned)GridFor(q, kQueryBlock, kCUs * 16));
}

template <int KIND>
void LaunchRayQuery(const MeshBvhView& bvh, const float* rays,
                    const uint32_t* order, int64_t q, float tnear, float tfar,
                    const RayQueryOut& out, int* status,
                    unsigned long long* visits, hipStream_t s) {
    if (visits)
        hipLaunchKernelGGL((RayQueryKernel<KIND, true>), RayGrid(q),
                           dim3(kQueryBlock), 0, s, bvh, rays, order, q, tnear,
                           tfar, out, status, visits);
    else
        hipLaunchKernelGGL((RayQueryKernel<KIND, false>), RayGrid(q),
                           dim3(kQueryBlock), 0, s, bvh, rays, order, q, tnear,
                           tfar, out, status, visits);
}

}  // namespace

int MeshBvhRayQueryAsync(const MeshBvhView& bvh, RayQueryKind kind,
                         const float* rays_dev, int64_t q, float tnear,
                         float tfar, const RayQueryOut& out, bool sort_rays,
                         void* scratch_dev, int* status_dev,
                         unsigned long long* visits_dev, hipStream_t s) {
    O3DMI_REQUIRE(bvh.leaves && bvh.m > 0 && (bvh.m == 1 || bvh.nodes) &&
                          rays_dev && q > 0 && status_dev,
                  "null argument");
    O3DMI_REQUIRE(!sort_rays || scratch_dev, "null argument");
    O3DMI_REQUIRE(tnear == tnear && tfar == tfar, "tnear / tfar is NaN");
    const uint32_t* order = nullptr;
    if (sort_rays) {
        char* base = (char*)scratch_dev;
        uint32_t* keys = (uint32_t*)base;
        uint32_t* vals =
                (uint32_t*)(base + Align256(sizeof(uint32_t) * (size_t)q));
        void* sort_scratch =
                base + 2 * Align256(sizeof(uint32_t) * (size_t)q);
        O3DMI_LAUNCH(OriginCodesKernel, q, rays_dev, 6, q, bvh, keys, vals);
        const int st =
                SortPairsAsync(keys, vals, q, kBvhMortonBits, sort_scratch, s);
        if (st) return st;
        order = vals;
    }
    switch (kind) {
        case kRayClosest:
            LaunchRayQuery<kRayClosest>(bvh, rays_dev, order, q, tnear, tfar,
                                        out, status_dev, visits_dev, s);
            break;
        case kRayAny:
            LaunchRayQuery<kRayAny>(bvh, rays_dev, order, q, tnear, tfar, out,
                                    status_dev, visits_dev, s);
            break;
        case kRayCount:
            LaunchRayQuery<kRayCount>(bvh, rays_dev, order, q, 0.0f, INFINITY,
                                      out, status_dev, visits_dev, s);
            break;
        default:
            O3DMI_REQUIRE(false, "unknown ray query kind");
    }
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int MeshBvhRayListAsync(const MeshBvhView& bvh, const float* rays_dev,
                        int64_t q, const int64_t* splits_dev,
                        const RayListOut& out, int* status_dev,
                        hipStream_t s) {
    O3DMI_REQUIRE(bvh.leaves && bvh.m > 0 && (bvh.m == 1 || bvh.nodes) &&
                          rays_dev && q > 0 && splits_dev && status_dev,
                  "null argument");
    hipLaunchKernelGGL(RayListKernel, RayGrid(q), dim3(kQueryBlock), 0, s, bvh,
                       rays_dev, q, splits_dev, out, status_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int MeshBvhVoteAsync(const MeshBvhView& bvh, const float* points_dev,
                     int64_t q, const float* dirs_dev, int nsamples,
                     float* occupancy_out_dev, float* distance_io_dev,
                     int* status_dev, hipStream_t s) {
    O3DMI_REQUIRE(bvh.leaves && bvh.m > 0 && (bvh.m == 1 || bvh.nodes) &&
                          points_dev && q > 0 && dirs_dev && status_dev,
                  "null argument");
    O3DMI_REQUIRE(nsamples >= 1 && (nsamples & 1),
                  "nsamples must be odd and >= 1");
    const int lanes = nsamples < kVoteLanes ? nsamples : kVoteLanes;
    const dim3 grid(
            (unsigned)GridFor(q, VotePointsPerBlock(lanes), kCUs * 16));
    hipLaunchKernelGGL(RayVoteKernel, grid, dim3(kQueryBlock), 0, s, bvh,
                       points_dev, q, dirs_dev, nsamples, lanes,
                       occupancy_out_dev, distance_io_dev, status_dev);
    O3DMI_HIP_CHECK(hipGetLastError());
    return O3DMI_OK;
}

int CreateRaysPinholeAsync(const PinholeFrame& frame, int width, int height,
                           float* rays_out_dev, hipStream_t s) {
    O3DMI_REQUIRE(width > 0 && height > 0 && rays_out_dev, "null argument");
    const int64_t n = (int64_t)width * height;
    O3DMI_LAUNCH(PinholeRaysKernel, n, frame, width, n, rays_out_dev);
    return O3DMI_OK;
}

}  // namespace o3dmi
