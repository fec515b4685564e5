// Kernels of ClipPlane / SlicePlane (trianglemesh_clip.h). Classification and
// emit run a thread per triangle and gather three float64 signed values by
// vertex index; the cut points run a thread per distinct point and gather two
// rows. All of it is bandwidth bound: no LDS, no float atomic (the only races
// are plain stores of the same flag value), and the library is built without
// FMA contraction, so every result is a pure function of the input.
#include "trianglemesh_clip.h"

#define O3DMI_LAUNCH_BLOCK kClipBlock
#include "mesh_launch.h"
#include "sort.h"

namespace o3dmi {
namespace {

// ---- the rules, shared by clip and slice ------------------------------------------
__device__ __forceinline__ uint64_t PackPair(uint32_t lo, uint32_t hi) {
    return ((uint64_t)lo << 32) | hi;
}
__device__ __forceinline__ uint32_t KeyLo(uint64_t k) {
    return (uint32_t)(k >> 32);
}
__device__ __forceinline__ uint32_t KeyHi(uint64_t k) { return (uint32_t)k; }
__device__ __forceinline__ bool IsVertexKey(uint64_t k) {
    return KeyLo(k) == KeyHi(k);
}

// The point of a crossing edge with the ends x, y in either order: the inside
// end itself when it lies on the contour, else the unordered edge.
__device__ __forceinline__ uint64_t PointKey(uint32_t x, uint32_t y, double sx,
                                             double sy, double c) {
    const bool x_in = sx >= c;
    const uint32_t u = x_in ? x : y;
    const double su = x_in ? sx : sy;
    if (su == c) return PackPair(u, u);
    return x < y ? PackPair(x, y) : PackPair(y, x);
}

// The parameter and the attribute of an edge point: the one device function
// clip and slice share, so the same edge gets the same bits from both.
__device__ __forceinline__ double CutParam(double c, double s_lo,
                                           double s_hi) {
    return (c - s_lo) / (s_hi - s_lo);
}
__device__ __forceinline__ double CutMix(double x_lo, double x_hi, double t) {
    return x_lo + t * (x_hi - x_lo);
}

// Triangle t rotated by r into (a, b, c); key_ab / key_bc / key_ca are the
// points of the rotated edges 0 (ab), 1 (bc), 2 (ca) where they cross: ab and
// ca with one vertex inside, bc and ca with two.
struct TriCut {
    int nin;
    int r;
    uint32_t a, b, c;
    uint64_t key_ab, key_bc, key_ca;
};

__device__ __forceinline__ TriCut LoadCut(const int32_t* __restrict__ tri,
                                          int64_t t,
                                          const double* __restrict__ s,
                                          double c) {
    const uint32_t t0 = (uint32_t)tri[3 * t], t1 = (uint32_t)tri[3 * t + 1],
                   t2 = (uint32_t)tri[3 * t + 2];
    const double s0 = s[t0], s1 = s[t1], s2 = s[t2];
    const bool i0 = s0 >= c, i1 = s1 >= c, i2 = s2 >= c;
    TriCut q;
    q.nin = (int)i0 + (int)i1 + (int)i2;
    q.r = 0;
    if (q.nin == 1) q.r = i0 ? 0 : (i1 ? 1 : 2);
    if (q.nin == 2) q.r = !i0 ? 1 : (!i1 ? 2 : 0);
    q.a = q.r == 0 ? t0 : (q.r == 1 ? t1 : t2);
    q.b = q.r == 0 ? t1 : (q.r == 1 ? t2 : t0);
    q.c = q.r == 0 ? t2 : (q.r == 1 ? t0 : t1);
    const double sa = q.r == 0 ? s0 : (q.r == 1 ? s1 : s2);
    const double sb = q.r == 0 ? s1 : (q.r == 1 ? s2 : s0);
    const double sc = q.r == 0 ? s2 : (q.r == 1 ? s0 : s1);
    q.key_ab = q.key_bc = q.key_ca = 0;
    if (q.nin == 1) q.key_ab = PointKey(q.a, q.b, sa, sb, c);
    if (q.nin == 2) q.key_bc = PointKey(q.b, q.c, sb, sc, c);
    if (q.nin == 1 || q.nin == 2) q.key_ca = PointKey(q.c, q.a, sc, sa, c);
    return q;
}

// The slot of the rotated edge e of triangle t.
__device__ __forceinline__ int64_t SlotOf(int64_t t, int r, int e) {
    const int k = r + e;
    return 3 * t + (k >= 3 ? k - 3 : k);
}

// Piece i of a clipped triangle: three keys and the rotated edge of each
// (unused for a vertex key). False when the triangle has no piece i.
struct Piece {
    uint64_t k0, k1, k2;
    int e0, e1, e2;
};
__device__ __forceinline__ bool ClipPiece(const TriCut& q, int i, Piece* p) {
    p->k0 = PackPair(q.a, q.a);
    p->e0 = p->e1 = p->e2 = 0;
    if (q.nin == 3 && i == 0) {
        p->k1 = PackPair(q.b, q.b);
        p->k2 = PackPair(q.c, q.c);
        return true;
    }
    if (q.nin == 1 && i == 0) {  // (a, ab, ca)
        p->k1 = q.key_ab;
        p->k2 = q.key_ca;
        p->e2 = 2;
        return true;
    }
    if (q.nin == 2 && i == 0) {  // (a, b, bc)
        p->k1 = PackPair(q.b, q.b);
        p->k2 = q.key_bc;
        p->e2 = 1;
        return true;
    }
    if (q.nin == 2 && i == 1) {  // (a, bc, ca)
        p->k1 = q.key_bc;
        p->e1 = 1;
        p->k2 = q.key_ca;
        p->e2 = 2;
        return true;
    }
    return false;
}
__device__ __forceinline__ bool PieceKept(const Piece& p) {
    return p.k0 != p.k1 && p.k1 != p.k2 && p.k0 != p.k2;
}

// The line of a sliced triangle, from where the winding leaves the inside to
// where it re-enters: (ab, ca) or (bc, ca). False when there is none or its
// ends are one point.
__device__ __forceinline__ bool SliceLine(const TriCut& q, int* e_from) {
    if (q.nin != 1 && q.nin != 2) return false;
    *e_from = q.nin == 1 ? 0 : 1;
    return (q.nin == 1 ? q.key_ab : q.key_bc) != q.key_ca;
}

// ---- classification ---------------------------------------------------------------
template <typename T>
__global__ void PlaneValuesKernel(const T* __restrict__ p, int64_t v,
                                  CutPlane pl, double* __restrict__ s,
                                  int* __restrict__ bad) {
    O3DMI_GRID_STRIDE(i, v) {
        const double x = (double)p[3 * i], y = (double)p[3 * i + 1],
                     z = (double)p[3 * i + 2];
        const double val = ((pl.n[0] * (x - pl.o[0]) + pl.n[1] * (y - pl.o[1])) +
                            pl.n[2] * (z - pl.o[2]));
        s[i] = val;
        if (!isfinite(val)) atomicOr(bad, 1);
    }
}

// The three slot flags of a triangle from the mask over its rotated edges.
__device__ __forceinline__ void StoreSlotFlags(int32_t* __restrict__ slot_used,
                                               int64_t t, int r, int mask) {
#pragma unroll
    for (int e = 0; e < 3; ++e) slot_used[SlotOf(t, r, e)] = (mask >> e) & 1;
}

__global__ void ClipClassifyKernel(const int32_t* __restrict__ tri, int64_t m,
                                   const double* __restrict__ s,
                                   int32_t* __restrict__ pieces,
                                   int32_t* __restrict__ slot_used,
                                   int32_t* __restrict__ vertex_used) {
    O3DMI_GRID_STRIDE(t, m) {
        const TriCut q = LoadCut(tri, t, s, 0.);
        int n = 0, mask = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            Piece p;
            if (!ClipPiece(q, i, &p) || !PieceKept(p)) continue;
            ++n;
            if (IsVertexKey(p.k0)) vertex_used[KeyLo(p.k0)] = 1;
            else mask |= 1 << p.e0;
            if (IsVertexKey(p.k1)) vertex_used[KeyLo(p.k1)] = 1;
            else mask |= 1 << p.e1;
            if (IsVertexKey(p.k2)) vertex_used[KeyLo(p.k2)] = 1;
            else mask |= 1 << p.e2;
        }
        pieces[t] = n;
        StoreSlotFlags(slot_used, t, q.r, mask);
    }
}

__global__ void SliceClassifyKernel(const int32_t* __restrict__ tri, int64_t m,
                                    const double* __restrict__ s, double c,
                                    int32_t* __restrict__ lines,
                                    int32_t* __restrict__ slot_used) {
    O3DMI_GRID_STRIDE(t, m) {
        const TriCut q = LoadCut(tri, t, s, c);
        int e_from = 0;
        const bool kept = SliceLine(q, &e_from);
        lines[t] = kept;
        StoreSlotFlags(slot_used, t, q.r, kept ? (1 << e_from) | 4 : 0);
    }
}

// ---- numbering --------------------------------------------------------------------
__global__ void CompactSlotsKernel(const int32_t* __restrict__ used,
                                   const int64_t* __restrict__ pos, int64_t n3,
                                   uint32_t* __restrict__ slot_of) {
    O3DMI_GRID_STRIDE(e, n3)
        if (used[e]) slot_of[pos[e]] = (uint32_t)e;
}

__device__ __forceinline__ uint64_t SlotKey(const int32_t* __restrict__ tri,
                                            const double* __restrict__ s,
                                            double c, uint32_t e) {
    const uint32_t t = e / 3, k = e - 3 * t;
    const uint32_t x = (uint32_t)tri[e];
    const uint32_t y = (uint32_t)tri[3 * (int64_t)t + (k == 2 ? 0 : k + 1)];
    return PointKey(x, y, s[x], s[y], c);
}

// 0: order = identity, keys = hi; 1: keys = lo of order; 2: keys = hi of order.
template <int kWhich>
__global__ void SlotKeysKernel(const int32_t* __restrict__ tri,
                               const double* __restrict__ s, double c,
                               const uint32_t* __restrict__ slot_of, int64_t n,
                               uint32_t* __restrict__ keys,
                               uint32_t* __restrict__ order) {
    O3DMI_GRID_STRIDE(j, n) {
        if (kWhich == 0) order[j] = (uint32_t)j;
        const uint64_t key =
                SlotKey(tri, s, c, slot_of[kWhich == 0 ? (uint32_t)j : order[j]]);
        keys[j] = kWhich == 1 ? KeyLo(key) : KeyHi(key);
    }
}

// ---- emit -------------------------------------------------------------------------
template <typename T, typename I>
__global__ void CutPointsKernel(SubdivEdges pt, int64_t n, int64_t base,
                                const double* __restrict__ s, double c,
                                CutAttrs at, I* __restrict__ source,
                                double* __restrict__ t_out) {
    O3DMI_GRID_STRIDE(q, n) {
        const int64_t lo = pt.lo[q], hi = pt.hi[q], row = base + pt.rank[q];
        const bool edge = lo != hi;
        const double t = edge ? CutParam(c, s[lo], s[hi]) : 0.;
#pragma unroll
        for (int k = 0; k < kMaxCutAttrs; ++k) {
            if (k >= at.n_attrs) continue;
            const T* __restrict__ in = (const T*)at.in[k];
            T* __restrict__ out = (T*)at.out[k];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const T x_lo = in[3 * lo + d];
                out[3 * row + d] =
                        edge ? (T)CutMix((double)x_lo, (double)in[3 * hi + d], t)
                             : x_lo;
            }
        }
        if (source) {
            source[2 * row] = (I)lo;
            source[2 * row + 1] = (I)hi;
            t_out[row] = t;
        }
    }
}

template <typename T, typename I>
__global__ void ClipOldVerticesKernel(const int32_t* __restrict__ used,
                                      const int64_t* __restrict__ old_id,
                                      int64_t v, CutAttrs at,
                                      I* __restrict__ source,
                                      double* __restrict__ t_out) {
    O3DMI_GRID_STRIDE(u, v) {
        if (!used[u]) continue;
        const int64_t row = old_id[u];
#pragma unroll
        for (int k = 0; k < kMaxCutAttrs; ++k) {
            if (k >= at.n_attrs) continue;
            const T* __restrict__ in = (const T*)at.in[k];
            T* __restrict__ out = (T*)at.out[k];
#pragma unroll
            for (int d = 0; d < 3; ++d) out[3 * row + d] = in[3 * u + d];
        }
        if (source) {
            source[2 * row] = (I)u;
            source[2 * row + 1] = (I)u;
            t_out[row] = 0.;
        }
    }
}

template <typename I>
__global__ void ClipEmitKernel(const int32_t* __restrict__ tri, int64_t m,
                               const double* __restrict__ s,
                               const int64_t* __restrict__ piece_pos,
                               const int64_t* __restrict__ old_id,
                               int64_t n_old,
                               const int64_t* __restrict__ slot_pos,
                               const int32_t* __restrict__ id_by_pos,
                               I* __restrict__ out, I* __restrict__ source) {
    O3DMI_GRID_STRIDE(t, m) {
        const TriCut q = LoadCut(tri, t, s, 0.);
        int64_t row = piece_pos[t];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            Piece p;
            if (!ClipPiece(q, i, &p) || !PieceKept(p)) continue;
            const uint64_t key[3] = {p.k0, p.k1, p.k2};
            const int edge[3] = {p.e0, p.e1, p.e2};
#pragma unroll
            for (int d = 0; d < 3; ++d)
                out[3 * row + d] =
                        (I)(IsVertexKey(key[d])
                                    ? old_id[KeyLo(key[d])]
                                    : n_old + id_by_pos[slot_pos[SlotOf(
                                                      t, q.r, edge[d])]]);
            if (source) source[row] = (I)t;
            ++row;
        }
    }
}

__global__ void SliceLineRecordsKernel(const int32_t* __restrict__ tri,
                                       int64_t m, const double* __restrict__ s,
                                       double c,
                                       const int32_t* __restrict__ lines,
                                       const int64_t* __restrict__ line_pos,
                                       const int64_t* __restrict__ slot_pos,
                                       const int32_t* __restrict__ id_by_pos,
                                       int32_t* __restrict__ rec) {
    O3DMI_GRID_STRIDE(t, m) {
        if (!lines[t]) continue;
        const TriCut q = LoadCut(tri, t, s, c);
        const int e_from = q.nin == 1 ? 0 : 1;
        const int64_t row = line_pos[t];
        rec[3 * row] = (int32_t)t;
        rec[3 * row + 1] = id_by_pos[slot_pos[SlotOf(t, q.r, e_from)]];
        rec[3 * row + 2] = id_by_pos[slot_pos[SlotOf(t, q.r, 2)]];
    }
}

template <typename I>
__global__ void SliceLinesOutKernel(const int32_t* __restrict__ rec, int64_t n,
                                    int64_t line_base, int64_t point_base,
                                    int contour, I* __restrict__ out,
                                    I* __restrict__ line_tri,
                                    int32_t* __restrict__ line_contour) {
    O3DMI_GRID_STRIDE(i, n) {
        const int64_t row = line_base + i;
        out[2 * row] = (I)(point_base + rec[3 * i + 1]);
        out[2 * row + 1] = (I)(point_base + rec[3 * i + 2]);
        if (line_tri) line_tri[row] = (I)rec[3 * i];
        if (line_contour) line_contour[row] = contour;
    }
}

}  // namespace

int PlaneValuesAsync(const void* positions_dev, int64_t v, int dtype,
                     const CutPlane& plane, double* s_dev, int* bad_dev,
                     hipStream_t s) {
    if (dtype == O3DMI_F64)
        O3DMI_LAUNCH(PlaneValuesKernel<double>, v, (const double*)positions_dev,
                     v, plane, s_dev, bad_dev);
    else
        O3DMI_LAUNCH(PlaneValuesKernel<float>, v, (const float*)positions_dev,
                     v, plane, s_dev, bad_dev);
    return O3DMI_OK;
}

int ClipClassifyAsync(const int32_t* tri, int64_t m, const double* s_dev,
                      int32_t* pieces_dev, int32_t* slot_used_dev,
                      int32_t* vertex_used_dev, hipStream_t s) {
    O3DMI_LAUNCH(ClipClassifyKernel, m, tri, m, s_dev, pieces_dev,
                 slot_used_dev, vertex_used_dev);
    return O3DMI_OK;
}

int SliceClassifyAsync(const int32_t* tri, int64_t m, const double* s_dev,
                       double c, int32_t* lines_dev, int32_t* slot_used_dev,
                       hipStream_t s) {
    O3DMI_LAUNCH(SliceClassifyKernel, m, tri, m, s_dev, c, lines_dev,
                 slot_used_dev);
    return O3DMI_OK;
}

int CompactSlotsAsync(const int32_t* slot_used_dev, const int64_t* pos_dev,
                      int64_t n_slots, uint32_t* slot_of_dev, hipStream_t s) {
    O3DMI_LAUNCH(CompactSlotsKernel, n_slots, slot_used_dev, pos_dev, n_slots,
                 slot_of_dev);
    return O3DMI_OK;
}

int SortSlotKeysAsync(const int32_t* tri, const double* s_dev, double c,
                      const uint32_t* slot_of_dev, int64_t n, int key_bits,
                      uint32_t* lo_dev, uint32_t* hi_dev, uint32_t* order_dev,
                      void* scratch_dev, hipStream_t s) {
    // by hi first, then stably by lo: ascending (lo, hi, slot)
    O3DMI_LAUNCH(SlotKeysKernel<0>, n, tri, s_dev, c, slot_of_dev, n, hi_dev,
                 order_dev);
    int st = SortPairsAsync(hi_dev, order_dev, n, key_bits, scratch_dev, s);
    if (st) return st;
    O3DMI_LAUNCH(SlotKeysKernel<1>, n, tri, s_dev, c, slot_of_dev, n, lo_dev,
                 order_dev);
    st = SortPairsAsync(lo_dev, order_dev, n, key_bits, scratch_dev, s);
    if (st) return st;
    O3DMI_LAUNCH(SlotKeysKernel<2>, n, tri, s_dev, c, slot_of_dev, n, hi_dev,
                 order_dev);
    return O3DMI_OK;
}

// kernel<T, I> by the position and the index dtype
#define O3DMI_DISPATCH_TI(kernel, n, dtype, index_dtype, I32ARGS, I64ARGS) \
    do {                                                                   \
        if ((dtype) == O3DMI_F64 && (index_dtype) == O3DMI_I64)            \
            O3DMI_LAUNCH((kernel<double, int64_t>), n, I64ARGS);           \
        else if ((dtype) == O3DMI_F64)                                     \
            O3DMI_LAUNCH((kernel<double, int32_t>), n, I32ARGS);           \
        else if ((index_dtype) == O3DMI_I64)                               \
            O3DMI_LAUNCH((kernel<float, int64_t>), n, I64ARGS);            \
        else                                                               \
            O3DMI_LAUNCH((kernel<float, int32_t>), n, I32ARGS);            \
    } while (0)

int CutPointsAsync(const SubdivEdges& points, int64_t n_points, int64_t base,
                   const double* s_dev, double c, int dtype,
                   const CutAttrs& attrs, int index_dtype, void* source_out_dev,
                   double* t_out_dev, hipStream_t s) {
#define O3DMI_ARGS(I)                                                      \
    points, n_points, base, s_dev, c, attrs, (I*)source_out_dev, t_out_dev
    O3DMI_DISPATCH_TI(CutPointsKernel, n_points, dtype, index_dtype,
                      O3DMI_ARGS(int32_t), O3DMI_ARGS(int64_t));
#undef O3DMI_ARGS
    return O3DMI_OK;
}

int ClipOldVerticesAsync(const int32_t* vertex_used_dev,
                         const int64_t* old_id_dev, int64_t v, int dtype,
                         const CutAttrs& attrs, int index_dtype,
                         void* source_out_dev, double* t_out_dev,
                         hipStream_t s) {
#define O3DMI_ARGS(I)                                                      \
    vertex_used_dev, old_id_dev, v, attrs, (I*)source_out_dev, t_out_dev
    O3DMI_DISPATCH_TI(ClipOldVerticesKernel, v, dtype, index_dtype,
                      O3DMI_ARGS(int32_t), O3DMI_ARGS(int64_t));
#undef O3DMI_ARGS
    return O3DMI_OK;
}

int ClipEmitAsync(const int32_t* tri, int64_t m, const double* s_dev,
                  const int64_t* piece_pos_dev, const int64_t* old_id_dev,
                  int64_t n_old, const int64_t* slot_pos_dev,
                  const int32_t* id_by_pos_dev, int index_dtype,
                  void* triangles_out_dev, void* triangle_source_out_dev,
                  hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(ClipEmitKernel<int64_t>, m, tri, m, s_dev, piece_pos_dev,
                     old_id_dev, n_old, slot_pos_dev, id_by_pos_dev,
                     (int64_t*)triangles_out_dev,
                     (int64_t*)triangle_source_out_dev);
    else
        O3DMI_LAUNCH(ClipEmitKernel<int32_t>, m, tri, m, s_dev, piece_pos_dev,
                     old_id_dev, n_old, slot_pos_dev, id_by_pos_dev,
                     (int32_t*)triangles_out_dev,
                     (int32_t*)triangle_source_out_dev);
    return O3DMI_OK;
}

int SliceLineRecordsAsync(const int32_t* tri, int64_t m, const double* s_dev,
                          double c, const int32_t* lines_dev,
                          const int64_t* line_pos_dev,
                          const int64_t* slot_pos_dev,
                          const int32_t* id_by_pos_dev, int32_t* rec_dev,
                          hipStream_t s) {
    O3DMI_LAUNCH(SliceLineRecordsKernel, m, tri, m, s_dev, c, lines_dev,
                 line_pos_dev, slot_pos_dev, id_by_pos_dev, rec_dev);
    return O3DMI_OK;
}

int SliceLinesOutAsync(const int32_t* rec_dev, int64_t n_lines,
                       int64_t line_base, int64_t point_base, int contour,
                       int index_dtype, void* lines_out_dev,
                       void* line_triangle_out_dev,
                       int32_t* line_contour_out_dev, hipStream_t s) {
    if (index_dtype == O3DMI_I64)
        O3DMI_LAUNCH(SliceLinesOutKernel<int64_t>, n_lines, rec_dev, n_lines,
                     line_base, point_base, contour, (int64_t*)lines_out_dev,
                     (int64_t*)line_triangle_out_dev, line_contour_out_dev);
    else
        O3DMI_LAUNCH(SliceLinesOutKernel<int32_t>, n_lines, rec_dev, n_lines,
                     line_base, point_base, contour, (int32_t*)lines_out_dev,
                     (int32_t*)line_triangle_out_dev, line_contour_out_dev);
    return O3DMI_OK;
}

}  // namespace o3dmi
