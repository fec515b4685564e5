// Host driver of FilterSharpen / FilterSmoothSimple / FilterSmoothLaplacian /
// FilterSmoothTaubin (legacy geometry/TriangleMesh.cpp:167-440): the checks,
// the CSR adjacency once per call, the float64 ping-pong buffers of the
// attributes in scope and one FilterPassAsync per pass with no wait between
// them. The kernels are in trianglemesh_filter.hip.
#include "../trianglemesh_clean.h"
#include "o3d_mi355x_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

constexpr int kScopeAll = 0, kScopeColor = 1, kScopeNormal = 2,
              kScopeVertex = 3;  // upstream's FilterScope

bool Overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    if (!a || !b || !a_bytes || !b_bytes) return false;
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

struct FilterCall {
    const void* positions;
    int64_t v;
    int dtype;
    const void* normals;
    const void* colors;
    int attr_dtype;
    const void* triangles;
    int64_t m;
    int index_dtype;
    int scope;
    void* positions_out;
    void* normals_out;
    void* colors_out;
    hipStream_t s;
};

// `passes` passes of `kind`, pass i with factors[i % 2].
int RunFilter(const FilterCall& c, int kind, int64_t passes,
              const double factors[2]) {
    int st = CheckFloat(c.dtype);
    if (!st) st = CheckSizes(c.v, c.m, c.index_dtype);
    if (!st)
        st = CheckVertexAttrs(c.dtype, c.attr_dtype, c.normals, c.colors,
                              c.normals_out, c.colors_out);
    if (st) return st;
    O3DMI_REQUIRE(c.scope >= kScopeAll && c.scope <= kScopeVertex,
                  "scope must be 0 (All), 1 (Color), 2 (Normal) or 3 (Vertex)");
    O3DMI_REQUIRE(c.v == 0 || (c.positions && c.positions_out),
                  "null argument");
    O3DMI_REQUIRE(c.m == 0 || c.triangles, "null argument");
    const int64_t v = c.v, m = c.m;
    const size_t row_bytes = 3 * ElemSize(c.dtype) * (size_t)v;
    const size_t tri_bytes =
            3 * (c.index_dtype == O3DMI_I64 ? 8 : 4) * (size_t)m;
    const void* ins[3] = {c.positions, c.normals, c.colors};
    void* outs[3] = {c.positions_out, c.normals_out, c.colors_out};
    for (int a = 0; a < 3; ++a) {
        if (!ins[a]) continue;
        for (int b = 0; b < 3; ++b)
            O3DMI_REQUIRE(!Overlap(outs[a], row_bytes, ins[b], row_bytes),
                          "an output overlaps an input");
        for (int b = 0; b < a; ++b)
            O3DMI_REQUIRE(!ins[b] ||
                                  !Overlap(outs[a], row_bytes, outs[b],
                                           row_bytes),
                          "two outputs overlap");
        O3DMI_REQUIRE(!Overlap(outs[a], row_bytes, c.triangles, tri_bytes),
                      "an output overlaps the triangles");
    }
    if (v == 0) return O3DMI_OK;

    hipStream_t s = c.s;
    PoolScratch pool(s);
    Words* w = nullptr;
    const int32_t* tri = nullptr;
    if ((st = AllocWords(pool, &w))) return st;
    if (m > 0 && (st = LoadTriangles(pool, w, c.triangles, m, c.index_dtype, v,
                                     &tri)))
        return st;
    if ((st = RequireFinite(c.positions, v, c.dtype, w, s))) return st;

    // positions first: the laplacian's weights read slot 0 when it is theirs
    const bool in_scope[3] = {
            c.scope == kScopeAll || c.scope == kScopeVertex,
            (c.scope == kScopeAll || c.scope == kScopeNormal) && c.normals,
            (c.scope == kScopeAll || c.scope == kScopeColor) && c.colors};
    int slot_of[3], n_attrs = 0;
    for (int a = 0; a < 3; ++a) {
        slot_of[a] = -1;
        if (passes > 0 && in_scope[a]) {
            slot_of[a] = n_attrs++;
        } else if (ins[a]) {
            O3DMI_HIP_CHECK(hipMemcpyAsync(outs[a], ins[a], row_bytes,
                                           hipMemcpyDeviceToDevice, s));
        }
    }
    if (n_attrs == 0) {
        O3DMI_HIP_CHECK(hipStreamSynchronize(s));
        return O3DMI_OK;
    }

    MeshAdjacency adj = {};
    int32_t* long_list = nullptr;
    if (m > 0) {
        if ((st = BuildAdjacency(pool, tri, m, v, true, 0, O3DMI_I32, nullptr,
                                 &adj)))
            return st;
    } else {  // every list is empty
        const size_t bytes = sizeof(int64_t) * ((size_t)v + 1);
        if ((st = pool.Alloc(&adj.row_splits, bytes))) return st;
        if ((st = pool.Alloc(&adj.neighbours, sizeof(int32_t)))) return st;
        O3DMI_HIP_CHECK(hipMemsetAsync(adj.row_splits, 0, bytes, s));
    }
    if ((st = AllocLongList(pool, v, &long_list))) return st;
    if ((st = LongListsAsync(adj.row_splits, v, long_list, s))) return st;

    const size_t buf_bytes = sizeof(double) * 3 * (size_t)v;
    double* buf[kMaxFilterAttrs][2] = {};
    double* fixed_ref = nullptr;  // the positions when they are out of scope
    for (int a = 0; a < 3; ++a) {
        const int k = slot_of[a];
        if (k < 0) continue;
        if ((st = pool.Alloc(&buf[k][0], buf_bytes))) return st;
        if ((st = pool.Alloc(&buf[k][1], buf_bytes))) return st;
        if ((st = WidenAsync(ins[a], 3 * v, c.dtype, buf[k][0], s))) return st;
    }
    if (kind == kFilterLaplacian && slot_of[0] < 0) {
        if ((st = pool.Alloc(&fixed_ref, buf_bytes))) return st;
        if ((st = WidenAsync(c.positions, 3 * v, c.dtype, fixed_ref, s)))
            return st;
    }
    int cur = 0;
    for (int64_t i = 0; i < passes; ++i, cur ^= 1) {
        FilterPass pass = {};
        pass.kind = kind;
        pass.n_attrs = n_attrs;
        for (int k = 0; k < n_attrs; ++k) {
            pass.prev[k] = buf[k][cur];
            pass.next[k] = buf[k][cur ^ 1];
        }
        pass.ref = fixed_ref ? fixed_ref : pass.prev[0];
        pass.factor = factors[i % 2];
        if ((st = FilterPassAsync(adj.row_splits, adj.neighbours, v, pass,
                                  long_list, s)))
            return st;
    }
    for (int a = 0; a < 3; ++a)
        if (slot_of[a] >= 0 &&
            (st = NarrowAsync(buf[slot_of[a]][cur], 3 * v, c.dtype, outs[a],
                              s)))
            return st;
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

}  // namespace

extern "C" {

int o3dmi_trianglemesh_filter_sharpen(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double strength, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream) {
    const double factors[2] = {strength, strength};
    return RunFilter({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype, scope,
                      positions_out_dev, normals_out_dev, colors_out_dev,
                      (hipStream_t)stream},
                     kFilterSharpen, iterations, factors);
}

int o3dmi_trianglemesh_filter_smooth_simple(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        int scope, void* positions_out_dev, void* normals_out_dev,
        void* colors_out_dev, o3dmi_stream_t stream) {
    const double factors[2] = {0.0, 0.0};
    return RunFilter({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype, scope,
                      positions_out_dev, normals_out_dev, colors_out_dev,
                      (hipStream_t)stream},
                     kFilterSimple, iterations, factors);
}

int o3dmi_trianglemesh_filter_smooth_laplacian(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double lambda_filter, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream) {
    const double factors[2] = {lambda_filter, lambda_filter};
    return RunFilter({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype, scope,
                      positions_out_dev, normals_out_dev, colors_out_dev,
                      (hipStream_t)stream},
                     kFilterLaplacian, iterations, factors);
}

int o3dmi_trianglemesh_filter_smooth_taubin(
        const void* positions_dev, int64_t v, int dtype,
        const void* normals_dev, const void* colors_dev, int attr_dtype,
        const void* triangles_dev, int64_t m, int index_dtype, int iterations,
        double lambda_filter, double mu, int scope, void* positions_out_dev,
        void* normals_out_dev, void* colors_out_dev, o3dmi_stream_t stream) {
    const double factors[2] = {lambda_filter, mu};
    return RunFilter({positions_dev, v, dtype, normals_dev, colors_dev,
                      attr_dtype, triangles_dev, m, index_dtype, scope,
                      positions_out_dev, normals_out_dev, colors_out_dev,
                      (hipStream_t)stream},
                     kFilterLaplacian, 2 * (int64_t)iterations, factors);
}

}  // extern "C"
