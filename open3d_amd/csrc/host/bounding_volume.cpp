// Host driver of GetOrientedBoundingBox (MINIMAL_APPROX, PCA) and
// GetOrientedBoundingEllipsoid (docs/bounding_volumes.md): the checks, the
// convex hull on the device (HullOf, pointcloud_hull_host.h, with its waits:
// once per round of insertions), the hull's vertices widened, then
//   MINIMAL_APPROX  four launches and ONE wait for the box;
//   PCA             one launch and one wait for the nine sums, the frame on
//                   the host, two launches and one wait for the extents;
//   the ellipsoid   resident form: one launch and ONE wait for the whole loop.
//                   Streamed form: two launches per iteration and one wait per
//                   BATCH of kObeBatch iterations. The loop's end is a word on
//                   the device, which turns the launches queued behind it into
//                   no-ops, so a batch costs at most kObeBatch - 1 idle
//                   iterations (two empty launches each, a few microseconds)
//                   while a wait costs a drained queue (tens of microseconds
//                   plus the launch latency of the next batch). Upstream's
//                   clouds end after 40 .. 1000 iterations; 50 keeps the waits
//                   at <= 21 per call and the idle tail below 5 % of a full
//                   run.
// The two host-only halves (o3dmi_bounding_box_frame_from_moments,
// o3dmi_bounding_ellipsoid_from_moments) are at the end. The kernels are in
// bounding_volume.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "../bounding_volume.h"
#include "../eigen3.h"
#include "../pointcloud_hull.h"
#include "o3d_mi355x_host.h"
#include "pointcloud_hull_host.h"
#include "trianglemesh_call.h"

using namespace o3dmi;

namespace {

constexpr int kObeBatch = 50;  // streamed iterations per wait (see above)

thread_local int64_t g_stats[5] = {0, 0, 0, -1, -2};
thread_local double g_values[16] = {0};

template <typename P>
int AllocN(PoolScratch& pool, P** out, size_t count) {
    return pool.Alloc(out, sizeof(P) * std::max<size_t>(count, 1));
}

// What both calls refuse from their arguments alone.
int CheckCall(const void* points_dev, int64_t n, int dtype) {
    const int st = CheckFloat(dtype);
    if (st) return st;
    O3DMI_REQUIRE(n >= 4, "too few points for a bounding volume (n >= 4)");
    O3DMI_REQUIRE(n < (1ll << 31) - 1, "n out of range (< 2^31 - 1 points)");
    O3DMI_REQUIRE(points_dev, "null argument");
    return O3DMI_OK;
}

// The hull of a call on the device: its V vertices widened and T triangles.
struct DeviceHull {
    double* X = nullptr;
    int32_t* tri = nullptr;
    int64_t n_verts = 0;
    int64_t n_tris = 0;
};

// The finiteness gate, the cloud widened, the hull at the capacities n and
// 2 n - 4 with Int32 indices, and its vertices widened again (bit copies of
// input rows: the same values).
int HullOnDevice(PoolScratch& pool, const void* points_dev, int64_t n,
                 int dtype, DeviceHull* h) {
    hipStream_t s = pool.s;
    Words* w = nullptr;
    double* P = nullptr;
    void* positions = nullptr;
    int32_t* indices = nullptr;
    int st = AllocWords(pool, &w);
    if (st) return st;
    if ((st = RequireFinite(points_dev, n, dtype, w, s))) return st;
    if ((st = AllocN(pool, &P, 3 * (size_t)n))) return st;
    if ((st = pool.Alloc(&positions, 3 * (size_t)n * ElemSize(dtype))))
        return st;
    if ((st = AllocN(pool, &indices, (size_t)n))) return st;
    if ((st = AllocN(pool, &h->tri, 3 * (size_t)(2 * n - 4)))) return st;
    if ((st = HullWidenAsync(points_dev, n, dtype, P, s))) return st;
    const HullOutput o = {positions, indices,   n,           h->tri,
                          2 * n - 4, O3DMI_I32, &h->n_verts, &h->n_tris};
    if ((st = HullOf(pool, P, n, false, points_dev, dtype, o))) return st;
    if ((st = AllocN(pool, &h->X, 3 * (size_t)h->n_verts))) return st;
    return HullWidenAsync(positions, h->n_verts, dtype, h->X, s);
}

void ResetStats(const DeviceHull& h) {
    g_stats[0] = h.n_verts;
    g_stats[1] = h.n_tris;
    g_stats[2] = 0;
    g_stats[3] = -1;
    g_stats[4] = -2;
    for (double& v : g_values) v = 0.0;
}

// The vertex slices a triangle's box is split over in MINIMAL_APPROX: 1 (lane =
// one triangle over every vertex) unless the internal entry point asks for
// more, and never more slices than vertices. Every value gives the same bits.
int ClampSplit(int split, int64_t n_verts) {
    return (int)std::min<int64_t>(std::max(split, 1), n_verts);
}

struct Box {
    double center[3], rotation[9], extent[3];
};

int MinimalApprox(PoolScratch& pool, const DeviceHull& h, int split,
                  Box* box) {
    split = ClampSplit(split, h.n_verts);
    double* scratch = nullptr;
    unsigned long long* words = nullptr;
    ObbResult* result_dev = nullptr;
    int st = AllocN(pool, &scratch, ObbApproxScratchDoubles(h.n_tris, split));
    if (!st) st = pool.Alloc(&words, 256);
    if (!st) st = pool.Alloc(&result_dev, sizeof(ObbResult));
    if (st) return st;
    if ((st = ObbApproxAsync(h.X, h.n_verts, h.tri, h.n_tris, split, scratch,
                             words, result_dev, pool.s)))
        return st;
    ObbResult r;
    if ((st = Download(result_dev, &r, sizeof(r), pool.s))) return st;
    if (r.winner < -1.0) {
        SetLastError("oriented bounding box: no candidate has a volume");
        return O3DMI_ERR_INTERNAL;
    }
    g_stats[4] = (int64_t)r.winner;
    for (int k = 0; k < 3; ++k) {
        g_values[9 + k] = r.lo[k];
        g_values[12 + k] = r.hi[k];
        box->center[k] = r.center[k];
        box->extent[k] = r.extent[k];
    }
    for (int k = 0; k < 9; ++k) box->rotation[k] = r.rotation[k];
    return O3DMI_OK;
}

int Pca(PoolScratch& pool, const DeviceHull& h, Box* box) {
    double* scratch = nullptr;
    double* sums_dev = nullptr;
    unsigned long long* keys_dev = nullptr;
    int st = AllocN(pool, &scratch, BvSumScratchDoubles(h.n_verts));
    if (!st) st = pool.Alloc(&sums_dev, 256);
    if (!st) st = pool.Alloc(&keys_dev, 256);
    if (st) return st;
    // sums_dev[0..9) the sums, the ticket behind them
    unsigned* ticket = (unsigned*)(sums_dev + 16);
    O3DMI_HIP_CHECK(hipMemsetAsync(sums_dev, 0, 256, pool.s));
    if ((st = BvMomentsAsync(h.X, h.n_verts, scratch, ticket, sums_dev,
                             pool.s)))
        return st;
    double sums[9], mean[3];
    if ((st = Download(sums_dev, sums, sizeof(sums), pool.s))) return st;
    if ((st = o3dmi_bounding_box_frame_from_moments(h.n_verts, sums, mean,
                                                    box->rotation)))
        return st;
    if ((st = BvExtentsAsync(h.X, h.n_verts, mean, box->rotation, keys_dev,
                             pool.s)))
        return st;
    unsigned long long keys[6];
    if ((st = Download(keys_dev, keys, sizeof(keys), pool.s))) return st;
    double lo[3], hi[3], m[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = FromOrderedKey(keys[k]);
        hi[k] = FromOrderedKey(keys[3 + k]);
        m[k] = (lo[k] + hi[k]) / 2.0;
        box->extent[k] = hi[k] - lo[k];
        g_values[9 + k] = lo[k];
        g_values[12 + k] = hi[k];
    }
    const double* R = box->rotation;
    for (int r = 0; r < 3; ++r)
        box->center[r] = ((R[3 * r] * m[0] + R[3 * r + 1] * m[1]) +
                          R[3 * r + 2] * m[2]) +
                         mean[r];
    for (int k = 0; k < 9; ++k) g_values[k] = sums[k];
    return O3DMI_OK;
}

int OrientedBox(const void* points_dev, int64_t n, int dtype, int method,
                int split, double* center_out, double* rotation_out, double* extent_out,
                hipStream_t s) {
    int st = CheckCall(points_dev, n, dtype);
    if (st) return st;
    O3DMI_REQUIRE(center_out && rotation_out && extent_out, "null argument");
    O3DMI_REQUIRE(split >= 1 && split <= kObbMaxSplit, "split out of range");
    O3DMI_REQUIRE(method == O3DMI_OBB_MINIMAL_APPROX ||
                          method == O3DMI_OBB_PCA ||
                          method == O3DMI_OBB_MINIMAL_JYLANKI,
                  "method must be MINIMAL_APPROX, PCA or MINIMAL_JYLANKI");
    if (method == O3DMI_OBB_MINIMAL_JYLANKI)
        return Unsupported(
                "MINIMAL_JYLANKI: upstream's traversal order is random and "
                "its searches are seeded edge to edge, so its result is not "
                "a function of the input");
    PoolScratch pool(s);
    DeviceHull h;
    if ((st = HullOnDevice(pool, points_dev, n, dtype, &h))) return st;
    ResetStats(h);
    Box box;
    st = method == O3DMI_OBB_PCA ? Pca(pool, h, &box)
                                 : MinimalApprox(pool, h, split, &box);
    if (st) return st;
    for (int k = 0; k < 3; ++k) {
        center_out[k] = box.center[k];
        extent_out[k] = box.extent[k];
    }
    for (int k = 0; k < 9; ++k) rotation_out[k] = box.rotation[k];
    return O3DMI_OK;
}

// O3DMI_OBE_FORM (docs/switches.md; per call): "resident" or "streamed" forces
// the form of Khachiyan's loop; otherwise the resident form up to its capacity.
int ReadForm(int64_t n_verts) {
    if (const char* v = std::getenv("O3DMI_OBE_FORM")) {
        if (std::string(v) == "resident") return kObeFormResident;
        if (std::string(v) == "streamed") return kObeFormStreamed;
    }
    return n_verts <= kObeResidentCapacity ? kObeFormResident
                                           : kObeFormStreamed;
}

int KhachiyanLoop(PoolScratch& pool, const DeviceHull& h, int form,
                  ObeWords* out) {
    hipStream_t s = pool.s;
    ObeWords* words = nullptr;
    int st = pool.Alloc(&words, sizeof(ObeWords));
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(words, 0, sizeof(ObeWords), s));
    if (form == kObeFormResident) {
        if ((st = ObeResidentAsync(h.X, h.n_verts, words, s))) return st;
        return Download(words, out, sizeof(*out), s);
    }
    double* scratch = nullptr;
    if ((st = AllocN(pool, &scratch, ObeStreamScratchDoubles(h.n_verts))))
        return st;
    if ((st = ObeStreamInitAsync(h.n_verts, scratch, s))) return st;
    // sums launch k ends iteration k; the one after the last iteration only
    // ends it
    for (int k = 0; k <= kObeMaxIterations; ++k) {
        if ((st = ObeStreamSumsAsync(h.X, h.n_verts, k, scratch, words, s)))
            return st;
        if (k < kObeMaxIterations &&
            (st = ObeStreamArgmaxAsync(h.X, h.n_verts, scratch, words, s)))
            return st;
        if (k % kObeBatch == kObeBatch - 1 || k == kObeMaxIterations) {
            if ((st = Download(words, out, sizeof(*out), s))) return st;
            if (out->done) return O3DMI_OK;
        }
    }
    SetLastError("bounding ellipsoid: the loop did not end");
    return O3DMI_ERR_INTERNAL;
}

int OrientedEllipsoid(const void* points_dev, int64_t n, int dtype,
                      double* center_out, double* rotation_out,
                      double* radii_out, int32_t* iterations_out,
                      hipStream_t s) {
    int st = CheckCall(points_dev, n, dtype);
    if (st) return st;
    O3DMI_REQUIRE(center_out && rotation_out && radii_out, "null argument");
    PoolScratch pool(s);
    DeviceHull h;
    if ((st = HullOnDevice(pool, points_dev, n, dtype, &h))) return st;
    ResetStats(h);
    const int form = ReadForm(h.n_verts);
    ObeWords w;
    if ((st = KhachiyanLoop(pool, h, form, &w))) return st;
    g_stats[2] = w.iterations;
    g_stats[3] = form;
    if (w.singular) {
        SetLastError("bounding ellipsoid: Lambda is not positive definite");
        return O3DMI_ERR_SINGULAR;
    }
    double center[3], rotation[9], radii[3];
    if ((st = o3dmi_bounding_ellipsoid_from_moments(w.sums, center, rotation,
                                                    radii)))
        return st;
    for (int k = 0; k < 9; ++k) g_values[k] = w.sums[k];
    g_values[15] = w.max_m;
    for (int k = 0; k < 3; ++k) {
        center_out[k] = center[k];
        radii_out[k] = radii[k];
    }
    for (int k = 0; k < 9; ++k) rotation_out[k] = rotation[k];
    if (iterations_out) *iterations_out = w.iterations;
    return O3DMI_OK;
}

double Norm3(const double* v) {
    return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// Columns i and j of V and their eigenvalues change places.
void SwapColumns(double (&e)[3], double (&V)[3][3], int i, int j) {
    std::swap(e[i], e[j]);
    for (int r = 0; r < 3; ++r) std::swap(V[r][i], V[r][j]);
}

bool AllFinite(const double* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

}  // namespace

extern "C" {

int o3dmi_pointcloud_oriented_bounding_box(
        const void* points_dev, int64_t n, int dtype, int method,
        double center_out[3], double rotation_out[9], double extent_out[3],
        o3dmi_stream_t stream) {
    return OrientedBox(points_dev, n, dtype, method, 1, center_out,
                       rotation_out, extent_out, (hipStream_t)stream);
}

int o3dmi_internal_pointcloud_obb_minimal_approx(
        const void* points_dev, int64_t n, int dtype, int split,
        double center_out[3], double rotation_out[9], double extent_out[3],
        o3dmi_stream_t stream) {
    return OrientedBox(points_dev, n, dtype, O3DMI_OBB_MINIMAL_APPROX, split,
                       center_out, rotation_out, extent_out,
                       (hipStream_t)stream);
}

int o3dmi_pointcloud_oriented_bounding_ellipsoid(
        const void* points_dev, int64_t n, int dtype, double center_out[3],
        double rotation_out[9], double radii_out[3], int32_t* iterations_out,
        o3dmi_stream_t stream) {
    return OrientedEllipsoid(points_dev, n, dtype, center_out, rotation_out,
                             radii_out, iterations_out, (hipStream_t)stream);
}

int o3dmi_bounding_box_frame_from_moments(int64_t n, const double sums[9],
                                          double mean_out[3],
                                          double rotation_out[9]) {
    O3DMI_REQUIRE(n >= 1, "n must be >= 1");
    O3DMI_REQUIRE(sums && mean_out && rotation_out, "null argument");
    O3DMI_REQUIRE(AllFinite(sums, 9), "a sum is not finite");
    // utility/Eigen.cpp:391-403
    double c[9];
    for (int k = 0; k < 9; ++k) c[k] = sums[k] / (double)n;
    double a[3][3], V[3][3];
    a[0][0] = c[3] - c[0] * c[0];
    a[1][1] = c[6] - c[1] * c[1];
    a[2][2] = c[8] - c[2] * c[2];
    a[0][1] = a[1][0] = c[4] - c[0] * c[1];
    a[0][2] = a[2][0] = c[5] - c[0] * c[2];
    a[1][2] = a[2][1] = c[7] - c[1] * c[2];
    JacobiEigenSym3<double>(a, V);
    double e[3] = {a[0][0], a[1][1], a[2][2]};
    // geometry/BoundingVolume.cpp:251-271
    if (e[1] > e[0]) SwapColumns(e, V, 1, 0);
    if (e[2] > e[0]) SwapColumns(e, V, 2, 0);
    if (e[2] > e[1]) SwapColumns(e, V, 2, 1);
    double col[3][3];
    for (int j = 0; j < 2; ++j) {
        const double v[3] = {V[0][j], V[1][j], V[2][j]};
        const double norm = Norm3(v);
        int big = 0;
        for (int r = 0; r < 3; ++r) {
            col[j][r] = v[r] / norm;
            if (std::fabs(col[j][r]) > std::fabs(col[j][big])) big = r;
        }
        if (col[j][big] < 0.0)
            for (int r = 0; r < 3; ++r) col[j][r] = -col[j][r];
    }
    col[2][0] = col[0][1] * col[1][2] - col[0][2] * col[1][1];
    col[2][1] = col[0][2] * col[1][0] - col[0][0] * col[1][2];
    col[2][2] = col[0][0] * col[1][1] - col[0][1] * col[1][0];
    for (int k = 0; k < 3; ++k) mean_out[k] = c[k];
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j) rotation_out[3 * r + j] = col[j][r];
    return O3DMI_OK;
}

int o3dmi_bounding_ellipsoid_from_moments(const double sums[9],
                                          double center_out[3],
                                          double rotation_out[9],
                                          double radii_out[3]) {
    O3DMI_REQUIRE(sums && center_out && rotation_out && radii_out,
                  "null argument");
    O3DMI_REQUIRE(AllFinite(sums, 9), "a sum is not finite");
    // MinimumOBE.cpp:171-192
    const double* c = sums;
    double S[3][3], inv[9];
    S[0][0] = sums[3] - c[0] * c[0];
    S[1][1] = sums[6] - c[1] * c[1];
    S[2][2] = sums[8] - c[2] * c[2];
    S[0][1] = S[1][0] = sums[4] - c[0] * c[1];
    S[0][2] = S[2][0] = sums[5] - c[0] * c[2];
    S[1][2] = S[2][1] = sums[7] - c[1] * c[2];
    if (!LdltInverse<3>(S, inv)) {
        SetLastError("bounding ellipsoid: PN - c c^T is not positive "
                     "definite");
        return O3DMI_ERR_SINGULAR;
    }
    double a[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) a[i][j] = a[j][i] = inv[3 * i + j] / 3.0;
    JacobiEigenSym3<double>(a, V);
    double e[3] = {a[0][0], a[1][1], a[2][2]};
    // ascending, as Eigen's SelfAdjointEigenSolver returns them
    if (e[1] < e[0]) SwapColumns(e, V, 1, 0);
    if (e[2] < e[0]) SwapColumns(e, V, 2, 0);
    if (e[2] < e[1]) SwapColumns(e, V, 2, 1);
    double radii[3];
    for (int k = 0; k < 3; ++k) radii[k] = 1.0 / std::sqrt(e[k]);
    if (!AllFinite(radii, 3)) {
        SetLastError("bounding ellipsoid: an eigenvalue of Q is not positive");
        return O3DMI_ERR_SINGULAR;
    }
    // MapOBEToClosestIdentity (MinimumOBE.cpp:50-104)
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2},
                                    {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    double best = -1e9;
    int best_p = 0, best_bits = 7;
    for (int p = 0; p < 6; ++p)
        for (int bits = 0; bits < 8; ++bits) {
            const double s0 = (bits & 1) ? 1.0 : -1.0;
            const double s1 = (bits & 2) ? 1.0 : -1.0;
            const double s2 = (bits & 4) ? 1.0 : -1.0;
            const double score = (s0 * V[0][perms[p][0]] +
                                  s1 * V[1][perms[p][1]]) +
                                 s2 * V[2][perms[p][2]];
            if (score > best) {
                best = score;
                best_p = p;
                best_bits = bits;
            }
        }
    for (int j = 0; j < 3; ++j) {
        const double sg = (best_bits & (1 << j)) ? 1.0 : -1.0;
        for (int r = 0; r < 3; ++r)
            rotation_out[3 * r + j] = sg * V[r][perms[best_p][j]];
        radii_out[j] = radii[perms[best_p][j]];
    }
    for (int k = 0; k < 3; ++k) center_out[k] = c[k];
    return O3DMI_OK;
}

int64_t o3dmi_internal_obe_resident_capacity() { return kObeResidentCapacity; }

int o3dmi_internal_bounding_volume_stats(int64_t stats[5],
                                         double values[16]) {
    O3DMI_REQUIRE(stats && values, "null argument");
    for (int k = 0; k < 5; ++k) stats[k] = g_stats[k];
    for (int k = 0; k < 16; ++k) values[k] = g_values[k];
    return O3DMI_OK;
}

}  // extern "C"
