// The call scaffold the PointCloud drivers (filter, smooth, segment, sample)
// share: the device word block of a call, the finiteness gate, the count
// download and the attribute check.
#pragma once

#include "../pointcloud_rows.h"
#include "host_util.h"

namespace o3dmi {
namespace {  // every driver gets its own copy: the library exports none of it

// Bytes of one coordinate; a row of points or normals is 3 of them.
inline size_t ElemSize(int dtype) { return dtype == O3DMI_F64 ? 8 : 4; }

inline int CheckAttrs(int n_attrs, const void* const* attrs_in,
                      const int64_t* row_bytes, void* const* attrs_out,
                      bool need_rows, SelectAttrs* out) {
    O3DMI_REQUIRE(n_attrs >= 1 && n_attrs <= kMaxSelectAttrs,
                  "n_attrs must be in [1, 8]");
    O3DMI_REQUIRE(attrs_in && row_bytes && attrs_out, "null argument");
    out->n_attrs = n_attrs;
    for (int k = 0; k < n_attrs; ++k) {
        O3DMI_REQUIRE(row_bytes[k] >= 1, "row_bytes must be >= 1");
        O3DMI_REQUIRE(!need_rows || (attrs_in[k] && attrs_out[k]),
                      "null attribute");
        out->in[k] = attrs_in[k];
        out->out[k] = attrs_out[k];
        out->row_bytes[k] = row_bytes[k];
    }
    return O3DMI_OK;
}

// The device word block of a call: {error flag, pad, 64-bit count, the total
// of a prefix sum}.
struct Words {
    int bad;
    int pad;
    unsigned long long count;
    long long total;
};

// A zeroed word block from the call's pool. Everything below that takes a
// Words* relies on this: nobody zeroes a word again.
inline int AllocWords(PoolScratch& pool, Words** w_dev) {
    const int st = pool.Alloc(w_dev, 256);
    if (st) return st;
    O3DMI_HIP_CHECK(hipMemsetAsync(*w_dev, 0, sizeof(Words), pool.s));
    return O3DMI_OK;
}

// dst[0 .. bytes) = src_dev[0 .. bytes) once the stream has drained: one copy,
// one wait.
inline int Download(const void* src_dev, void* dst, size_t bytes,
                    hipStream_t s) {
    O3DMI_HIP_CHECK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost,
                                   s));
    O3DMI_HIP_CHECK(hipStreamSynchronize(s));
    return O3DMI_OK;
}

// Refuses a cloud with a NaN or Inf coordinate (one launch, one download).
inline int RequireFinite(const void* points_dev, int64_t n, int dtype,
                         Words* w_dev, hipStream_t s) {
    int st = CheckFiniteAsync(points_dev, n, dtype, &w_dev->bad, s);
    if (st) return st;
    int bad = 0;
    if ((st = Download(&w_dev->bad, &bad, sizeof(bad), s))) return st;
    O3DMI_REQUIRE(!bad,
                  "non-finite coordinate: run RemoveNonFinitePoints first");
    return O3DMI_OK;
}

// *m_out = w_dev->count once the stream has drained.
inline int DownloadCount(const Words* w_dev, int64_t* m_out, hipStream_t s) {
    unsigned long long c = 0;
    const int st = Download(&w_dev->count, &c, sizeof(c), s);
    if (st) return st;
    *m_out = (int64_t)c;
    return O3DMI_OK;
}

}  // namespace
}  // namespace o3dmi
