// Small helpers shared by the host drivers (registration, odometry, RANSAC,
// rigid multiway alignment): 4x4 float64 matrices and the scope guards of a
// driver call's device resources.
#pragma once

#include <cstring>

#include "../common.h"
#include "../nns.h"

namespace o3dmi {

inline void Eye4(double* T) {
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// C = A B, row-major (C may be A or B): update.Matmul(transformation),
// Registration.cpp:319 (host F64).
inline void Matmul4(const double* A, const double* B, double* C) {
    double R[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
            R[i * 4 + j] = s;
        }
    std::memcpy(C, R, sizeof(R));
}

// Records `msg` and returns the status of a mode this backend does not have.
static inline int Unsupported(const char* msg) {
    SetLastError(msg);
    return O3DMI_ERR_UNSUPPORTED;
}

struct DeviceBuffer {
    void* p = nullptr;
    // The driver drains the stream before its buffers go out of scope
    // (SyncOnExit below).
    ~DeviceBuffer() { PoolFree(p); }
    int Alloc(size_t bytes) {
        PoolFree(p);
        p = nullptr;
        return PoolAlloc(&p, bytes ? bytes : 1);
    }
};

// `completed`: set by the owner once every kernel that used the index is
// known to have finished (its results were read on the host); the destructor
// then skips the device-wide wait of the public o3dmi_nns_destroy.
struct NnsGuard {
    o3dmi_nns_t* nns = nullptr;
    bool completed = false;
    ~NnsGuard() {
        if (completed) o3dmi_internal_nns_destroy_completed(nns);
        else o3dmi_nns_destroy(nns);
    }
};

// Declared after a call's pooled buffers so that it runs first on every exit
// path: pooled buffers may only be released once the streams have drained.
// `drained`: set once the host has SEEN the last launch of the call finish
// (the mailbox of the final evaluation): the caller's stream is in order,
// and everything the side stream did was waited for by a later launch on
// the caller's stream, so both are idle -- and hipStreamSynchronize costs
// 16 us per stream even then (measured: 32 us of every tracked frame).
struct SyncOnExit {
    hipStream_t s;
    hipStream_t side = nullptr;
    bool drained = false;
    ~SyncOnExit() {
        if (drained) return;
        (void)hipStreamSynchronize(s);
        if (side && side != s) (void)hipStreamSynchronize(side);
    }
};

}  // namespace o3dmi
