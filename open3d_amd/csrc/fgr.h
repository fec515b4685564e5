// Private seam between fgr.hip (the kernels of Fast Global Registration, rules
// 1-6 of "Fast Global Registration" in o3d_mi355x.h) and host/fgr.cpp (the C
// ABI of FastGlobalRegistrationBasedOnCorrespondence / ...FeatureMatching).
// Every launcher is stream-ordered; only the tuple test waits (per batch).
#pragma once

#include "common.h"

namespace o3dmi {

constexpr int kFgrTile = 256;   // correspondences (rule 4) / rows (rule 1) per tile
constexpr int kFgrSums = 16;    // distinct sums of rule 4
constexpr int kFgrBlock = 512;  // the resident loop's one workgroup
// Resident capacity: two tiles per wave of the 512-thread workgroup, eight
// correspondences per lane in registers: 96 of a lane's 256 VGPRs hold p and
// q. (At 1024 threads a lane has 128 VGPRs; p and q of 4096 correspondences
// take 48 of them and the solve needs about 80 more: the compiler spilled
// some 300 registers to scratch memory, which is global traffic inside the
// loop.)
constexpr int64_t kFgrResident = (int64_t)(kFgrBlock / 64) * 2 * kFgrTile;

// The tuple test's batch schedule: trials per batch, doubling up to the cap.
constexpr int64_t kFgrFirstBatch = 1ll << 16;
constexpr int64_t kFgrMaxBatch = 1ll << 22;

constexpr int kFgrFormAuto = 0;
constexpr int kFgrFormResident = 1;
constexpr int kFgrFormStreamed = 2;

// What rule 1 leaves on the device: {mean_s[3], mean_t[3], max_scale_s,
// max_scale_t, scale_global, par_start} and the gate's flags.
struct FgrNormWords {
    double mean[6];
    double max_scale[2];
    double scale_global;
    double par_start;
    int bad;  // non-zero: a non-finite coordinate (CheckFiniteAsync)
    int pad;
};

// Doubles of scratch FgrNormalizeAsync needs for clouds of ns and nt rows (the
// levels of the sum tree).
size_t FgrNormScratchDoubles(int64_t ns, int64_t nt);

// Rule 1 without its host part: sums, means, max norms, scales and the two
// normalised float64 clouds. words_dev is zeroed by the caller (its `bad` may
// already carry flags).
int FgrNormalizeAsync(const void* source_dev, int64_t ns,
                      const void* target_dev, int64_t nt, int dtype,
                      int use_absolute_scale, double* scratch_dev,
                      FgrNormWords* words_dev, double* source_out_dev,
                      double* target_out_dev, hipStream_t s);

// corres_dev {n, 2}: the two columns exchanged in place.
int FgrSwapPairsAsync(int64_t* corres_dev, int64_t n, hipStream_t s);

}  // namespace o3dmi

extern "C" {
// o3dmi_fgr_tuple_test with the first batch's size given (tests place the cap
// inside a later batch); *n_batches (optional) = batches run.
int o3dmi_internal_fgr_tuple_test(uint64_t seed, const void* source_dev,
                                  int64_t ns, const void* target_dev,
                                  int64_t nt, int dtype,
                                  const int64_t* corres_dev, int64_t n_corres,
                                  double tuple_scale,
                                  int64_t maximum_tuple_count,
                                  int64_t first_batch, int64_t* tuples_dev,
                                  int64_t* n_tuples, int64_t* n_trials,
                                  int64_t* n_batches, o3dmi_stream_t stream);
// o3dmi_fgr_optimize with the form given: kFgrFormAuto (resident up to
// kFgrResident correspondences), kFgrFormResident (refused above the
// capacity) or kFgrFormStreamed. *form_out (optional) = the form that ran
// (0: fewer than 10 correspondences).
int o3dmi_internal_fgr_optimize(const double* source_dev, int64_t ns,
                                const double* target_dev, int64_t nt,
                                const int64_t* corres_dev, int64_t n_corres,
                                double par, double division_factor,
                                int decrease_mu,
                                double maximum_correspondence_distance,
                                int iteration_number, int form,
                                void* scratch_dev, double* out_dev,
                                int* form_out, o3dmi_stream_t stream);
// Bytes of scratch the streamed form needs at any count (the public
// o3dmi_fgr_optimize_scratch_bytes is 0 up to the resident capacity).
size_t o3dmi_internal_fgr_stream_scratch_bytes(int64_t n_corres);
// kFgrResident, for tests and tools.
int64_t o3dmi_internal_fgr_resident_capacity(void);
}
