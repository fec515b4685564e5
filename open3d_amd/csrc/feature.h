// Private seam between the FPFH / feature-matching driver (host/feature.cpp)
// and feature.hip (each entry point is described at its definition).
#pragma once

#include "common.h"

extern "C" {

int o3dmi_internal_fpfh_mark_indices(const int64_t* idx_dev, int64_t m,
                                     int64_t n, uint8_t* mask_dev,
                                     int* bad_dev, o3dmi_stream_t stream);
int o3dmi_internal_fpfh_mark_lists(const int32_t* idx_dev, int64_t m,
                                   uint8_t* mask_dev, o3dmi_stream_t stream);
int o3dmi_internal_mask_nonzero(const uint8_t* mask_dev, int64_t n,
                                int32_t* list32_dev, int64_t* list64_dev,
                                int64_t* count, o3dmi_stream_t stream);
int o3dmi_internal_short_rows(const int32_t* counts_dev, int64_t n, int k,
                              int32_t* ids_dev, int* n_ids_dev, int* n_ids,
                              o3dmi_stream_t stream);
int o3dmi_internal_bounds(const void* points_dev, int64_t n, int dtype,
                          double* lo, double* hi, o3dmi_stream_t stream);
int o3dmi_internal_feature_nn1(const void* a_dev, int64_t na, const void* b_dev,
                               int64_t nb, int dim, int dtype,
                               int32_t* nn_dev, o3dmi_stream_t stream);
int o3dmi_internal_feature_mutual(const int32_t* ij_dev, const int32_t* ji_dev,
                                  int64_t n, int mutual_filter, float ratio,
                                  int64_t* corres_dev, int64_t* info_dev,
                                  o3dmi_stream_t stream);

}  // extern "C"
