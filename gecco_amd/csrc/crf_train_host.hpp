// Host helpers of the two trainers (crf_train.hip, crf_train_general.hip): upload, error return, concatenation, launch size.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_model.hpp"
#include "crf_plan.hpp"

namespace gecco {

// Allocates *d for h (one element where h is empty, so that the pointer is a device pointer either way) and copies h there.
template <class T>
int dev_upload(T **d, const std::vector<T> &h, const char *what) {
    int rc = check_hip(hipMalloc(reinterpret_cast<void **>(d), std::max<size_t>(h.size(), 1) * sizeof(T)), what);
    if (rc) return rc;
    if (h.empty()) return GECCO_CRF_OK;
    return check_hip(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice), what);
}

inline int fail(const std::string &msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

template <class T>
void append(std::vector<T> &dst, const std::vector<T> &src) {
    dst.insert(dst.end(), src.begin(), src.end());
}

inline int64_t blocks_of(int64_t n, int per) { return (n + per - 1) / per; }

}  // namespace gecco
