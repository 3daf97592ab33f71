// Host helpers of the two trainers (crf_train.hip, crf_train_general.hip): error return, concatenation, launch size.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_hip_own.hpp"
#include "crf_model.hpp"
#include "crf_plan.hpp"

namespace gecco {

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
