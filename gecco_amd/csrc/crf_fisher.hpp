// Two-sided Fisher exact test over a batch of 2x2 tables (gecco_crf_fisher_exact, include/gecco_crf.h).
#pragma once
#include <cstdint>

namespace gecco {

// The argument checks of gecco_crf_fisher_exact (no device needed): GECCO_CRF_OK or GECCO_CRF_EINVAL with a message.
int fisher_check(const int64_t *tables, int64_t n, const double *pvalue);
// The p-values of n >= 1 checked tables on `device` (the current device is the caller's business).  Synchronous.
int fisher_exact(int32_t device, const int64_t *tables, int64_t n, double *pvalue);

}  // namespace gecco
