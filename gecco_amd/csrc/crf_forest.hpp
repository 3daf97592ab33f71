// Random-forest fit and predict of GECCO's cluster type classifier (gecco_crf_forest_*, include/gecco_crf.h).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "crf_hip_own.hpp"

namespace gecco {

// Range of gecco_crf_forest_fit: one workgroup per tree keeps the tree's sample and feature arrays in LDS.
constexpr int32_t kForestMaxSamples = 4096;
constexpr int32_t kForestMaxFeatures = 8192;
constexpr int32_t kForestMaxOutputs = 64;
constexpr int32_t kForestMaxProblems = 1024;  // forests fitted or scored by one launch (gecco_crf_forest_*_batch)

struct Forest {
    int32_t device = 0;
    int32_t n_trees = 0, n_features = 0, n_outputs = 0, max_n_classes = 1, cap = 0;  // cap: node slots per tree (2 n - 1)
    std::vector<uint8_t> n_classes;
    std::vector<int32_t> node_count, max_depth;
    // device, [n_trees][cap] (value: [n_trees][cap][n_outputs][max_n_classes]); all of them lie in the one allocation d_slab
    DeviceBlock<char> d_slab;
    int32_t *d_left = nullptr, *d_right = nullptr, *d_feature = nullptr, *d_n_node = nullptr;
    double *d_threshold = nullptr, *d_impurity = nullptr, *d_weighted = nullptr, *d_value = nullptr;
    uint8_t *d_ncls = nullptr;
};

// What differs between the problems of one forest_fit_batch: the per-problem arguments of gecco_crf_forest_fit.
struct ForestProblem {
    int32_t n_samples;
    const int32_t *col_ptr, *row_idx;
    const float *values;
    const uint8_t *n_classes, *y;
    const int32_t *sample_counts;
    const uint32_t *rand_state;
};

// Argument checks of gecco_crf_forest_fit (no device needed): GECCO_CRF_OK or GECCO_CRF_EINVAL with a message.
int forest_fit_check(int32_t n_samples, int32_t n_features, const int32_t *col_ptr, const int32_t *row_idx, const float *values,
                     int32_t n_outputs, const uint8_t *n_classes, const uint8_t *y, int32_t n_trees, const int32_t *sample_counts,
                     const uint32_t *rand_state, int32_t max_features);
// The same ranges per problem of a batch; the message names the offending problem.
int forest_fit_batch_check(int32_t n_problems, int32_t n_features, int32_t n_outputs, int32_t n_trees, int32_t max_features,
                           const ForestProblem *problems);
// n_problems x n_trees workgroups in one launch; out[k] is what problem k alone gives, bit for bit.  `lone`: the batch of one
// behind gecco_crf_forest_fit (its message prefix).  On failure no forest is returned.
int forest_fit_batch(int32_t device, int32_t n_problems, int32_t n_features, int32_t n_outputs, int32_t n_trees,
                     int32_t max_features, const ForestProblem *problems, bool lone, std::vector<std::unique_ptr<Forest>> *out);
int forest_export(const Forest *f, int32_t tree, int32_t *left, int32_t *right, int32_t *feature, double *threshold,
                  double *impurity, int32_t *n_node_samples, double *weighted_n_node_samples, double *value);
// Argument checks of gecco_crf_forest_predict_batch (no device needed).
int forest_predict_batch_check(const Forest *const *f, int32_t n_problems, const int32_t *n_rows, const double *const *x,
                               double *const *posit);
// Forest k scores its n_rows[k] rows x[k] into posit[k]: one launch and one download; the rows of each block are uploaded
// from the caller's buffer as they are.
int forest_predict_batch(const Forest *const *f, int32_t n_problems, const int32_t *n_rows, const double *const *x,
                         double *const *posit);

}  // namespace gecco
