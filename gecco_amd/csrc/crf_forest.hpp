// Random-forest fit and predict of GECCO's cluster type classifier (gecco_crf_forest_*, include/gecco_crf.h).
#pragma once
#include <cstdint>
#include <vector>

namespace gecco {

// Range of gecco_crf_forest_fit: one workgroup per tree keeps the tree's sample and feature arrays in LDS.
constexpr int32_t kForestMaxSamples = 4096;
constexpr int32_t kForestMaxFeatures = 8192;
constexpr int32_t kForestMaxOutputs = 64;

struct Forest {
    int32_t device = 0;
    int32_t n_trees = 0, n_features = 0, n_outputs = 0, max_n_classes = 1, cap = 0;  // cap: node slots per tree (2 n - 1)
    std::vector<uint8_t> n_classes;
    std::vector<int32_t> node_count, max_depth;
    // device, [n_trees][cap] (value: [n_trees][cap][n_outputs][max_n_classes])
    int32_t *d_left = nullptr, *d_right = nullptr, *d_feature = nullptr, *d_n_node = nullptr;
    double *d_threshold = nullptr, *d_impurity = nullptr, *d_weighted = nullptr, *d_value = nullptr;
    uint8_t *d_ncls = nullptr;
    ~Forest();
};

// Argument checks of gecco_crf_forest_fit (no device needed): GECCO_CRF_OK or GECCO_CRF_EINVAL with a message.
int forest_fit_check(int32_t n_samples, int32_t n_features, const int32_t *col_ptr, const int32_t *row_idx, const float *values,
                     int32_t n_outputs, const uint8_t *n_classes, const uint8_t *y, int32_t n_trees, const int32_t *sample_counts,
                     const uint32_t *rand_state, int32_t max_features);
int forest_fit(int32_t device, int32_t n_samples, int32_t n_features, const int32_t *col_ptr, const int32_t *row_idx,
               const float *values, int32_t n_outputs, const uint8_t *n_classes, const uint8_t *y, int32_t n_trees,
               const int32_t *sample_counts, const uint32_t *rand_state, int32_t max_features, Forest **out);
int forest_export(const Forest *f, int32_t tree, int32_t *left, int32_t *right, int32_t *feature, double *threshold,
                  double *impurity, int32_t *n_node_samples, double *weighted_n_node_samples, double *value);
int forest_predict(const Forest *f, int32_t n_rows, const double *x, double *posit);

}  // namespace gecco
