// Training objective of the 2-label linear-chain CRF on the device (gecco_crf_trainer_*, gecco_crf_trainer_batch_*,
// include/gecco_crf.h): the negative log-likelihood of every training window ([EXT] CRFsuite crf1d_encode's objective,
// without the regularisation terms the host optimiser adds) and its gradient with respect to the generated features.
// One Trainer holds K problems; a lone trainer is K = 1 of the same kernels.
#pragma once
#include <cstdint>

namespace gecco {

struct Trainer;

// Arguments as gecco_crf_trainer_create; returns GECCO_CRF_* (message via set_error).
int trainer_create(int32_t device, const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                   const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                   const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, Trainer **out);
// Arguments as gecco_crf_trainer_batch_create: one entry per problem in every array.
int trainer_batch_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                         const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                         const int32_t *num_attrs, const int32_t *num_labels, int32_t window, int32_t step,
                         const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                         Trainer **out);
// Arguments as gecco_crf_trainer_grid_create: one entry per set in the set arrays, problem k on set problem_set[k].
int trainer_grid_create(int32_t device, int32_t n_sets, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                        const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                        const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                        const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                        int32_t n_problems, const int32_t *problem_set, int64_t scratch_budget_bytes, Trainer **out);
int trainer_eval(Trainer *t, const double *w, double *f, double *g);
// (a grid's evaluation too)
int trainer_batch_eval(Trainer *t, const uint8_t *active, const double *const *w, double *f, double *const *g);
int32_t trainer_num_problems(const Trainer *t);
int64_t trainer_num_windows(const Trainer *t, int32_t k);
// Scratch bytes of problem k; k = -1: the work space allocated (the most one group may use).  -1 for a bad k.
int64_t trainer_scratch_bytes(const Trainer *t, int32_t k);
void trainer_destroy(Trainer *t);

}  // namespace gecco
