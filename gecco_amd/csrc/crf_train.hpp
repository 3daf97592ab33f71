// Training objective of the 2-label linear-chain CRF on the device (gecco_crf_trainer_*, gecco_crf_trainer_batch_*,
// gecco_crf_trainer_grid_*, include/gecco_crf.h): the negative log-likelihood of every training window ([EXT] CRFsuite
// crf1d_encode's objective, without the regularisation terms the host optimiser adds) and its gradient with respect to
// the generated features.  There is one path: a Trainer holds training sets and problems over them, created by
// trainer_create and evaluated by trainer_eval.  The three C families differ in argument shape only: a lone trainer is
// one set with one problem, a batch is problem k on set k with one window and step.
#pragma once
#include <cstdint>

namespace gecco {

struct Trainer;

// Sets as gecco_crf_trainer_grid_create takes them (one entry per set in the set arrays, each with its own window and
// step), problem k on set problem_set[k], or on set k where problem_set is NULL (then n_problems == n_sets).
// scratch_budget_bytes <= 0: every problem fits in one group.  `family` names the caller in error messages ("batch",
// "grid"); NULL is the lone trainer, whose messages carry no prefix.  Returns GECCO_CRF_* (message via set_error).
int trainer_create(int32_t device, int32_t n_sets, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                   const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                   const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                   const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                   int32_t n_problems, const int32_t *problem_set, int64_t scratch_budget_bytes, const char *family,
                   Trainer **out);
// f[k] and g[k] of every problem with active[k] != 0 under the weights w[k]; the other entries are not touched.
int trainer_eval(Trainer *t, const uint8_t *active, const double *const *w, double *f, double *const *g);
int32_t trainer_num_problems(const Trainer *t);
int64_t trainer_num_windows(const Trainer *t, int32_t k);
// Scratch bytes of problem k; k = -1: the work space allocated (the most one group may use).  -1 for a bad k.
int64_t trainer_scratch_bytes(const Trainer *t, int32_t k);
void trainer_destroy(Trainer *t);

}  // namespace gecco
