// Training objective of the 2-label linear-chain CRF on the device (gecco_crf_trainer_*, gecco_crf_trainer_batch_*,
// gecco_crf_trainer_grid_*, include/gecco_crf.h): the negative log-likelihood of every training window ([EXT] CRFsuite
// crf1d_encode's objective, without the regularisation terms the host optimiser adds) and its gradient with respect to
// the generated features.  There is one path: a Trainer holds training sets and problems over them, created by
// trainer_create and evaluated by trainer_eval.  The three C families differ in argument shape only: a lone trainer is
// one set with one problem, a batch is problem k on set k with one window and step.
#pragma once
#include <cstdint>
#include <vector>

namespace gecco {

struct Trainer;
struct TrainerGeneral;

// One problem's training set as a trainer builds it on the host: the arrays it uploads and what eval needs afterwards.
struct HostProblem {
    int32_t A = 0, n_items = 0, K = 0;
    int64_t n_win = 0;
    std::vector<int32_t> state_fid, trans_fid;  // [A*L], [L*L]: feature id of every dense slot, or -1
    std::vector<double> empirical;              // [K] observed feature counts over all windows
    std::vector<int32_t> item_ptr, attr_id, label, win_start, iw_first, iw_cnt, iw_off, attr_ptr, attr_items;
    std::vector<int32_t> win_len;  // whole-sequence instances only: the items of instance q (win_start[q] is its first)
    // problems with attribute values only: the values parallel to attr_id, and parallel to attr_items
    std::vector<double> attr_value, attr_item_value;
    // problems with sequence weights only: the weight of every instance's sequence, parallel to win_start
    std::vector<double> inst_weight;
};

// Checks one problem (the lone trainer's checks and messages) and builds its windows, coverage, empirical counts and
// attribute -> items transpose.  max_labels = 2: the 2-label families (any other num_labels is "only 2-label models");
// larger: the general family, num_labels in [2, max_labels] and labels in [0, num_labels).  whole_sequences: the
// instances are the sequences themselves (window and step are not read; a sequence without items is refused), listed in
// win_start / win_len longest first, ties by index; iw_first / iw_off are not built.  attr_value: null, or the value of every
// attribute entry (parallel to attr_id; a NaN or infinite one is refused): the empirical count of a state feature is then the
// sum of value x coverage over its entries, in item and CSR order, and attr_value / attr_item_value are built.  seq_weight: null,
// or one weight per sequence (checked by the caller): every empirical term is multiplied by the weight of its sequence (state:
// value x coverage x weight, transition: the weight per covered pair), in the same order, and inst_weight is built.
int build_problem(const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                  const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                  const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, int32_t max_labels,
                  HostProblem *hp, bool whole_sequences = false, const double *attr_value = nullptr,
                  const double *seq_weight = nullptr);

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

// The general-label family (gecco_crf_trainer_general_*, crf_train_general.hip): the same objective for 2 to 32 labels,
// problem k with its own label count, window and step.  Errors carry "trainer general: problem k: ".  attr_value (the
// *_create_valued entries): null, or per problem the values of its attribute entries, entry k null for a problem without.
// allowed (the *_create_partial entries): null, or per problem one mask per item, bit y set when label y is allowed, entry k
// null for a labelled problem.  A problem with masks minimises log Z - log Z_A; its labels[k] is not read,
// and a mask of 0 or with a bit at or above its label count is refused on the host, naming the problem and the item.
// seq_weight / label_cost (the *_create_weighted entries): null, or per problem one weight >= 0 per sequence /
// the label-cost matrix [L][L], row = gold, >= 0 with a zero diagonal; entry k null: weights of 1 / no costs.  Such a problem
// minimises sum over instances of omega * (log Z_C - score(gold)), Z_C over state scores s_t[y'] + C[y_t][y'].  A weight or cost
// that is negative or not finite, a non-zero diagonal and costs on a problem with masks are refused on the host.
int trainer_general_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                           const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                           const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                           const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                           TrainerGeneral **out, const double *const *attr_value = nullptr,
                           const uint32_t *const *allowed = nullptr, const double *const *seq_weight = nullptr,
                           const double *const *label_cost = nullptr);
int trainer_general_eval(TrainerGeneral *t, const uint8_t *active, const double *const *w, double *f, double *const *g);
int32_t trainer_general_num_problems(const TrainerGeneral *t);
int64_t trainer_general_num_windows(const TrainerGeneral *t, int32_t k);
int64_t trainer_general_scratch_bytes(const TrainerGeneral *t, int32_t k);  // (k = -1: the sum over the problems)
void trainer_general_destroy(TrainerGeneral *t);

// The whole-sequence family (gecco_crf_trainer_sequences_*, crf_train_general.hip): the general family's objective with one
// instance per sequence, of that sequence's length (any length >= 1).  The handle is a TrainerGeneral whose problems have
// no window: eval, num_problems, scratch_bytes and destroy are the general family's, and num_windows counts the
// sequences.  Errors carry "trainer sequences: problem k: ".
int trainer_sequences_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                             const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                             const int32_t *num_attrs, const int32_t *num_labels, const int32_t *const *state_fid,
                             const int32_t *const *trans_fid, const int32_t *num_features, TrainerGeneral **out,
                             const double *const *attr_value = nullptr, const uint32_t *const *allowed = nullptr,
                             const double *const *seq_weight = nullptr, const double *const *label_cost = nullptr);

}  // namespace gecco
