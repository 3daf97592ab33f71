/*
 * gecco_crf.h -- C ABI of the MI355X-native linear-chain CRF inference engine for GECCO's
 * `gecco.crf` hot path.
 *
 * This is the drop-in boundary: the native interface GECCO reaches today for this path is
 * python-crfsuite's `Tagger` ([EXT] CRFsuite 0.12 `crfsuite_tagger_t`: open / labels / set /
 * marginal_point / viterbi), crossed once per sliding window at
 *     /root/reference/gecco/crf/__init__.py:253   self.model.predict_marginals_single(feats[win])
 * inside the per-contig window loop at :244-258.  The entry points below replace that
 * per-window boundary with one call per *batch of contigs*; the reference-side binding a
 * maintainer would add (a ctypes stub inside a `ClusterCRF` subclass handed to
 * `gecco.cli.main(crf_type=...)`, gecco/cli/commands/__init__.py:127-137) is shown in
 * INTEGRATION.md and implemented in gecco_amd/crf.py.
 *
 * Conventions: plain pointers and sizes; every function returns an int status (0 = OK,
 * <0 = error, text via gecco_crf_last_error()); caller owns all buffers.  Model handles are
 * immutable after creation and may be shared between threads; a plan may be launched from several
 * threads (its lazily created work space is guarded), but concurrent launches of ONE plan share that
 * work space and must therefore go to one stream; sessions serialise their batches.  Batches are CSR:
 *   contig_ptr[n_contigs+1]  gene offsets of each contig          (host memory, always)
 *   gene_ptr  [n_genes+1]    attribute offsets of each gene
 *   attr_id   [nnz]          attribute ids; ids outside [0, num_attrs) count as unknown attributes
 *                            and carry no weight, as names CRFsuite does not know do
 * Genes are in the reference's order: sorted by (contig id, start) -- crf/__init__.py:199.
 * There is NO CPU fallback in this library: without a HIP device the compute entry points
 * return GECCO_CRF_ENODEV.
 */
#ifndef GECCO_CRF_H
#define GECCO_CRF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GECCO_CRF_OK 0
#define GECCO_CRF_EINVAL (-1)       /* bad argument; window errors mirror _meta.py:127-130 */
#define GECCO_CRF_EFORMAT (-2)      /* malformed CRFsuite model blob */
#define GECCO_CRF_ENOMEM (-3)
#define GECCO_CRF_EHIP (-4)         /* HIP runtime error */
#define GECCO_CRF_ENODEV (-5)       /* no usable HIP device */
#define GECCO_CRF_EUNSUPPORTED (-6) /* model/window shape outside every kernel's range */

typedef struct gecco_crf_model gecco_crf_model;
typedef struct gecco_crf_plan gecco_crf_plan;

/* Thread-local description of the last error returned on this thread. */
const char *gecco_crf_last_error(void);
/* ABI version: major*100 + minor*10 + patch (2.10.0 = 300, 2.11.0 = 310, 2.12.0 = 320, 2.13.0 = 330, 2.14.0 = 340).
 * ABI 2.15.0 adds the *_constrained one-shots and keeps 340: the new entries are detected by symbol presence.
 * ABI 2.16.0 adds gecco_crf_span_probabilities in the same way, ABI 2.17.0 gecco_crf_sample_paths, ABI 2.18.0
 * gecco_crf_viterbi_kbest, ABI 2.19.0 gecco_crf_edge_posteriors, ABI 2.20.0 gecco_crf_viterbi_min_run, ABI 2.21.0
 * gecco_crf_run_posteriors, ABI 2.22.0 gecco_crf_marginals_min_run, ABI 2.23.0 gecco_crf_run_counts, ABI 2.24.0
 * gecco_crf_span_conditionals, ABI 2.25.0 gecco_crf_max_marginals, ABI 2.26.0 the *_create_weighted trainers, ABI 2.27.0
 * gecco_crf_viterbi_run_length and gecco_crf_marginals_run_length, ABI 2.28.0 gecco_crf_ring. */
int gecco_crf_version(void);

/* ---- model (replaces [EXT] pycrfsuite.Tagger.open / labels() / info(); the blob is the
 * `__FILE_RESOURCE_DATA__` bytes held by the pickle that ClusterCRF.trained() loads,
 * gecco/crf/__init__.py:61-99) ------------------------------------------------------- */
int gecco_crf_model_load(const uint8_t *lcrf, size_t n_bytes, gecco_crf_model **out);
/* Model from dense tables (row-major state[A][L], trans[L][L]); names are "0".."L-1" and
 * "a<id>".  Used for synthetic benchmark models. */
int gecco_crf_model_from_tables(const double *state, const double *trans, int32_t num_attrs,
                                int32_t num_labels, gecco_crf_model **out);
void gecco_crf_model_free(gecco_crf_model *m);
int32_t gecco_crf_model_num_labels(const gecco_crf_model *m);
int32_t gecco_crf_model_num_attrs(const gecco_crf_model *m);
int32_t gecco_crf_model_num_features(const gecco_crf_model *m); /* state + transition */
const char *gecco_crf_model_label_name(const gecco_crf_model *m, int32_t id); /* NULL if out of range */
const char *gecco_crf_model_attr_name(const gecco_crf_model *m, int32_t id);
int32_t gecco_crf_model_label_id(const gecco_crf_model *m, const char *name); /* -1 if unknown */
int32_t gecco_crf_model_attr_id(const gecco_crf_model *m, const char *name);  /* -1 if unknown */
/* Bulk name->id (ids[i] = -1 for names the model does not know). */
int gecco_crf_model_map_attrs(const gecco_crf_model *m, const char *const *names, int32_t n, int32_t *ids);
/* Dense weights; `present` (may be NULL) flags which entries are actual model features
 * ([EXT] CRF.state_features_ / transition_features_ list only those). */
int gecco_crf_model_state_weights(const gecco_crf_model *m, double *w /* A*L */, uint8_t *present /* A*L */);
int gecco_crf_model_trans_weights(const gecco_crf_model *m, double *w /* L*L */, uint8_t *present /* L*L */);
/* Two-label models: the per-attribute factor table behind the window kernels' slot constants, as the devices get it (host
 * only, no device needed).  pairs: A + 1 entries (delta_a, exp(delta_a)), delta_a = w[a][label] - w[a][1 - label]; the last
 * entry is the neutral pair (0, 1) of attribute ids outside the dictionary.  dmax = max |delta_a|; prod_max_cnt = floor(700 /
 * dmax) (0 from dmax >= 700 on, INT32_MAX for dmax == 0).  Any output may be null.  gecco_crf_slot_prod_max_cnt: the rule alone. */
int gecco_crf_model_slot_table(const gecco_crf_model *m, int32_t label, double *pairs /* 2*(A+1) */, double *dmax, int32_t *prod_max_cnt);
int32_t gecco_crf_slot_prod_max_cnt(double dmax);

/* ---- devices ---------------------------------------------------------------------- */
int gecco_crf_device_count(int32_t *n);

/* ---- one-shot, host buffers in / host buffers out, synchronous ----------------------
 * Row W (+D,S,A/B,P): p_out[g] = max over sliding windows covering gene g of
 * P(y_g = label) from an independent forward-backward on each window of `window` genes
 * (gecco/crf/__init__.py:209-258).  Contigs shorter than the window are centre-padded
 * with empty genes when pad != 0, else skipped and their genes get NaN ("no prediction",
 * :228-234,246-248).  Genes covered by no window (step > 1) get 0.0 (:251). */
int gecco_crf_windowed_marginals(const gecco_crf_model *m, int32_t device,
                                 const int32_t *contig_ptr, int32_t n_contigs,
                                 const int32_t *gene_ptr, const int32_t *attr_id,
                                 int32_t window, int32_t step, int32_t label, int32_t pad,
                                 double *p_out /* n_genes */);
/* Row W for EVERY label in one pass (ABI 2.11, additive; crf_general_windowed.hip): the windows, padding, centring and
 * `step` of gecco_crf_windowed_marginals, one forward-backward per window.
 *   p_all[g][l] = max over the windows covering gene g of P_w(y_g = l)            (row-major [n_genes][L])
 *   p_any[g]    = max over the same windows of sum_{l != background} P_w(y_g = l)  (label-index order)
 * Every value of both outputs lies in [0, 1], exactly 1 at the most.
 * p_any is what a caller whose label 'background' means "in no cluster" thresholds: the maximum of a sum is not a sum of
 * maxima, so it cannot be formed from the columns.  With 2 labels and background 0 it is column 1 bit for bit.
 * background == -1: no p_any, which must then be NULL; a buffer without a background label, a missing buffer with one,
 * and background >= L are GECCO_CRF_EINVAL.  Genes of skipped contigs hold NaN and genes no window covers 0.0 in every
 * column and in p_any, as in the single-label entry.  1 <= L <= 32 labels; windows of up to 48 genes (up to 32 at 2 to 4
 * labels when the lane-per-window kernel serves the model), GECCO_CRF_EUNSUPPORTED beyond -- the single-label entry's
 * 2-label kernels have no such limit.
 * A gene's results depend on its own contig only: the same contig alone or inside any batch gives the same bits.
 * One device per call (there is no batch-driver form of this entry). */
int gecco_crf_windowed_marginals_all(const gecco_crf_model *m, int32_t device,
                                     const int32_t *contig_ptr, int32_t n_contigs,
                                     const int32_t *gene_ptr, const int32_t *attr_id,
                                     int32_t window, int32_t step, int32_t background /* label id, or -1 */, int32_t pad,
                                     double *p_all /* [n_genes][L] */, double *p_any /* [n_genes], NULL iff background == -1 */);
/* Row F (extension; [EXT] CRF.predict_marginals_single on a whole contig): marginals of
 * every label, marg[n_genes][L]; lognorm[n_contigs] may be NULL.
 * With 3 to 32 labels the sum-product kernels (this entry, every lattice query behind it, and the windowed entries) take
 * exp(transition weight): a model whose largest transition weight is outside [-700, 700] is GECCO_CRF_EINVAL.  Subtracting
 * a constant from every transition weight leaves the model's distribution unchanged.  Viterbi is not refused. */
int gecco_crf_marginals_full(const gecco_crf_model *m, int32_t device,
                             const int32_t *contig_ptr, int32_t n_contigs,
                             const int32_t *gene_ptr, const int32_t *attr_id,
                             double *marg, double *lognorm);
/* Row V (extension; [EXT] CRF.predict_single / crf1dc_viterbi): best label path per
 * contig, first-argmax tie-breaking; score[n_contigs] may be NULL. */
int gecco_crf_viterbi(const gecco_crf_model *m, int32_t device,
                      const int32_t *contig_ptr, int32_t n_contigs,
                      const int32_t *gene_ptr, const int32_t *attr_id,
                      int8_t *y_out /* n_genes */, double *score);
/* Row R (gecco/refine.py:51-64,118-200, criterion "gecco"): threshold run-length
 * segmentation with the stateful grouper, optional trimming of un-annotated edge genes and
 * validation.  seg_out rows = (contig, cluster_number, first_gene, last_gene_exclusive);
 * *n_seg receives the number of rows; GECCO_CRF_EINVAL if max_seg is too small.
 * carry_state: the grouper lives for one `iter_clusters` call (refine.py:186).  0 = one call per
 * contig, what the CLI does (cli/commands/_common.py:621-623): every contig starts "out".
 * 1 = one call over all contigs: a contig that starts with genes without probability inherits the
 * state the previous contig ended in. */
int gecco_crf_segment(int32_t device, const double *p, const uint8_t *annotated,
                      const int32_t *contig_ptr, int32_t n_contigs,
                      double threshold, int32_t n_cds, int32_t edge_distance, int32_t trim,
                      int32_t carry_state, int32_t *seg_out, int32_t max_seg, int32_t *n_seg);

/* ClusterRefiner's parameters (gecco/refine.py:75-116) for the *_ex entry points.  criterion 0 = "gecco"
 * (:142-156: annotated genes, and genes away from the contig edges, >= n_cds); 1 = "antismash" (:157-163: mean
 * probability of the member genes >= average_threshold, distinct marker domains among ALL their domains >=
 * n_biopfams, member genes >= n_cds).  The marker domains (the reference's BIO_PFAMS list, refine.py:19-27) come
 * as a CSR over the batch's genes: marker_ptr[n_genes+1], marker_id[...] in [0, 256) = index of the domain in the
 * caller's marker list; only read when criterion == 1 (gecco_crf_segment_ex wants marker_ptr[0] == 0; the batch driver and
 * the plan take any non-decreasing offsets, like gene_ptr).  (The mean is the left-to-right sum over the count;
 * numpy.mean's own last bit depends on the SIMD width numpy dispatches to, so the reference does not pin it.) */
typedef struct {
    double threshold;         /* 0.8 */
    double average_threshold; /* 0.6 */
    int32_t criterion;        /* 0 */
    int32_t n_cds;            /* 5 */
    int32_t n_biopfams;       /* 5 */
    int32_t edge_distance;    /* 0 */
    int32_t trim;             /* 1 */
    int32_t carry_state;      /* see gecco_crf_segment; the batch driver always works per contig */
    const int32_t *marker_ptr;
    const int32_t *marker_id;
} gecco_crf_refine_params;
int gecco_crf_segment_ex(int32_t device, const double *p, const uint8_t *annotated,
                         const int32_t *contig_ptr, int32_t n_contigs, const gecco_crf_refine_params *params,
                         int32_t *seg_out, int32_t max_seg, int32_t *n_seg);

/* Weighted domain composition of called clusters (gecco/model.py:458-503
 * `Cluster.domain_composition(all_possible, normalize)`, assembled per cluster for the type
 * classifier at gecco/types/__init__.py:118).  seg rows as written by gecco_crf_segment
 * (only first_gene / last_gene_exclusive are read); dom_ptr[n_genes+1] = CSR of the domain
 * rows of every gene in the order of `gene.protein.domains`; dom_col[row] = index of the
 * domain's name in all_possible or -1; dom_weight[row] = 1 - pvalue (or -log10, the caller's
 * choice as in the reference).  comp_out[n_seg][n_cols], every entry numpy.sum of the matching
 * weights and every row divided by `row.sum() or 1` when normalize != 0: bit-identical to
 * numpy's pairwise summation. */
int gecco_crf_domain_composition(int32_t device, const int32_t *seg, int32_t n_seg,
                                 const int32_t *dom_ptr, int32_t n_genes,
                                 const int32_t *dom_col, const double *dom_weight,
                                 int32_t n_cols, int32_t normalize, double *comp_out);

/* ---- resident / asynchronous API ----------------------------------------------------
 * A plan owns the device copies of the model tables and of the contig layout of one
 * batch; bulk arrays stay in caller-owned DEVICE memory and launches go to the caller's
 * stream (`stream` is a hipStream_t passed as void*; NULL = the default stream).  This is
 * what bench.py and multi-GPU drivers use: one plan per rank/shard, no collectives. */
int gecco_crf_plan_create(const gecco_crf_model *m, int32_t device,
                          const int32_t *contig_ptr /* host */, int32_t n_contigs,
                          int32_t window, int32_t step, int32_t pad, gecco_crf_plan **out);
void gecco_crf_plan_free(gecco_crf_plan *p);
int32_t gecco_crf_plan_num_genes(const gecco_crf_plan *p);
int64_t gecco_crf_plan_num_windows(const gecco_crf_plan *p); /* = the reference's progress `total` */
int32_t gecco_crf_plan_num_tiles(const gecco_crf_plan *p);   /* workgroups of the windowed kernel */
int32_t gecco_crf_plan_tile_out(const gecco_crf_plan *p);    /* output slots per workgroup of the windowed kernel */
/* Name of the kernel variant the plan dispatches to (for profiles / bench). */
const char *gecco_crf_plan_kernel_name(const gecco_crf_plan *p);
int gecco_crf_plan_run_windowed(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                int32_t label, double *d_p_out, void *stream);
/* gecco_crf_windowed_marginals_all on device buffers: d_p_all [n_genes][L], d_p_any [n_genes] or NULL (background == -1).
 * gecco_crf_plan_all_kernel_name: the kernel that call dispatches to ("gl_all_small": one lane per window, 2 to 8 labels
 * inside the range guard; "gl_all_groups": one group of lanes per window, everything else). */
int gecco_crf_plan_run_windowed_all(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                    int32_t background, double *d_p_all, double *d_p_any, void *stream);
const char *gecco_crf_plan_all_kernel_name(const gecco_crf_plan *p);
int gecco_crf_plan_run_marginals_full(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                      double *d_marg, double *d_lognorm, void *stream);
int gecco_crf_plan_run_viterbi(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                               int8_t *d_y, double *d_score, void *stream);
/* Windowed marginals (gecco/crf/__init__.py:244-258) and whole-contig Viterbi ([EXT]
 * CRF.predict_single) of the same batch in one pass over the CSR: the state scores
 * ([EXT] crf1dt_state_score) are accumulated once and shared.  Same outputs, bit for bit, as
 * gecco_crf_plan_run_windowed followed by gecco_crf_plan_run_viterbi; d_score may be NULL. */
int gecco_crf_plan_run_decode(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                              int32_t label, double *d_p_out, int8_t *d_y, double *d_score, void *stream);
/* The same decode, software-pipelined over a sequence of batches (throughput form): call k enqueues the windowed marginals
 * of batch k (plan p, its CSR arrays, d_p_out) and the Viterbi labels of batch k - 1 (plan `prev`, the plan of the
 * previous call -- it may be the same plan --, labels to d_prev_y) -- in ONE launch when both qualify (2-label model,
 * window 20, no contig longer than 2048 genes): the Viterbi workgroups, which leave the CUs idle when they run alone,
 * run under the window tiles of the next batch.  First call: prev = NULL.  Last call: p = NULL (labels of the last batch
 * only), so K batches take K + 1 calls.  Outputs are the bits of gecco_crf_plan_run_decode.  The caller keeps the CSR
 * arrays of a batch alive until the call that delivers its labels has been enqueued, and does not use `prev` for other
 * whole-contig calls in between (they would recompute the state scores; results stay correct). */
int gecco_crf_plan_run_decode_pipelined(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                        int32_t label, double *d_p_out, gecco_crf_plan *prev, int8_t *d_prev_y,
                                        void *stream);
/* Row R chained behind the marginals, on the same stream, without moving them: d_p (e.g. the output
 * of gecco_crf_plan_run_windowed) and d_annotated are device arrays over the plan's genes; rows go
 * to d_seg[max_seg][4] and their number to *d_n_seg, both device-accessible (device memory, or
 * memory from gecco_crf_host_alloc).  The reference runs this right behind predict_probabilities
 * (cli/commands/_common.py:595-625 -> refine.py:118-200). */
int gecco_crf_plan_run_segment(gecco_crf_plan *p, const double *d_p, const uint8_t *d_annotated,
                               double threshold, int32_t n_cds, int32_t edge_distance, int32_t trim,
                               int32_t carry_state, int32_t *d_seg, int32_t max_seg, int32_t *d_n_seg,
                               void *stream);
/* Same with the full parameter set; marker_ptr / marker_id are DEVICE arrays over the plan's genes. */
int gecco_crf_plan_run_segment_ex(gecco_crf_plan *p, const double *d_p, const uint8_t *d_annotated,
                                  const gecco_crf_refine_params *params, int32_t *d_seg, int32_t max_seg,
                                  int32_t *d_n_seg, void *stream);
/* Average milliseconds per launch of `iters` back-to-back windowed launches, measured with
 * HIP events on `stream` (after `warmup` untimed launches). */
int gecco_crf_plan_time_windowed(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                 int32_t label, double *d_p_out, void *stream,
                                 int32_t warmup, int32_t iters, float *ms_per_launch);
/* The same for gecco_crf_plan_run_windowed_all. */
int gecco_crf_plan_time_windowed_all(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                     int32_t background, double *d_p_all, double *d_p_any, void *stream,
                                     int32_t warmup, int32_t iters, float *ms_per_launch);
/* The same for the pipelined decode launch (the plan following itself: window tiles of the batch + Viterbi workgroups of
 * the batch before, one launch per iteration); the interval includes the boundaries between the launches. */
int gecco_crf_plan_time_decode_pipelined(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                         int32_t label, double *d_p_out, int8_t *d_y, void *stream, int32_t warmup,
                                         int32_t iters, float *ms_per_launch);
/* What the 2-label Viterbi decoder of this plan has met since the last call with reset != 0 (waits for the device):
 * out[0] decisions inside the coarse margin of their threshold (candidates), out[1] decisions inside the margin in which the
 * difference form is not provably [EXT] crf1dc_viterbi's, out[2] contigs decoded again with CRFsuite's own recursion
 * because of those, out[3] the genes of these contigs.  All zero for models the any-label kernels serve. */
int gecco_crf_plan_viterbi_stats(gecco_crf_plan *p, int64_t out[4], int32_t reset);

/* ---- batch driver: host buffers in, host buffers out, one or several devices ----------------
 * What `gecco run` reaches through ClusterCRF.predict_probabilities (gecco/crf/__init__.py:244-258:
 * one loop iteration per contig, nothing shared).  A session owns, per device, a ring of lanes
 * (stream + reusable plan + device buffers); a batch is cut into chunks at contig boundaries, the
 * chunks are dealt to the devices longest-first by gene count (per-GPU queues, no collective), and
 * chunk k+1 is uploaded while chunk k computes and chunk k-1 is downloaded.  Host buffers from
 * gecco_crf_host_alloc (pinned) make every copy asynchronous; any other host memory works too.
 * Nothing is allocated once a session has seen its largest chunk.  One batch at a time per session
 * (calls are serialised); free a session before its model.  The one-shot entry points above run on
 * a per-device session owned by the model. */
typedef struct gecco_crf_session gecco_crf_session;
int gecco_crf_host_alloc(size_t n_bytes, void **out);
void gecco_crf_host_free(void *p);
int gecco_crf_session_create(const gecco_crf_model *m, const int32_t *devices, int32_t n_devices,
                             gecco_crf_session **out);
void gecco_crf_session_free(gecco_crf_session *s);
int gecco_crf_session_set_chunk_genes(gecco_crf_session *s, int32_t genes); /* default 2^19 */
/* Small batches -- what `gecco run` on ONE genome hands over: a contig of a few dozen genes, BASELINE.json configs[0],
 * /root/reference/tests/test_cli/test_run.py:35-70 -- take the DIRECT path: the batch is one chunk, its arrays are read by the
 * kernels from pinned host memory (the caller's own buffers when they come from gecco_crf_host_alloc and are large enough for
 * that to matter, a pinned staging copy otherwise) and its outputs are written there; no copy command, no second stream, the
 * call is its launches and one wait (input arrays of 256 KB and more are copied to device memory by a copy command on that same
 * stream).  `genes` = largest batch that takes it (half of that for cluster calls; 0 = never; never more than the chunk size;
 * -1 = the defaults: every batch that is one chunk anyway -- 2^19 genes -- on a one-device session, 131072 on a session over
 * several devices, 65536 for cluster calls).  Same output bits as the chunked path up to the last ulp of the 0.3 % of windows
 * that take the max-normalised form (reference-bits mode: the same bits).  Whole-contig marginals and path
 * scores always take the chunked path. */
int gecco_crf_session_set_direct_genes(gecco_crf_session *s, int32_t genes);
/* Figures of the last batch (any pointer may be NULL). */
int gecco_crf_session_stats(const gecco_crf_session *s, int32_t *n_chunks, int64_t *h2d_bytes,
                            int64_t *d2h_bytes, double *host_plan_seconds, double *wall_seconds);
/* REFERENCE-BITS MODE.  The fast kernels reorganise CRFsuite's arithmetic; their probabilities lie within a few ulps of the
 * reference's (<= 13 on the BGC0001866 fixture) -- enough for bit-identical cluster calls, not for the reference's own acceptance
 * test, which compares whole output files (/root/reference/galaxy/gecco.xml:83-111; probabilities are printed with 16-17
 * digits).  With this switch on, the session's windowed marginals -- and so its cluster calls and the p of its decode calls --
 * are computed in CRFsuite's OWN operation order ([EXT] crf1dc_exp_state / alpha_score / beta_score / marginal_point as
 * restated in oracle/crf_oracle.c) with a CORRECTLY ROUNDED exp in place of libm's.  What that is and is not: bit-identical to
 * the oracle run with a correctly rounded exp (libquadmath) on every gene, string-identical to the reference's fixture files
 * (85 of 85 float cells); against the oracle run with the host's glibc exp -- what CRFsuite calls -- 2 881 of 1 999 989 genes of
 * the C3 benchmark batch differ, by at most 14 ulps (glibc's exp is not correctly rounded on every argument, and which ones
 * depends on its version and the CPU's FMA path); the fast kernels differ on 89 % of the genes, by at most 64 ulps.  About five
 * times the fast window kernel's time.  2-label models, windows of at most 32 genes (GECCO_CRF_EUNSUPPORTED otherwise).
 * GECCO_CRF_REFERENCE_BITS=1 (read once per process) switches it on for the windowed marginals of every 2-label session and plan
 * whose window it covers; other layouts keep their kernels. */
int gecco_crf_session_set_reference_bits(gecco_crf_session *s, int32_t on);
/* The exp that mode uses, on the host (a double-double evaluation; same code as the device's): out[i] = the double nearest to
 * exp(x[i]). */
int gecco_crf_exp_correctly_rounded(const double *x, int64_t n, double *out);
/* The same and more as one struct: whether the batch took the direct path, and the time the submitting host threads spent
 * issuing work (HIP API calls + chunk layouts), which is what bounds a session over many devices. */
typedef struct {
    int32_t n_chunks, n_devices, direct, host_threads;
    int64_t h2d_bytes, d2h_bytes;
    double host_plan_seconds, host_issue_seconds, wall_seconds;
} gecco_crf_session_stats_t;
int gecco_crf_session_stats_ex(const gecco_crf_session *s, gecco_crf_session_stats_t *out);
/* = gecco_crf_windowed_marginals over the session's devices. */
int gecco_crf_session_windowed(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                               const int32_t *gene_ptr, const int32_t *attr_id, int32_t window,
                               int32_t step, int32_t label, int32_t pad, double *p_out);
/* gecco_crf_session_windowed with a lighter wire format: `degree[i]` = gene_ptr[i + 1] - gene_ptr[i] as ONE BYTE per gene
 * (the caller guarantees the equality and that no gene has more than 255 domains; the packers know the counts anyway).
 * The degrees cross PCIe instead of the row pointers (2 instead of 8 MB per 2 M genes: a third of the upload); the row
 * pointers are rebuilt on the device by a prefix sum.  gene_ptr is still passed -- host memory, read at chunk boundaries
 * only.  Same output bits. */
int gecco_crf_session_windowed_degrees(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                       const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                       int32_t window, int32_t step, int32_t label, int32_t pad, double *p_out);
/* Windowed marginals + Viterbi labels of the same batch (state scores gathered once). */
int gecco_crf_session_decode(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                             const int32_t *gene_ptr, const int32_t *attr_id, int32_t window,
                             int32_t step, int32_t label, int32_t pad, double *p_out, int8_t *y_out);
/* gecco_crf_session_windowed (y_out NULL) / gecco_crf_session_decode with the compact wire format: `degree` (or NULL) =
 * the genes' domain counts as bytes, sent instead of the row pointers (gecco_crf_session_windowed_degrees); `attr_id16`
 * (or NULL) = the attribute indices as 16-bit words, read instead of attr_id, for a model with at most 65536 attributes
 * (EINVAL otherwise).  Same bits out. */
int gecco_crf_session_decode_wire(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                  const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                  const uint16_t *attr_id16, int32_t window, int32_t step, int32_t label, int32_t pad,
                                  double *p_out, int8_t *y_out /* or NULL */);
/* predict_probabilities + ClusterRefiner in one pass, one grouper per contig like the CLI
 * (cli/commands/_common.py:595-625): the probabilities never leave the device unless p_out is given;
 * what comes back is the rows (batch-wide contig / gene indices) and, if seg_p_out is given, the
 * probabilities of the genes of every row (row k at seg_off_out[k] .. seg_off_out[k+1]), which is
 * all a cluster table needs of them (average_p, max_p: gecco/model.py:442-454). */
int gecco_crf_session_clusters(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                               const int32_t *gene_ptr, const int32_t *attr_id, const uint8_t *annotated,
                               int32_t window, int32_t step, int32_t label, int32_t pad,
                               double threshold, int32_t n_cds, int32_t edge_distance, int32_t trim,
                               double *p_out /* n_genes or NULL */, int32_t *seg_out, int32_t max_seg,
                               int32_t *n_seg, double *seg_p_out /* or NULL */, int64_t max_seg_genes,
                               int64_t *seg_off_out /* max_seg + 1, with seg_p_out */);

/* Same with the full parameter set (host marker arrays over the batch's genes; carry_state is ignored). */
int gecco_crf_session_clusters_ex(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                  const int32_t *gene_ptr, const int32_t *attr_id, const uint8_t *annotated,
                                  int32_t window, int32_t step, int32_t label, int32_t pad,
                                  const gecco_crf_refine_params *params, double *p_out, int32_t *seg_out,
                                  int32_t max_seg, int32_t *n_seg, double *seg_p_out, int64_t max_seg_genes,
                                  int64_t *seg_off_out);
/* gecco_crf_session_clusters_ex with the degree-byte wire format of gecco_crf_session_windowed_degrees: `degree` crosses
 * PCIe instead of the row pointers.  Same rows, same probabilities.  With `degree`, `annotated` may be NULL: a gene then
 * counts as annotated iff it carries a domain the model knows (degree > 0), and nothing else is uploaded for it. */
int gecco_crf_session_clusters_degrees(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                       const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                       const uint8_t *annotated, int32_t window, int32_t step, int32_t label, int32_t pad,
                                       const gecco_crf_refine_params *params, double *p_out, int32_t *seg_out,
                                       int32_t max_seg, int32_t *n_seg, double *seg_p_out, int64_t max_seg_genes,
                                       int64_t *seg_off_out);

/* gecco_crf_session_clusters_degrees with one more option of the wire format: `attr_id16` (or NULL), the attribute indices
 * as 16-bit words, read instead of attr_id -- for a model with at most 65536 attributes (GECCO's has 2766; EINVAL
 * otherwise).  2 instead of 4 bytes per domain cross PCIe and are widened on the device.  Same rows, same probabilities. */
int gecco_crf_session_clusters_wire(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                    const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                    const uint16_t *attr_id16, const uint8_t *annotated, int32_t window, int32_t step,
                                    int32_t label, int32_t pad, const gecco_crf_refine_params *params, double *p_out,
                                    int32_t *seg_out, int32_t max_seg, int32_t *n_seg, double *seg_p_out,
                                    int64_t max_seg_genes, int64_t *seg_off_out);

/* ---- columnar host side: table columns -> CSR batch, called clusters -> clusters.tsv rows --------
 * Strings travel as Arrow-style columns: one byte buffer + int64 offsets[n+1] per column (what
 * pandas / polars / pyarrow hold them in).  gecco_crf_pack_columns does, on columns, what the reference
 * does on Gene objects before the tagger sees them: genes by (sequence_id, start) with ties in
 * first-appearance order (sorted() is stable, gecco/crf/__init__.py:199-206), a gene's domains by
 * domain_start (:200-201), repeated names collapsed (crf/features.py:31-35), names the model does not know
 * dropped ([EXT] CRFsuite attribute lookup).  Feature rows: one per domain hit (gecco/model.py:629-642);
 * gene rows (optional, so that genes without any domain are kept): one per gene (:781-789).  The CSR lands
 * in pinned memory when a device is present.  Pointers returned by the accessors live as long as the handle. */
typedef struct {
    const uint8_t *data;
    const int64_t *offsets;
} gecco_crf_strings;
typedef struct {
    int64_t n_rows; /* feature table */
    gecco_crf_strings sequence_id, protein_id, domain;
    const int64_t *start, *domain_start;
    int64_t n_genes; /* gene table, may be 0 */
    gecco_crf_strings gene_sequence_id, gene_protein_id;
    const int64_t *gene_start;
    int64_t n_markers; /* marker domain names for the antismash criterion (<= 256), may be 0 */
    gecco_crf_strings markers;
} gecco_crf_table_columns;
typedef struct gecco_crf_packed gecco_crf_packed;
typedef struct gecco_crf_cluster_rows gecco_crf_cluster_rows;
int gecco_crf_pack_columns(const gecco_crf_model *m, const gecco_crf_table_columns *t, gecco_crf_packed **out);
void gecco_crf_packed_free(gecco_crf_packed *p);
/* Sizes and diagnostics (any pointer may be NULL): duplicated ids in the gene table (the last row of an id
 * stands for it) and proteins of the feature table the gene table does not list -- the reference raises on
 * both (`annotate_genes`, gecco/cli/commands/_common.py), callers that mirror it check these. */
int gecco_crf_packed_info(const gecco_crf_packed *p, int32_t *n_genes, int32_t *n_contigs, int64_t *nnz,
                          int32_t *n_duplicate_gene_ids, int32_t *n_unlisted_proteins, int32_t *pinned);
const int32_t *gecco_crf_packed_contig_ptr(const gecco_crf_packed *p); /* [n_contigs+1] */
const int32_t *gecco_crf_packed_gene_ptr(const gecco_crf_packed *p);   /* [n_genes+1] */
const int32_t *gecco_crf_packed_attr_id(const gecco_crf_packed *p);    /* [nnz] */
const uint8_t *gecco_crf_packed_annotated(const gecco_crf_packed *p);  /* [n_genes] has >= 1 feature row */
const int64_t *gecco_crf_packed_gene_row(const gecco_crf_packed *p);   /* [n_genes] gene-table row, or -1 - first feature row */
const int32_t *gecco_crf_packed_row_gene(const gecco_crf_packed *p);   /* [n_rows] gene position of every feature row */
const int64_t *gecco_crf_packed_row_order(const gecco_crf_packed *p);  /* [n_rows] rows by (gene position, domain_start) */
const int64_t *gecco_crf_packed_row_ptr(const gecco_crf_packed *p);    /* [n_genes+1] */
/* per gene the distinct marker domains among its rows (index into `markers`); NULL without markers */
const int32_t *gecco_crf_packed_marker_ptr(const gecco_crf_packed *p); /* [n_genes+1] */
const int32_t *gecco_crf_packed_marker_id(const gecco_crf_packed *p);
/* Rows of clusters.tsv (gecco/model.py:731-760) for segments as returned by gecco_crf_session_clusters:
 * start / end over the member genes (gene_end: the gene table's `end`, feature_end: the feature table's),
 * average_p = statistics.mean of the members' probabilities, exactly rounded (:442-447), max_p, the sorted
 * protein ids and the sorted domain names joined by ';', "<sequence_id>_cluster_<number>". */
int gecco_crf_cluster_rows_build(const gecco_crf_packed *p, const gecco_crf_table_columns *t, const int64_t *gene_end,
                                 const int64_t *feature_end, const int32_t *seg, int32_t n_seg, const double *seg_p,
                                 const int64_t *seg_off, gecco_crf_cluster_rows **out);
void gecco_crf_cluster_rows_free(gecco_crf_cluster_rows *r);
const int64_t *gecco_crf_cluster_rows_start(const gecco_crf_cluster_rows *r);
const int64_t *gecco_crf_cluster_rows_end(const gecco_crf_cluster_rows *r);
const double *gecco_crf_cluster_rows_average_p(const gecco_crf_cluster_rows *r);
const double *gecco_crf_cluster_rows_max_p(const gecco_crf_cluster_rows *r);
/* which: 0 sequence_id, 1 cluster_id, 2 proteins, 3 domains */
int gecco_crf_cluster_rows_strings(const gecco_crf_cluster_rows *r, int32_t which, const uint8_t **data,
                                   const int64_t **offsets);
/* statistics.mean of the non-NaN values: the exact sum divided by the count, rounded once.  Any finite doubles of either
 * sign; infinite values follow float arithmetic (inf, -inf, NaN for both signs); NaN when there is no value. */
double gecco_crf_exact_mean(const double *v, int64_t n);
/* Output columns of the columnar path, on several host threads (ABI 2.2.1).  gather: out[i] = src[idx[i]] -- the feature
 * table's `cluster_probability` is its genes' probabilities (gecco/crf/features.py:92-96).  order_info, given the gene table's
 * `start` / `end` columns: rows_in_order = the genes in scoring order are the gene table's rows 0 .. n - 1 (the table can be
 * handed back as it is); refiner_order_differs = two genes of a contig share a start with their ends in decreasing order, so the
 * refiner's (start, end) order (gecco/refine.py:190) is not the CRF's (contig, start) order (gecco/crf/__init__.py:199). */
int gecco_crf_gather_f64(const double *src, int64_t n_src, const int32_t *idx, int64_t n, double *out);
int gecco_crf_packed_order_info(const gecco_crf_packed *p, const int64_t *gene_start, const int64_t *gene_end, int64_t n_gene_rows,
                                int32_t *rows_in_order, int32_t *refiner_order_differs);
/* TSV text of a table, the wire format either side of the path (gecco/_base.py:133-152): `header` first, then
 * n_rows lines of tab-separated cells.  kinds[c]: 0 text (data[c] bytes + offsets[c]), 1 int64, 2 float64; floats
 * are written with the shortest digits that round-trip, laid out as Python's repr() does, NaN as an empty field.
 * *out is malloc'ed: release it with gecco_crf_buffer_free. */
int gecco_crf_tsv_format(int64_t n_rows, int32_t n_cols, const int32_t *kinds, const void *const *data,
                         const int64_t *const *offsets, const char *header, uint8_t **out, int64_t *out_len);
void gecco_crf_buffer_free(uint8_t *p);

/* ---- training (ABI 2.3.0): objective and gradient of a 2-label CRF on the device ------------------------------
 * What `ClusterCRF.fit` (gecco/crf/__init__.py:275-378) hands to CRFsuite's L-BFGS trainer: the training instances are every
 * sliding window of `window` items, `step` apart, of every sequence (no padding: a sequence shorter than the window is EINVAL).
 * Sequences are CSR over items (seq_ptr[n_seqs+1], seq_ptr[0] = 0), items CSR over attributes (item_ptr[n_items+1],
 * attr_id in [0, num_attrs)), labels[n_items] in {0, 1}.  The host generates the features: state_fid[a*L + y] is the id of
 * the state feature (attribute a, label y) and trans_fid[i*L + j] that of the transition (i, j), -1 where there is none;
 * ids are in [0, num_features).  The training set is copied to `device` once and stays there; every array may be freed
 * after the call.  num_labels must be 2 and window at most 32 (GECCO_CRF_EUNSUPPORTED otherwise).
 * eval: f = sum over windows of (log Z - score of the gold path), g[k] = expected - empirical count of feature k, under
 * the weights w[num_features] (features absent from both tables weigh 0).  No regularisation terms.  Synchronous; every
 * sum has a fixed order, so equal weights give equal bits.  One evaluation at a time per trainer.  (A lone trainer is the
 * one-problem case of gecco_crf_trainer_batch_*, below: the same kernels.)
 * Range: correct for any finite weights.  Each window runs a scaled forward-backward (transitions max-shifted); a window
 * whose scaled intermediates leave the normal fp64 range (state-score gaps beyond ~708 nats, transition weights more
 * than ~708 apart) is recomputed in log space.  Non-finite weights give a non-finite f. */
typedef struct gecco_crf_trainer gecco_crf_trainer;
int gecco_crf_trainer_create(int32_t device, const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr,
                             const int32_t *attr_id, const int32_t *labels, int32_t num_attrs, int32_t num_labels,
                             int32_t window, int32_t step, const int32_t *state_fid, const int32_t *trans_fid,
                             int32_t num_features, gecco_crf_trainer **out);
int gecco_crf_trainer_eval(gecco_crf_trainer *t, const double *w, double *f, double *g);
int64_t gecco_crf_trainer_num_windows(const gecco_crf_trainer *t);
void gecco_crf_trainer_free(gecco_crf_trainer *t);

/* ---- training, several problems at once (ABI 2.5.0) --------------------------------------------------------------
 * K independent training sets resident on one device, evaluated together (cross-validation folds, for example).  Problem k
 * is exactly what gecco_crf_trainer_create takes: seq_ptr[k], n_seqs[k], item_ptr[k], attr_id[k], labels[k], num_attrs[k],
 * num_labels[k], state_fid[k], trans_fid[k], num_features[k]; all problems share `window` and `step`.  The single trainer's
 * checks apply to every problem, and the first bad problem is reported by its index ("problem k: ..." in the message).
 * Memory is about the sum of the lone trainers' (GECCO_CRF_ENOMEM, with nothing left allocated, when it does not fit).
 * eval: for every k with active[k] != 0, f[k] and g[k][num_features[k]] under the weights w[k][num_features[k]]; the
 * entries of inactive problems are neither read nor written (their w[k] and g[k] may be NULL).  One upload, six launches
 * whatever K is, one download; synchronous.
 * Bit contract: f[k] and g[k] are bitwise equal to gecco_crf_trainer_eval on a trainer built from problem k alone, with the
 * same w[k], whatever the other problems hold and whichever of them are active: every sum stays inside its problem, in the
 * lone trainer's order (a problem whose transitions force log space, or whose weights are not finite, affects no other).
 * num_windows(t, k): the windows of problem k (-1 for a bad k); num_problems: K. */
typedef struct gecco_crf_trainer_batch gecco_crf_trainer_batch;
int gecco_crf_trainer_batch_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                                   const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                                   const int32_t *num_attrs, const int32_t *num_labels, int32_t window, int32_t step,
                                   const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                                   gecco_crf_trainer_batch **out);
int gecco_crf_trainer_batch_eval(gecco_crf_trainer_batch *t, const uint8_t *active, const double *const *w, double *f,
                                 double *const *g);
int32_t gecco_crf_trainer_batch_num_problems(const gecco_crf_trainer_batch *t);
int64_t gecco_crf_trainer_batch_num_windows(const gecco_crf_trainer_batch *t, int32_t k);
void gecco_crf_trainer_batch_free(gecco_crf_trainer_batch *t);

/* ---- training, a grid of problems over shared training sets (ABI 2.8.0) ------------------------------------------
 * A hyperparameter search: n_sets training sets, each uploaded once, and n_problems problems, problem k on set
 * problem_set[k] with its own weights.  Set s is exactly what gecco_crf_trainer_create takes, with its own window[s] and
 * step[s]: seq_ptr[s], n_seqs[s], item_ptr[s], attr_id[s], labels[s], num_attrs[s], num_labels[s], window[s], step[s],
 * state_fid[s], trans_fid[s], num_features[s].  The lone trainer's checks apply to every set ("set s: ..." in the
 * message); a problem_set entry outside [0, n_sets) is EINVAL ("problem k: ...").
 * eval: as gecco_crf_trainer_batch_eval, w[k] and g[k] of num_features[problem_set[k]] entries.  Problems of one set
 * read its arrays once per launch (their item scores from one read of its attribute ids).  Each problem has its own
 * scratch (node marginals [windows][W][2], window rows, item scores and marginals: about 16 W + 40 bytes per window
 * plus 32 per item; num_windows and scratch_bytes give it).  The active problems are cut, in problem order, into groups
 * whose scratch together fits scratch_budget_bytes (a problem larger than the budget runs alone; <= 0: no limit), and
 * the groups run one after another: one upload, six launches per group, one download; synchronous.  Device memory is
 * the sets once plus the larger of the budget and the largest problem's scratch (at most the sum of all problems').
 * Bit contract: f[k] and g[k] are bitwise equal to gecco_crf_trainer_eval on a lone trainer built from set
 * problem_set[k], with the same w[k], whatever the other problems hold, which of them are active and however they are
 * grouped: every sum stays inside its problem, in the lone trainer's order (a problem whose transitions force log
 * space, or whose weights are not finite, affects no other).
 * num_windows(t, k): the windows of problem k's set (-1 for a bad k); scratch_bytes(t, k): problem k's scratch, and for
 * k = -1 the work space allocated; num_problems: n_problems. */
typedef struct gecco_crf_trainer_grid gecco_crf_trainer_grid;
int gecco_crf_trainer_grid_create(int32_t device, int32_t n_sets, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                                  const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                                  const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                                  const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                                  int32_t n_problems, const int32_t *problem_set, int64_t scratch_budget_bytes,
                                  gecco_crf_trainer_grid **out);
int gecco_crf_trainer_grid_eval(gecco_crf_trainer_grid *t, const uint8_t *active, const double *const *w, double *f,
                                double *const *g);
int32_t gecco_crf_trainer_grid_num_problems(const gecco_crf_trainer_grid *t);
int64_t gecco_crf_trainer_grid_num_windows(const gecco_crf_trainer_grid *t, int32_t k);
int64_t gecco_crf_trainer_grid_scratch_bytes(const gecco_crf_trainer_grid *t, int32_t k);
void gecco_crf_trainer_grid_free(gecco_crf_trainer_grid *t);

/* ---- training with 2 to 32 labels (ABI 2.10.0) -------------------------------------------------------------------
 * The same objective for any CRFsuite-style tagging task of 2 to 32 labels: n_problems independent problems resident on
 * one device, problem k with its own label count num_labels[k], window[k] and step[k]; the other arguments are
 * gecco_crf_trainer_batch_create's, with labels[k] in [0, num_labels[k]), state_fid[k] of num_attrs[k] * L and
 * trans_fid[k] of L * L entries (L = num_labels[k]).  The lone trainer's checks apply to every problem ("trainer
 * general: problem k: ..." in the message); num_labels outside 2..32 and windows outside 1..32 are
 * GECCO_CRF_EUNSUPPORTED.  The 2-label families above are unchanged and keep their own kernels; at num_labels = 2 this
 * family agrees with them to rounding, not to the bit.
 * eval: as gecco_crf_trainer_batch_eval (inactive entries neither read nor written; a problem without windows gives
 * f = 0, g = 0).  One upload, six launches per active problem, one download; synchronous.
 * Method: log-space forward-backward throughout (no scaled path, so no range conditions): correct for any finite weights;
 * non-finite weights give a non-finite f.  No float atomics: every sum has one fixed order that depends on neither the
 * device nor the other problems, so f[k] and g[k] are bitwise what a trainer built from problem k alone returns for
 * w[k], whichever problems are active, and two evaluations give the same bits.
 * Memory: per problem, item scores and item marginals [items][L], node marginals [windows][W][L] and one (1 + L * L)
 * block per 128 windows (the pairwise expectations are summed inside the workgroup; no L * L block per window);
 * scratch_bytes(t, k) gives it, k = -1 the sum that is allocated.
 * num_windows(t, k): the windows of problem k (-1 for a bad k); num_problems: n_problems. */
typedef struct gecco_crf_trainer_general gecco_crf_trainer_general;
int gecco_crf_trainer_general_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                                     const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                                     const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                                     const int32_t *step, const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                     const int32_t *num_features, gecco_crf_trainer_general **out);
int gecco_crf_trainer_general_eval(gecco_crf_trainer_general *t, const uint8_t *active, const double *const *w, double *f,
                                   double *const *g);
int32_t gecco_crf_trainer_general_num_problems(const gecco_crf_trainer_general *t);
int64_t gecco_crf_trainer_general_num_windows(const gecco_crf_trainer_general *t, int32_t k);
int64_t gecco_crf_trainer_general_scratch_bytes(const gecco_crf_trainer_general *t, int32_t k);
void gecco_crf_trainer_general_free(gecco_crf_trainer_general *t);

/* ---- training on whole sequences (ABI 2.12.0) ---------------------------------------------------------------------
 * CRFsuite's own training mode: one instance per sequence, of that sequence's length, for 2 to 32 labels:
 *     f(w) = sum over sequences of (log Z(sequence) - score(gold labels)),  g(w) = expected - empirical feature counts.
 * The arguments are gecco_crf_trainer_general_create's without window and step; a sequence may hold any number of items
 * from 1 up.  Refused on the host before any device work, with "trainer sequences: problem k: ..." in the message: a null
 * argument, num_labels outside 2..32 (GECCO_CRF_EUNSUPPORTED), a label outside [0, L), an attribute id outside [0, A), a
 * sequence of 0 items, a non-monotone seq_ptr or item_ptr, more than 2^31 workgroups in one launch.
 * eval: as gecco_crf_trainer_general_eval (a problem without sequences gives f = 0, g = 0).  One upload, five launches per
 * active problem, one download; synchronous.
 * Method: the general family's log-space forward-backward over each whole sequence, G lanes per sequence (G = the power of
 * two at or above L); the kernel's node marginals are the item marginals (every item lies in exactly one instance).  A
 * workgroup owns 256 / G sequences of the problem's slot order (by length, longest first, ties by index: computed on the
 * host from the problem alone) and runs them side by side.  No float atomics, every sum has one fixed order: f[k] and g[k] are bitwise what a trainer built
 * from problem k alone returns for w[k], whichever problems are active, and two evaluations give the same bits.
 * Cost: a sequence is sequential in its length (L exponentials per lane per step, forward and backward), so an evaluation
 * takes at least the time of the longest sequence; one very long sequence is correct but slow.
 * Memory: per problem 8 * (2 * items * L + (ceil(sequences / (256 / G)) + 32) * (1 + L * L)) bytes; scratch_bytes(t, k) gives
 * exactly that, k = -1 the sum that is allocated.  num_sequences(t, k): the sequences of problem k (-1 for a bad k). */
typedef struct gecco_crf_trainer_sequences gecco_crf_trainer_sequences;
int gecco_crf_trainer_sequences_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                                       const int32_t *const *item_ptr, const int32_t *const *attr_id,
                                       const int32_t *const *labels, const int32_t *num_attrs, const int32_t *num_labels,
                                       const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                       const int32_t *num_features, gecco_crf_trainer_sequences **out);
int gecco_crf_trainer_sequences_eval(gecco_crf_trainer_sequences *t, const uint8_t *active, const double *const *w, double *f,
                                     double *const *g);
int32_t gecco_crf_trainer_sequences_num_problems(const gecco_crf_trainer_sequences *t);
int64_t gecco_crf_trainer_sequences_num_sequences(const gecco_crf_trainer_sequences *t, int32_t k);
int64_t gecco_crf_trainer_sequences_scratch_bytes(const gecco_crf_trainer_sequences *t, int32_t k);
void gecco_crf_trainer_sequences_free(gecco_crf_trainer_sequences *t);

/* ---- real-valued attributes (ABI 2.13.0, additive) ------------------------------------------------------------------
 * CRFsuite's name:value items: every attribute entry carries a value, attr_value parallel to attr_id (same CSR positions),
 * a finite fp64 that may be negative or zero.  The state score of an item is s[y] = sum over its entries of v * w[a][y],
 * every term added as fma(v, w, acc) in CSR order; everything downstream of the state scores is the unvalued code.  The
 * model file stores no values, so models load and save as before.  Every entry above keeps its behaviour and its bits.
 *
 * Inference one-shots: the sibling's arguments plus attr_value (length nnz) after attr_id; one device per call, one plan
 * over the whole batch (no session, batch-driver or multi-device form).
 *   * A valued call always takes the any-L kernels (crf_general.hip), at 2 labels too; reference-bits mode and the
 *     GECCO_CRF_REFERENCE_BITS switch do not apply.  With every value 1.0 a model of 3 or more labels gives the bytes of the
 *     unvalued sibling; a 2-label model agrees with its specialised kernels to rounding.
 *   * Limits: 1 <= L <= 32.  gecco_crf_windowed_marginals_valued: windows of up to 48 genes at 2 labels and wherever the
 *     lane-group kernel serves the model, up to 32 / 20 / 32 genes at 3-4 / 5-8 / 9-32 labels under the lane-per-window
 *     kernels' transition guard (as the unvalued entry at 3 or more labels) -- so at 2 labels a window of more than 48
 *     genes, which the unvalued entry serves, is GECCO_CRF_EUNSUPPORTED here.  gecco_crf_windowed_marginals_all_valued:
 *     the limits of gecco_crf_windowed_marginals_all.
 *   * Viterbi: the chunked kernels' exactness margin bounds a partial sum of state scores by nnz * max|v| * max|w|, max|v|
 *     taken over the batch on the host; decisions inside the margin are decoded again by CRFsuite's sequential recursion.
 *   * Attribute ids outside [0, A) carry no weight, whatever their value.
 *   * Refused on the host before any device work, GECCO_CRF_EINVAL: a NaN or infinite value ("attribute value k is not
 *     finite"), a NULL attr_value with nnz > 0.
 * Trainers: gecco_crf_trainer_general_create / gecco_crf_trainer_sequences_create plus attr_value after attr_id; entry k
 * may be NULL, which makes problem k unvalued with the bits it has from the unvalued create.  eval, num_*, scratch_bytes
 * and free are the family's.  The objective keeps its form; the gradient of state feature (a, y) is the sum over instances
 * and items holding a of v * P(y_t = y) minus the sum of v * [y_t = y], the second summed on the host in one fixed order
 * (a double, no longer an integer).  A problem whose values are all 1.0 has the bytes of the unvalued problem.  A NaN or
 * infinite value is GECCO_CRF_EINVAL ("trainer general: problem k: trainer: attribute value j is not finite").
 * Memory: a valued problem's scratch_bytes grows by 8 * nnz (the values in attribute -> items order). */
int gecco_crf_windowed_marginals_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                        const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                        int32_t window, int32_t step, int32_t label, int32_t pad, double *p_out /* n_genes */);
int gecco_crf_windowed_marginals_all_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                            int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                            const double *attr_value, int32_t window, int32_t step,
                                            int32_t background /* label id, or -1 */, int32_t pad, double *p_all /* [n_genes][L] */,
                                            double *p_any /* [n_genes], NULL iff background == -1 */);
int gecco_crf_marginals_full_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                    const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value, double *marg,
                                    double *lognorm);
int gecco_crf_viterbi_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                             const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                             int8_t *y_out /* n_genes */, double *score);
int gecco_crf_trainer_general_create_valued(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                            const int32_t *n_seqs, const int32_t *const *item_ptr, const int32_t *const *attr_id,
                                            const double *const *attr_value, const int32_t *const *labels,
                                            const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                                            const int32_t *step, const int32_t *const *state_fid,
                                            const int32_t *const *trans_fid, const int32_t *num_features,
                                            gecco_crf_trainer_general **out);
int gecco_crf_trainer_sequences_create_valued(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                              const int32_t *n_seqs, const int32_t *const *item_ptr,
                                              const int32_t *const *attr_id, const double *const *attr_value,
                                              const int32_t *const *labels, const int32_t *num_attrs, const int32_t *num_labels,
                                              const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                              const int32_t *num_features, gecco_crf_trainer_sequences **out);

/* ---- partially labelled training sets (ABI 2.14.0, additive) ---------------------------------------------------------
 * Marginal-likelihood ("partial-label", "constrained-lattice") training: every item of a problem carries a set of allowed
 * labels A_t, one uint32_t with bit y set when label y is allowed (at 32 labels bit 31 is a label like any other), and
 *     f(w) = sum over instances of (log Z - log Z_A),    g(w) = E[feature counts] - E_A[feature counts],
 * Z_A and E_A over the label paths with y_t in A_t for every t; the instances are the family's (windows, or whole sequences).
 * With every set a singleton this is the labelled objective (to rounding: the operations differ); with every set full f and
 * g are 0.  The objective is not convex.  Log space throughout, right for any finite weights: a disallowed label is excluded
 * (an exact 0), not penalised.  No float atomics: an evaluation is bit-reproducible, and a problem's bits do not depend on its
 * neighbours.
 * The arguments of the *_create_valued sibling plus `allowed` after labels: allowed[k] holds one mask per item of problem k,
 * or is NULL, which makes problem k an ordinary labelled problem with the bits it has from the other creates.  For a problem
 * with masks labels[k] is not read and may be NULL.  attr_value may be NULL as a whole (no problem has values) or per problem;
 * a problem with masks and values uses the valued kernels like any other.  eval, num_*, scratch_bytes and free are the
 * family's.  Refused on the host before the device is looked at, GECCO_CRF_EINVAL, naming problem and item: a mask of 0
 * ("trainer general: problem k: item i allows no label"), a mask with a bit at or above num_labels[k].
 * Memory: a problem with masks adds the second pass's log alpha to its scratch_bytes: 8 * n_windows * window * L bytes
 * (whole sequences: 8 * n_items * L), and 4 bytes per item for the masks. */
int gecco_crf_trainer_general_create_partial(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                             const int32_t *n_seqs, const int32_t *const *item_ptr, const int32_t *const *attr_id,
                                             const double *const *attr_value, const int32_t *const *labels,
                                             const uint32_t *const *allowed, const int32_t *num_attrs, const int32_t *num_labels,
                                             const int32_t *window, const int32_t *step, const int32_t *const *state_fid,
                                             const int32_t *const *trans_fid, const int32_t *num_features,
                                             gecco_crf_trainer_general **out);
int gecco_crf_trainer_sequences_create_partial(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                               const int32_t *n_seqs, const int32_t *const *item_ptr,
                                               const int32_t *const *attr_id, const double *const *attr_value,
                                               const int32_t *const *labels, const uint32_t *const *allowed,
                                               const int32_t *num_attrs, const int32_t *num_labels,
                                               const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                               const int32_t *num_features, gecco_crf_trainer_sequences **out);

/* ---- cost-sensitive training: sequence weights and a label-cost matrix (ABI 2.26.0, additive; gecco_crf_version() stays 340) ----
 * Every sequence q of a problem carries a weight omega(q) >= 0, and the problem a cost matrix C[gold][predicted] >= 0 with a
 * zero diagonal ("softmax-margin"):
 *     f(w) = sum over instances of omega * (log sum over y' of exp(score(y') + sum_t C[y_t][y'_t]) - score(y)),
 *     g(w) = sum over instances of omega * (E_cost-augmented[feature counts] - empirical counts),
 * omega the weight of the sequence the instance was cut from (every window of it, or the whole sequence).  Both keep the
 * objective convex.  The partition function sees a wrong label y' at an item whose gold label is y as C[y][y'] better than it
 * is, so the optimum separates the gold path from costly mistakes by a margin.  Costs exist in training only: the model file
 * and every prediction path are unchanged.  Log space throughout; no float atomics: an evaluation is bit-reproducible, and a
 * problem's bits do not depend on its neighbours.
 * The arguments of the *_create_partial sibling plus, after `allowed`:
 *     seq_weight  const double *const *: per problem n_seqs[k] doubles.  NULL as a whole or per problem: weights of 1.
 *     label_cost  const double *const *: per problem L * L doubles, row = gold.  NULL as a whole or per problem: no costs.
 * attr_value and allowed may be NULL as a whole or per problem, as there.  A problem with neither weights nor costs is the
 * problem the other creates build, with their kernels and their bits.  A problem with masks takes weights only:
 * f = sum of omega * (log Z - log Z_A).  A weight of 0 is legal: the sequence contributes exact zeros.  eval, num_*,
 * scratch_bytes and free are the family's.  The empirical counts are weighted on the host in one fixed order (state feature:
 * value x coverage x omega; transition: omega per covered pair).
 * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, naming problem and index: a weight that is negative,
 * NaN or infinite ("trainer general: problem k: weight of sequence s is negative or not finite"), a cost that is negative, NaN
 * or infinite ("... cost [a][b] is negative or not finite"), a non-zero diagonal cost ("... cost [a][a] is on the diagonal and
 * not 0"), costs on a problem with masks ("... label costs on a problem with allowed-label masks").
 * Memory: a problem with weights or costs adds 8 bytes per instance (window, or sequence) to its scratch_bytes, and with costs
 * 8 * L * L more; that is exactly what create uploads for it. */
int gecco_crf_trainer_general_create_weighted(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                              const int32_t *n_seqs, const int32_t *const *item_ptr, const int32_t *const *attr_id,
                                              const double *const *attr_value, const int32_t *const *labels,
                                              const uint32_t *const *allowed, const double *const *seq_weight,
                                              const double *const *label_cost, const int32_t *num_attrs,
                                              const int32_t *num_labels, const int32_t *window, const int32_t *step,
                                              const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                              const int32_t *num_features, gecco_crf_trainer_general **out);
int gecco_crf_trainer_sequences_create_weighted(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                const int32_t *const *attr_id, const double *const *attr_value,
                                                const int32_t *const *labels, const uint32_t *const *allowed,
                                                const double *const *seq_weight, const double *const *label_cost,
                                                const int32_t *num_attrs, const int32_t *num_labels,
                                                const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                                const int32_t *num_features, gecco_crf_trainer_sequences **out);

/* ---- allowed-label sets at inference (ABI 2.15.0, additive; gecco_crf_version() stays 340) ----------------------------------
 * Constrained decoding: every gene carries a set of allowed labels, one uint32_t with bit y set when label y is allowed, as
 * the *_create_partial trainers define it (at 32 labels bit 31 is a label like any other).  A constrained call is the
 * unconstrained call on a lattice in which a disallowed (gene, label) pair has state score -infinity: excluded exactly, not
 * penalised.
 *   * Viterbi: CRFsuite's recursion (strict `<`, first arg max) on that table; the path never uses a disallowed label and
 *     score is its score.
 *   * Whole-sequence marginals: P(y_t = l | x, path inside the sets); a disallowed entry is exactly 0.0; lognorm is log Z_A,
 *     so lognorm_constrained - lognorm is the log-probability that the path lies inside the sets.
 *   * Windowed forms: an independent forward-backward per window on the restricted lattice, the per-gene maximum, p_any as
 *     before; padding items allow every label; a disallowed entry of p_out / p_all is exactly 0.0.
 * Arguments: the *_valued sibling's plus `allowed` after attr_value, one mask per gene, indexed like the rows of gene_ptr
 * (gene g of the caller's arrays: a batch with contig_ptr[0] > 0 reads allowed[contig_ptr[0]] first).  attr_value may be NULL
 * here: no values.  With values the state scores are the valued ones.  One device per call, one plan over the whole batch (no
 * session, batch-driver or multi-device form).
 *   * A constrained call takes the any-L kernels at every label count, like a valued one, with its limits (single-label
 *     windows of up to 48 genes at 2 labels); reference-bits mode does not apply.  With every mask full the results are the
 *     bytes of the any-L call without masks.  Results are right wherever the unconstrained call is right for the same model:
 *     the state scores are shifted by their maximum over the ALLOWED labels, so every gene keeps an emission of 1 and no
 *     range guard narrows.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL: a NULL allowed with at least one gene; a mask of
 *     0 ("constrained: gene i allows no label (a mask of 0)"); a mask with a bit at or above the model's label count. */
int gecco_crf_viterbi_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                  const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* or NULL */,
                                  const uint32_t *allowed, int8_t *y_out /* n_genes */, double *score);
int gecco_crf_marginals_full_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                         const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* or NULL */,
                                         const uint32_t *allowed, double *marg, double *lognorm);
int gecco_crf_windowed_marginals_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                             int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                             const double *attr_value /* or NULL */, const uint32_t *allowed, int32_t window,
                                             int32_t step, int32_t label, int32_t pad, double *p_out /* n_genes */);
int gecco_crf_windowed_marginals_all_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                 int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                 const double *attr_value /* or NULL */, const uint32_t *allowed, int32_t window,
                                                 int32_t step, int32_t background /* label id, or -1 */, int32_t pad,
                                                 double *p_all /* [n_genes][L] */, double *p_any /* [n_genes], NULL iff background == -1 */);

/* ---- region posteriors (ABI 2.16.0, additive; gecco_crf_version() stays 340) ------------------------------------------------
 * logp[q] = log P(y_t in S_q for every t in [begin_q, end_q) | x): the posterior probability, under the model and the whole
 * contig, that every gene of a span carries a label of a set.  It is a property of the path distribution, not a function of
 * the per-gene marginals.  The lattice is the whole-contig one of gecco_crf_marginals_full and gecco_crf_viterbi (not a
 * windowed one); with `allowed` (one mask per gene, as the *_constrained entries take them) it is the lattice restricted by
 * the masks, and the probability is conditional on the path lying inside them.  attr_value and allowed may each be NULL.
 *   * Span q is (span_contig[q], span_begin[q], span_end[q], span_mask[q]): a contig of the batch, gene offsets from that
 *     contig's first gene with the end exclusive, and a mask with bit y set when label y is in the set.  Offsets are relative
 *     to the contig, so a batch with contig_ptr[0] > 0 works as in the other one-shots.  Spans may overlap and repeat; equal
 *     queries give equal bits.
 *   * One forward-backward pass over the batch serves every span; a span then costs a sequential walk of its own genes by one
 *     group of lanes (a few hundred microseconds per thousand genes: spans are not chunked).  marg [n_genes][L] and lognorm
 *     [n_contigs], each optional, are the bytes gecco_crf_marginals_full (or its _valued / _constrained sibling, by the
 *     arguments given) writes for the batch.  (A 2-label model without values and masks has kernels of its own for those:
 *     asking for marg or lognorm there costs a second pass.)  n_spans == 0 is a valid call that fills marg and lognorm.
 *   * Results: logp <= 0.0; a set that holds every label gives exactly 0.0; -infinity where the probability is zero (some
 *     gene of the span allows no label of the set); never NaN.  Inside the span the state scores are shifted by their maximum
 *     over the SET, so a label outside the set that leads by hundreds costs its exact, finite amount.  The
 *     two genes bordering a span enter through the whole-contig pass's forward vector and marginals and inherit its range: a
 *     (gene, label) pair whose forward value underflowed there contributes nothing, as it contributes nothing to marg.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL with a message that names the span ("span q: ..."):
 *     a contig index outside the batch; begin < 0, begin >= end, or end beyond the contig's length (so a contig without genes
 *     holds no span); a mask of 0; a mask with a bit at or above the model's label count.  The checks of the *_valued and
 *     *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_span_probabilities(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                 const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                                 const uint32_t *allowed /* NULL: no masks */, const int32_t *span_contig,
                                 const int32_t *span_begin, const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans,
                                 double *logp /* [n_spans] */, double *marg /* [n_genes][L] or NULL */,
                                 double *lognorm /* [n_contigs] or NULL */);

/* ---- marginals given a region, and knock-out attributions (ABI 2.24.0, additive; gecco_crf_version() stays 340) ----------------
 * cond[r][l] = P(y_t = l | E, x), E the event "every gene of span q carries a label of its set": the marginals conditioned on a
 * region, for the genes of the span and `reach` genes on either side, on the lattice of gecco_crf_span_probabilities (whose
 * arguments, checks and refusals this entry shares, in the same words).  From them, exactly, what the region's log-probability
 * rests on: changing the state scores of ONE gene t by delta_l multiplies Z by sum_l marg_t(l) e^{delta_l} and Z_E by
 * sum_l cond_t(l) e^{delta_l}, so
 *     log P(E | x) - log P(E | x with the change) = log sum_l marg_t(l) e^{delta_l} - log sum_l cond_t(l) e^{delta_l}.
 *   * Rows.  Query q's rows are the genes max(begin - reach, 0) .. min(end + reach, T) of its contig of T genes, in gene order;
 *     the queries' rows follow each other in query order.  row_ptr [n_spans + 1] holds the cumulative row counts (row_ptr[0] = 0),
 *     occ_ptr [n_rows + 1] (optional) the cumulative numbers of attribute occurrences of the rows' genes, gene_ptr[g + 1] -
 *     gene_ptr[g] each.  The caller computes both -- they size its buffers -- and the library holds them to its own: a mismatch
 *     is GECCO_CRF_EINVAL, "span q: ...", before any device work.  So is reach < 0.
 *   * cond [n_rows][L].  A row sums to 1; inside the span an entry outside the set is exactly 0.0, and so is a disallowed (gene,
 *     label) pair anywhere.  A row is one fixed operation sequence: its bytes depend neither on reach, nor on the other queries,
 *     nor on the query's place in the batch; equal queries give equal bits.
 *   * item_contribution [n_rows] (optional): the change above for delta_l = -s_t(l), the gene without anything it carries (to
 *     the model a gene without domain hits).  attr_contribution [n_occ] (optional, needs occ_ptr): for delta_l = -v w[a][l], one
 *     occurrence of attribute a with value v taken out, for every occurrence of the row's gene in CSR order, valued or not (an
 *     id outside the model's dictionary has no weight: 0.0).  Positive when the region leans on it.  Each sum is shifted by its
 *     own largest delta: a |delta| of 1 000 does not overflow.  Labels without mass take no part.
 *   * logp [n_spans] has the bytes of gecco_crf_span_probabilities for the same queries (that kernel runs as it is); marg and
 *     lognorm, each optional, are as there.  Where logp[q] is -infinity the query's rows and contributions are all 0.0.  Never
 *     NaN.  n_spans == 0 is a valid call that fills marg and lognorm.
 *   * Range.  Inside the span the state scores are shifted by their maximum over the SET, and a row's own gene enters with its
 *     raw scores, so a label that leads by hundreds at the gene is knocked out exactly.  The other genes enter
 *     through the whole-contig pass's forward vector and marginals and inherit its range: a (gene, label) pair whose forward
 *     value underflowed there contributes nothing, as it contributes nothing to marg.
 *   * Cost: one forward-backward pass, the span kernel, two sequential walks per query (its span plus its reach on one side
 *     each) by one group of lanes, and one group of lanes per row; 8 (end - begin + rows) L bytes of device workspace per query.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_span_conditionals(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                                const uint32_t *allowed /* NULL: no masks */, const int32_t *span_contig,
                                const int32_t *span_begin, const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans,
                                int32_t reach, const int64_t *row_ptr /* [n_spans + 1] */,
                                const int64_t *occ_ptr /* [n_rows + 1] or NULL */, double *logp /* [n_spans] */,
                                double *cond /* [n_rows][L] */, double *item_contribution /* [n_rows] or NULL */,
                                double *attr_contribution /* [n_occ] or NULL */, double *marg /* [n_genes][L] or NULL */,
                                double *lognorm /* [n_contigs] or NULL */);

/* ---- label paths drawn from the posterior (ABI 2.17.0, additive; gecco_crf_version() stays 340) --------------------------------
 * y[g * n_samples + s] = the label of gene g in sample s: n_samples label paths per contig drawn from p(y | x) on the
 * whole-contig lattice of gecco_crf_marginals_full and gecco_crf_viterbi (not a windowed one), by forward filtering and backward
 * sampling.  With `allowed` (one mask per gene, as the *_constrained entries take them) the lattice is the restricted one: no
 * sample carries a disallowed label.  attr_value and allowed may each be NULL.  One forward-backward pass over the batch serves
 * every sample; the draws are parallel over samples and contigs and sequential along a contig (contigs are not chunked).
 *   * The rule.  alpha_t is the pass's forward vector at gene t (used as a direction: its scaling cancels), M = exp(trans).  A
 *     sample walks from its contig's last gene to its first.  With j the label drawn at gene t + 1, the weights are
 *     w_i = alpha_t(i) * M(i, j) (w_i = alpha_t(i) at the last gene), their running sums c_i = w_0 + ... + w_i in label order,
 *     and the label is the smallest i with c_i > u * c_{L-1}.  A label whose weight is exactly 0 is never drawn (a disallowed
 *     label, a transition with exp(trans) = 0, an underflowed alpha); where rounding leaves no such i, the label is the last i
 *     with w_i > 0.
 *   * The uniforms.  u comes from Philox4x32-10 (Salmon et al., Random123) with key (seed & 0xffffffff, seed >> 32) and counter
 *     (t, s, c, 0): t the gene's offset inside its contig, s the sample, c the contig's index in the batch.  From the output
 *     words x0, x1: u = double(((uint64_t)x0 << 21) ^ (x1 >> 11)) * 2^-53, in [0, 1).  No state is kept: equal arguments give
 *     equal bytes, and sample s of a contig does not depend on n_samples.
 *   * The fallback.  Where c_{L-1} is not > 0 or not finite -- every weight lost to underflow, which is outside the range
 *     gecco_crf_marginals_full documents -- the label is the first arg max of marg at that gene.  No label >= num_labels is
 *     ever written.
 *   * Run query q is (run_contig[q], run_anchor[q], run_mask[q]): a contig of the batch, a gene offset from that contig's first
 *     gene, and a mask with bit y set when label y is in the set.  runs[(q * n_samples + s) * 2 + {0, 1}] = (first, last + 1),
 *     offsets inside the contig, of the maximal run of genes around the anchor whose labels in sample s all lie in the set, or
 *     (-1, -1) where the anchor's own label does not.
 *   * Outputs.  y is int8 [n_genes][n_samples], gene-major; y == NULL is valid (the paths then live in device workspace only,
 *     for the runs).  runs is int32 [n_runs][n_samples][2], NULL iff n_runs == 0.  marg [n_genes][L] and lognorm [n_contigs],
 *     each optional, are the bytes gecco_crf_marginals_full (or its _valued / _constrained sibling, by the arguments given)
 *     writes for the batch.  (A 2-label model without values and masks has kernels of its own for those: asking for marg or
 *     lognorm there costs a second pass.)  Sizes are computed in size_t; a failed allocation is GECCO_CRF_ENOMEM.  A batch
 *     without genes writes nothing but lognorm = 0; contigs without genes and contig_ptr[0] > 0 work as in the other one-shots.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL with a message that names the argument or the run
 *     ("run q: ..."): n_samples outside 1 .. 2^20; a run's contig outside the batch; an anchor outside its contig (so a contig
 *     without genes holds no anchor); a mask of 0; a mask with a bit at or above the model's label count.  The checks of the
 *     *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_sample_paths(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                           const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                           const uint32_t *allowed /* NULL: no masks */, int32_t n_samples, uint64_t seed,
                           const int32_t *run_contig, const int32_t *run_anchor, const uint32_t *run_mask, int32_t n_runs,
                           int8_t *y /* [n_genes][n_samples] or NULL */, int32_t *runs /* [n_runs][n_samples][2], NULL iff n_runs == 0 */,
                           double *marg /* [n_genes][L] or NULL */, double *lognorm /* [n_contigs] or NULL */);

/* ---- the K best label paths with exact path scores (ABI 2.18.0, additive; gecco_crf_version() stays 340) ------------------------
 * y[g * k + r] = the label of gene g on the rank-r path of its contig, score[c * k + r] that path's score, n_paths[c] how many
 * ranks of contig c a path fills: the k highest-scoring label paths of every contig, in order, on the whole-contig lattice of
 * gecco_crf_viterbi and gecco_crf_marginals_full (not a windowed one).  exp(score - lognorm[c]) is a path's probability
 * p(y | x), exactly (not a share of draws).  With `allowed` (one mask per gene, as the *_constrained entries take them) the
 * lattice is the restricted one: no path carries a disallowed label, and lognorm is the restricted log Z.  attr_value and allowed
 * may each be NULL.  The walk is parallel over contigs and labels and sequential along a contig (contigs are not chunked).
 *   * The recursion.  For every (gene t, label j) the k best prefix scores in order, delta_t[j][0 .. k):
 *     delta_0[j] = [state_0[j]], and delta_t[j] holds the k best of (delta_{t-1}[i][r] + trans[i][j]) + state_t[j] over the
 *     source label i and the source rank r -- the operation order of gecco_crf_viterbi, so a path's score is the left-to-right
 *     sum of its terms, every addition rounded on its own.  Every source list is sorted: a step is an L-way merge that stops
 *     after k outputs.
 *   * The order is total.  Greater score first; among equal scores the smaller source label i, then the smaller source rank r;
 *     at the end of the contig the L final lists merge by the same rule (smaller last label, then smaller rank).  In exact
 *     arithmetic that is "score descending, then the reversed path (y_{T-1}, ..., y_0) ascending lexicographically".  Rank 0 is
 *     the path gecco_crf_viterbi (or its _valued / _constrained sibling) returns.
 *   * Empty ranks.  A candidate whose score is -infinity (a disallowed label on it) does not exist and is never emitted.  A rank
 *     that no path fills -- a contig of T genes has at most the product of its genes' allowed-label counts, L^T without masks --
 *     has score -infinity and label -1 at every gene of the contig; the filled ranks are 0 .. n_paths[c] - 1.
 *   * The prefix property.  The order is total and merges preserve it: rank r of a call with k' < k is rank r of the call with
 *     k, labels and score byte for byte.
 *   * Outputs.  y is int8 [n_genes][k], gene-major; score is double [n_contigs][k]; n_paths is int32 [n_contigs].  lognorm
 *     [n_contigs], optional, is the bytes gecco_crf_marginals_full (or its _valued / _constrained sibling, by the arguments
 *     given) writes for the batch.  (A 2-label model without values and masks has kernels of its own for that: asking for
 *     lognorm there costs a second pass.)  A contig without genes gets n_paths = 0, scores -infinity and lognorm 0.
 *     contig_ptr[0] > 0 works as in the other one-shots.  The back-pointers are workspace of n_genes * L * k * 2 bytes; sizes
 *     are computed in size_t; a failed allocation is GECCO_CRF_ENOMEM.
 *   * Limits: 1 <= k <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL: k outside 1 .. 32 ("viterbi_kbest: k = ... is
 *     outside 1 .. 32").  The checks of the *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_viterbi_kbest(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                            const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                            const uint32_t *allowed /* NULL: no masks */, int32_t k, int8_t *y /* [n_genes][k] */,
                            double *score /* [n_contigs][k] */, int32_t *n_paths /* [n_contigs] */,
                            double *lognorm /* [n_contigs] or NULL */);

/* ---- max-marginals (ABI 2.25.0, additive; gecco_crf_version() stays 340) ----------------------------------------------------------
 * through[g * L + l] = the score of the best label path of gene g's contig that gives gene g the label l, on the whole-contig
 * lattice of gecco_crf_viterbi and gecco_crf_viterbi_kbest (not a windowed one): to gecco_crf_viterbi what
 * gecco_crf_marginals_full is to the sum-product pass.  best[c] - through is how much worse the best reading becomes when a gene is
 * labelled differently.  These are score differences -- the log of the ratio of two single paths' probabilities --, not
 * posteriors.  With `allowed` (one mask per gene, as the *_constrained entries take them) the lattice is the restricted one.
 * attr_value and allowed may each be NULL.  The walks are parallel over contigs and labels and sequential along a contig
 * (contigs are not chunked); one more walk than gecco_crf_viterbi.
 *   * Definitions, for a contig of T genes with raw state scores s_t(l) (-infinity where `allowed` forbids) and raw transition
 *     weights A; every addition is rounded on its own, in the order written:
 *       forward    a_0(j) = s_0(j),   a_t(j) = max_i (a_{t-1}(i) + A(i, j)) + s_t(j)      (gecco_crf_viterbi's order)
 *       best[c]    = max_j a_{T-1}(j): the score bits of gecco_crf_viterbi_kbest's rank 0
 *       backward   b_{T-1}(i) = 0,    b_t(i) = max_j ((b_{t+1}(j) + s_{t+1}(j)) + A(i, j))
 *       through    = a_t(l) + b_t(l).  It is not clamped: under rounding it may differ from best[c] by a few ulps on the Viterbi
 *                  path; with weights whose sums are exact, max_l through_t(l) == best[c] at every gene.
 *   * Label sets.  set_mask[s], s < n_sets, has bit y set when label y is inside set s.  inside[g * n_sets + s] = the maximum of
 *     through[g][l] over the labels inside, outside[g * n_sets + s] over the labels not inside -- -infinity when that side is
 *     empty (a full set) or wholly disallowed.  A set's values do not depend on the other sets of the call.
 *   * Span queries.  Query q is (span_contig[q], span_begin[q], span_end[q], span_mask[q]) as gecco_crf_span_probabilities takes
 *     it: gene offsets from the contig's first gene, the end exclusive, bit y of the mask set when label y is in the set S.
 *       span_best[q]   = the best score of a path of the contig whose labels on [begin, end) all lie in S: v_begin(j) = a_begin(j)
 *                        for j in S and -infinity elsewhere, v_t(j) = max_i (v_{t-1}(i) + A(i, j)) + s_t(j) for j in S and
 *                        -infinity elsewhere, and the result max_j (v_{end-1}(j) + b_{end-1}(j));
 *       span_broken[q] = the best score of a path with at least one gene of the span outside S: the maximum of through[t][l] over
 *                        the genes t of the span and the labels l not in S.
 *     max(span_best, span_broken) is best[c] up to rounding.  A query's results depend on no other query.
 *   * -infinity and NaN.  A value is -infinity exactly where no such path exists (a disallowed label, a span gene that allows no
 *     label of S, a full S for span_broken), and never NaN.
 *   * Outputs.  through [n_genes][L], inside and outside [n_genes][n_sets], span_best and span_broken [n_spans] are each optional
 *     (NULL: not formed, and the others keep their bytes); best [n_contigs] is always written.  lognorm [n_contigs], optional, is
 *     the bytes gecco_crf_marginals_full (or its _valued / _constrained sibling, by the arguments given) writes for the batch, so
 *     that best[c] - lognorm[c] is the Viterbi path's log-probability.  The max walks need the state scores alone: the
 *     sum-product pass runs only when lognorm is asked for, and costs about as much as the two walks again; without it a model
 *     whose transitions lie outside that pass's range is taken.  (A 2-label model without values and masks has kernels of its own
 *     for lognorm: asking for it there costs a second pass.)  A contig without genes gets best = 0 (gecco_crf_viterbi's score),
 *     lognorm 0 and nothing else.  contig_ptr[0] > 0 works as in the other one-shots.  The two vectors are workspace of
 *     16 * n_genes * L bytes; sizes are computed in size_t; a failed allocation is GECCO_CRF_ENOMEM.  Equal calls give equal bytes
 *     (no atomics).
 *   * Limits: num_labels <= 32, 0 <= n_sets <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL with a message that starts "max_marginals:": n_sets
 *     outside 0 .. 32; a set mask of 0 or with a bit at or above num_labels ("max_marginals: set s: ..."); inside or outside given
 *     without a set; span_best or span_broken given without spans; a negative n_spans; a NULL array of a non-empty list; and,
 *     naming the query ("max_marginals: span q: ..."), the span checks of gecco_crf_span_probabilities.  The checks of the
 *     *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_max_marginals(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                            const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                            const uint32_t *allowed /* NULL: no masks */, const uint32_t *set_mask /* [n_sets] */, int32_t n_sets,
                            const int32_t *span_contig, const int32_t *span_begin, const int32_t *span_end,
                            const uint32_t *span_mask, int32_t n_spans, double *through /* [n_genes][L] or NULL */,
                            double *inside /* [n_genes][n_sets] or NULL */, double *outside /* [n_genes][n_sets] or NULL */,
                            double *span_best /* [n_spans] or NULL */, double *span_broken /* [n_spans] or NULL */,
                            double *best /* [n_contigs] */, double *lognorm /* [n_contigs] or NULL */);

/* ---- edge posteriors (ABI 2.19.0, additive; gecco_crf_version() stays 340) -----------------------------------------------------
 * The pairwise (edge) marginals xi_t(i, j) = P(y_{t-1} = i, y_t = j | x) on the whole-contig lattice of gecco_crf_viterbi and
 * gecco_crf_marginals_full (not a windowed one), and what follows from them, behind ONE forward-backward pass of the batch.  With
 * `allowed` (one mask per gene, as the *_constrained entries take them) the lattice is the restricted one, and a disallowed
 * (gene, label) pair contributes exact zeros everywhere.  attr_value and allowed may each be NULL.  Every output may be NULL: it
 * is then neither computed nor stored.  An edge depends on the two genes it joins only: the query is parallel over genes.
 *   * pair [n_genes][L][L]: pair[g][i][j] = xi of the edge entering gene g, all zeros for a contig's first gene.  8 L^2 bytes per
 *     gene (8 KB at 32 labels): ask for it only when the table itself is wanted.
 *   * enter, leave [n_genes][n_sets], for the label sets set_mask[0 .. n_sets) (bit y set: label y is inside):
 *     enter[g][s] = P(y_g in S and (g is its contig's first gene or y_{g-1} not in S)): a run of labels of S starts at g;
 *     leave[g][s] = P(y_g in S and (g is its contig's last gene or y_{g+1} not in S)): a run of labels of S ends at g.
 *     Sums of entries of xi, formed without storing pair; a set's values do not depend on the other sets or their order.
 *     The sum of enter over a contig is the expected number of runs of S on it, and equals the sum of leave.
 *   * transitions [n_contigs][L][L]: N(i, j) = sum over the contig's edges of xi(i, j); zeros for a contig of 0 or 1 genes.
 *   * entropy [n_contigs]: H(Y | x) of the contig's path distribution in nats, by the chain rule -- the entropy of the first
 *     gene's marginals plus, per edge, the entropy of every conditional row P(y_t = . | y_{t-1} = i) weighted by the marginal
 *     of i -- a sum of non-negative terms: never negative, never NaN, and small on a confident contig without cancellation.
 *     0 for a contig without genes.
 *   * marg [n_genes][L] and lognorm [n_contigs], optional, are the bytes gecco_crf_marginals_full (or its _valued /
 *     _constrained sibling, by the arguments given) writes for the batch.  (A 2-label model without values and masks has
 *     kernels of its own for that: asking for either there costs a second pass.)
 *   * Determinism: no floating-point atomics; a contig's sums are added in gene order in runs of 32 genes counted from the
 *     contig's first gene; equal calls give equal bytes.  contig_ptr[0] > 0 works as in the other one-shots.
 *   * Limits: 1 <= n_sets <= 32 (n_sets = 0 with enter = leave = NULL: no set is asked) and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL: n_sets outside that range, an empty mask, a mask
 *     with a bit at or above num_labels ("set 3: ..."), enter or leave without a set.  The checks of the *_valued and
 *     *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_edge_posteriors(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                              const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                              const uint32_t *allowed /* NULL: no masks */, const uint32_t *set_mask /* [n_sets] */, int32_t n_sets,
                              double *pair /* [n_genes][L][L] or NULL */, double *enter /* [n_genes][n_sets] or NULL */,
                              double *leave /* [n_genes][n_sets] or NULL */, double *transitions /* [n_contigs][L][L] or NULL */,
                              double *entropy /* [n_contigs] or NULL */, double *marg /* [n_genes][L] or NULL */,
                              double *lognorm /* [n_contigs] or NULL */);

/* ---- decoding under a minimum run length (ABI 2.20.0, additive; gecco_crf_version() stays 340) ----------------------------------
 * y[g] = the label of gene g on the best label path of its contig AMONG THE FEASIBLE ONES, score[c] that path's score, and
 * lognorm_min_run[c] = log Z_C, the log-mass of all feasible paths, on the whole-contig lattice of gecco_crf_viterbi and
 * gecco_crf_marginals_full (not a windowed one).  set_mask names a label set S (bit y set: label y is inside; S may be every
 * label).  A path is feasible when every maximal run of consecutive genes whose labels lie in S has at least min_run genes; runs
 * that touch the contig's first or last gene count like any other, and the labels inside a run may differ from gene to gene.
 * That is not the free Viterbi path with its short runs deleted: the model may prefer to stretch a run, or to merge two across a
 * gap.  exp(lognorm_min_run - lognorm) = P(no run shorter than min_run | x); exp(score - lognorm) is the path's probability,
 * exp(score - lognorm_min_run) its probability given the constraint.  With `allowed` (one mask per gene, as the *_constrained
 * entries take them) a path with a disallowed label does not exist, and lognorm is the restricted log Z.  attr_value and allowed
 * may each be NULL.  The walk is parallel over contigs and labels and sequential along a contig (contigs are not chunked).
 *   * The recursion runs on the lattice expanded by a run counter.  A label outside S has one state; a label j in S has the
 *     states (j, d), d = 1 .. min_run, d = min(run length so far, min_run); states are ordered by label, then by d.  At gene 0
 *     the states with d <= 1 (the outside states among them) start at state_0[j], the others at -infinity.  The sources of a
 *     destination at gene t: j outside S -- every label i, its one state if i is outside S, (i, min_run) alone if inside (a run
 *     may end only once it is long enough); (j, 1) -- the labels i outside S; (j, d) with 1 < d < min_run -- (i, d - 1), i in S;
 *     (j, min_run) -- (i, min_run - 1) and (i, min_run), i in S.  With min_run = 1 the expanded lattice is the plain one.  At
 *     the contig's end the outside states and the states (j, min_run) are admissible.
 *   * Max semiring: value = (delta[source] + trans[i][j]) + state_t[j] -- the operation order of gecco_crf_viterbi, so the score
 *     is the left-to-right sum of the path's terms, every addition rounded on its own.
 *   * The tie rule is operational.  A destination scans its sources in ascending (source label, source d) order with a strict
 *     `>` update; at the end the first arg max over the admissible states, in state order, wins.  This is a rule on expanded
 *     states and NOT "reversed path ascending" (no local rule can give that here: two expanded states stand for one label).
 *     With min_run = 1 it is gecco_crf_viterbi's rule: the same labels, and the score bits of gecco_crf_viterbi_kbest's rank 0.
 *   * Sum semiring: the same sources with a max-shifted log-sum-exp in place of the max, fp64 throughout; a destination all of
 *     whose sources are -infinity stays -infinity.  It runs only when lognorm_min_run is given, and asking for it changes no
 *     byte of y or score.
 *   * No feasible path (S every label and fewer than min_run genes, or masks that forbid it): score -infinity, label -1 at
 *     every gene of the contig, lognorm_min_run -infinity; never NaN.
 *   * Outputs.  y is int8 [n_genes]; score, lognorm_min_run (optional) and lognorm (optional) are double [n_contigs].  lognorm
 *     is the bytes gecco_crf_marginals_full (or its _valued / _constrained sibling, by the arguments given) writes for the
 *     batch.  (A 2-label model without values and masks has kernels of its own for that: asking for lognorm there costs a
 *     second pass.)  A contig without genes gets gecco_crf_viterbi's score, 0, and 0 for both log Z.  contig_ptr[0] > 0 works
 *     as in the other one-shots.  The back-pointers are workspace of n_genes * L * min_run bytes; sizes are computed in size_t;
 *     a failed allocation is GECCO_CRF_ENOMEM.  Equal calls give equal bytes (no atomics).
 *   * Limits: 1 <= min_run <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL: min_run outside 1 .. 32 ("viterbi_min_run: min_run
 *     = ... is outside 1 .. 32"), a set_mask of 0, a set_mask with a bit at or above num_labels ("set_mask 0: ...").  The checks
 *     of the *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_viterbi_min_run(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                              const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                              const uint32_t *allowed /* NULL: no masks */, uint32_t set_mask, int32_t min_run,
                              int8_t *y /* [n_genes] */, double *score /* [n_contigs] */,
                              double *lognorm_min_run /* [n_contigs] or NULL */, double *lognorm /* [n_contigs] or NULL */);

/* ---- marginals under a minimum run length (ABI 2.22.0, additive; gecco_crf_version() stays 340) ---------------------------------
 * marg[g][j] = P(gene g has label j | x, every maximal run of labels of S has at least min_run genes) and inside[g] = the sum of
 * marg[g] over the labels of S: how sure the model is of each gene AMONG THE FEASIBLE PATHS of gecco_crf_viterbi_min_run -- the
 * same set, the same feasibility, the same whole-contig lattice, `allowed` and attr_value as there.  These are not the free
 * marginals of gecco_crf_marginals_full, which give mass to paths with short runs: a lone high-scoring gene can have a free
 * marginal of 0.9 and a constrained one near 0.
 *   * A forward-backward on the lattice expanded by a run counter (the states, sources and admissible end states of
 *     gecco_crf_viterbi_min_run above), in log space with a max-shifted log-sum-exp per state, fp64 throughout.  The forward walk
 *     is the sum-semiring walk of gecco_crf_viterbi_min_run with its values kept: lognorm_min_run has that entry's bits.  The
 *     backward walk transposes the table: a state outside S is followed by every label outside S and by (k, 1), k in S; (i, d)
 *     with d < min_run by (k, d + 1), k in S, only; (i, min_run) by (k, min_run), k in S, and every label outside S.  beta is 0
 *     at the admissible states of the last gene; beta_t(s) = LSE over successors of trans[i][k] + state_{t+1}[k] + beta_{t+1}.
 *     marg[g][j] = the sum over d, ascending, of exp((alpha + beta) - lognorm_min_run).
 *   * Outputs.  marg is double [n_genes][num_labels] or NULL, inside double [n_genes] or NULL -- at least one of them; with marg
 *     NULL only 8 bytes per gene come back, and inside has the bytes it has when both are asked for.  lognorm_min_run
 *     [n_contigs] is required; lognorm [n_contigs] (optional) is the bytes gecco_crf_marginals_full (or its _valued /
 *     _constrained sibling, by the arguments given) writes for the batch, so exp(lognorm_min_run - lognorm) = P(no run shorter
 *     than min_run | x).  A disallowed (gene, label) pair gives exactly 0.0.  A contig without a feasible path gives 0.0 at every
 *     gene and lognorm_min_run -infinity; never NaN.  A contig without genes gets 0 for both log Z and nothing else.  A marginal
 *     is stored as computed: a sum over labels may differ from 1 by rounding.  contig_ptr[0] > 0 works as in the other one-shots.
 *   * The forward values are workspace of 8 * n_genes * num_labels * min_run bytes; sizes are computed in size_t; a failed
 *     allocation is GECCO_CRF_ENOMEM.  Equal calls give equal bytes (no atomics), and a contig's bytes do not depend on the
 *     other contigs of the batch.
 *   * Limits: 1 <= min_run <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, every message prefixed "marginals_min_run:": min_run
 *     outside 1 .. 32, a set_mask of 0 or with a bit at or above num_labels, marg and inside both NULL, lognorm_min_run NULL.
 *     The checks of the *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form); contigs are not chunked. */
int gecco_crf_marginals_min_run(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                                const uint32_t *allowed /* NULL: no masks */, uint32_t set_mask, int32_t min_run,
                                double *marg /* [n_genes][L] or NULL */, double *inside /* [n_genes] or NULL */,
                                double *lognorm_min_run /* [n_contigs] */, double *lognorm /* [n_contigs] or NULL */);

/* ---- circular contigs (ABI 2.28.0, additive; gecco_crf_version() stays 340) ----------------------------------------------------------
 * EVERY contig of the call is a RING: a complete chromosome or plasmid, whose last gene has a transition into its first.  (The
 * caller splits a mixed batch: the linear contigs go to the other entries.)  A ring of n >= 1 genes has n edges, t -> (t + 1) mod n,
 * all scored by the model's one transition table:
 *     score(y) = sum_t state_t[y_t] + sum_{t = 0 .. n-1} trans[y_t][y_{(t+1) mod n}]
 * so a ring of one gene has the self-edge trans[y_0][y_0] and a ring of two genes both trans[y_0][y_1] and trans[y_1][y_0].
 * lognorm_ring[c] = log Z_ring, the log-mass of all label paths of ring c; marg[g][j] = P(gene g has label j | x) on the ring; y the
 * ring's best path and score[c] its score, closing edge included.  None of them depends on where the ring was cut: rotating the
 * genes of a ring rotates marg and y and keeps lognorm_ring and score (up to rounding; exactly with integer weights and a unique
 * best path).  The chain entries do not have that property.  With `allowed` (one mask per gene, as the *_constrained entries take
 * them) a path with a disallowed label does not exist, and lognorm_ring is the restricted log Z.  attr_value and allowed may each
 * be NULL.  The walks are parallel over rings and labels and sequential along a ring (rings are not chunked).
 *   * Recursions.  Exact inference conditions on the start label a = y_0; the lattice is the whole-contig one expanded by a, and
 *     the L conditioned chains meet at the closing edge only.  With R the max-shifted log-sum-exp (sum semiring) or the max:
 *       F_0[a][j] = state_0[a] if j = a, else -infinity;   F_t[a][j] = R_i(F_{t-1}[a][i] + trans[i][j]) + state_t[j];
 *       closed[a] = R_j(F_{n-1}[a][j] + trans[j][a]);       log Z_ring = LSE_a closed[a];
 *       B_{n-1}[a][i] = trans[i][a];   B_t[a][i] = LSE_k((trans[i][k] + state_{t+1}[k]) + B_{t+1}[a][k]);
 *       marg[g][i] = the sum over a, ascending, of exp((F_t[a][i] + B_t[a][i]) - log Z_ring), at most 1.
 *     fp64 and log space throughout: any finite weights are right, and no transition range applies.  The whole-contig marginals
 *     of the chain do not run.
 *   * Decoding needs no L * L back-pointer table.  Pass one is a max-plus walk over all start labels without back-pointers; it
 *     leaves closed[a] = max_j(V_{n-1}[a][j] + trans[j][a]) and a* = its arg max.  Pass two is the Viterbi walk conditioned on
 *     y_0 = a*, with one byte of back-pointer per (gene, label); then the backtrack.  score has the bits of closed[a*]; values are
 *     (previous + trans) + state, every addition rounded on its own.
 *   * Tie rule.  Equal closed[a]: the smaller a.  Inside the conditioned walk: gecco_crf_viterbi's rule, sources in ascending label
 *     order with a strict `>` (the earlier source wins).  The last label is the first arg max of V_{n-1}[a*][j] + trans[j][a*].
 *   * Outputs that are not asked for are neither computed nor stored: the two max-plus passes run only for y (int8 [n_genes])
 *     and score (double [n_contigs]), which go together; the forward workspace and the backward walk only for marg (double
 *     [n_genes][num_labels]).  lognorm_ring (double [n_contigs]) is required, and asking for the others changes no byte of it,
 *     nor do they change each other's.  A disallowed (gene, label) pair gives exactly 0.0 in marg.  A ring without a feasible
 *     path gives lognorm_ring and score -infinity, 0.0 at every gene of marg and label -1 at every gene; never NaN.  A ring
 *     without genes gets 0 for lognorm_ring and score and nothing else.  contig_ptr[0] > 0 works as in the other one-shots.
 *   * Workspace: the forward values, 8 * n_genes * L * L bytes (and 8 bytes per gene and per ring behind them: the sum walks
 *     keep their values small by a shift per gene, which never enters a marginal), for marg only; the back-pointers,
 *     n_genes * L bytes, for y only.
 *     Sizes are computed in size_t; a failed allocation is GECCO_CRF_ENOMEM.
 *   * Determinism: no atomics.  Equal calls give equal bytes, and a ring's bytes do not depend on the other rings of the batch.
 *   * Limits: num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, every message prefixed "ring:": lognorm_ring NULL,
 *     y without score or score without y, more than 32 labels.  The checks of the *_valued and *_constrained entries apply to
 *     attr_value and allowed, with one exception: a mask of 0 is taken here, and the ring of such a gene has no feasible path.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form); rings are not chunked. */
int gecco_crf_ring(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                   const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                   const uint32_t *allowed /* NULL: no masks */, int8_t *y /* [n_genes] or NULL */,
                   double *score /* [n_contigs] or NULL */, double *marg /* [n_genes][L] or NULL */,
                   double *lognorm_ring /* [n_contigs] */);

/* ---- run-length potentials: decoding (ABI 2.27.0, additive; gecco_crf_version() stays 340) ---------------------------------------
 * A score on the LENGTH of a run, on the whole-contig lattice of gecco_crf_viterbi and gecco_crf_marginals_full (not a windowed
 * one).  set_mask names a label set S as in gecco_crf_viterbi_min_run, and a run is that entry's: a maximal stretch of genes
 * whose labels lie in S; runs that touch the contig's first or last gene count like any other, and the labels inside a run may
 * differ.  length_score[0 .. max_length - 1] = g[1 .. M] and tail = tau are each finite or -infinity.  For a path y whose runs
 * have n_r genes,
 *     score_g(y) = score(y) + sum over runs of ( g[min(n_r, M)] + tau * max(n_r - M, 0) ),
 * and a term of -infinity makes the path infeasible.
 *     g = 0, tau = 0                                 the plain lattice
 *     M = m, g = (-inf, ..., -inf, 0), tau = 0       gecco_crf_viterbi_min_run with min_run = m
 *     tau = -inf                                     a maximum run length M
 *     anything else                                  a soft duration model
 * y[g] = the label of gene g on the path of its contig with the largest score_g, score[c] = that score_g, lognorm_run_length[c]
 * = log Z_g, the log-mass of all paths under score_g.  exp(score - lognorm_run_length) is the path's probability under the
 * extended model; lognorm_run_length - lognorm compares the two models' masses.  attr_value and allowed as in
 * gecco_crf_viterbi_min_run.  The walk is parallel over contigs and labels and sequential along a contig (not chunked).
 *   * States: gecco_crf_viterbi_min_run's, with M for min_run.  The exit aggregate of a source label scores a run where it ends:
 *     A_t(i) = (+)_d (alpha_t(i, d) + g[d]) for i in S, alpha_t(i) for i outside.  The sources of a destination at gene t: j
 *     outside S -- A_{t-1}(i) + trans[i][j], every label i; (j, 1) -- alpha_{t-1}(i) + trans[i][j], i outside S, and at M = 1
 *     also (alpha_{t-1}(i, 1) + tau) + trans[i][j], i in S; (j, d), 1 < d < M -- alpha_{t-1}(i, d - 1) + trans[i][j], i in S;
 *     (j, M), M > 1 -- (i, M - 1) likewise and (alpha_{t-1}(i, M) + tau) + trans[i][j], i in S; then + state_t[j].  The total is
 *     (+)_i A_{T-1}(i): a run that reaches the last gene is scored like any other.
 *   * Max semiring: ((delta + g or tau) + trans) + state, every addition rounded on its own.  With integer weights and scores
 *     every output equals enumeration bit for bit; with g = 0, tau = 0 the score is gecco_crf_viterbi_kbest's rank 0; with the
 *     min-run table the score and the labels are gecco_crf_viterbi_min_run's.
 *   * The tie rule is operational, as in gecco_crf_viterbi_min_run: a destination scans its sources in ascending label order, a
 *     label's tau source directly behind its other one, with a strict `>` update; the aggregate scans d ascending with a strict
 *     `>`; at the end the smaller label wins among equal aggregates.  A rule on expanded states, not an order on paths.
 *   * Sum semiring: the same sources and aggregates with a max-shifted log-sum-exp, fp64 throughout; a destination all of whose
 *     sources are -infinity stays -infinity.  It runs only when lognorm_run_length is given, and changes no byte of y or score.
 *   * No feasible path: score -infinity, label -1 at every gene of the contig, lognorm_run_length -infinity; never NaN.
 *   * Outputs.  y is int8 [n_genes]; score, lognorm_run_length (optional) and lognorm (optional) are double [n_contigs], lognorm
 *     the bytes of gecco_crf_marginals_full (or its sibling by the arguments given).  A contig without genes gets score 0 and 0
 *     for both log Z.  The back-pointers are workspace of n_genes * L * (M + 1) bytes: gecco_crf_viterbi_min_run's byte per
 *     (gene, label, d) and one per (gene, label), the arg max d of the aggregate.  Equal calls give equal bytes (no atomics).
 *   * Limits: 1 <= max_length <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, every message prefixed "viterbi_run_length:":
 *     max_length outside 1 .. 32, a NaN or +infinity in length_score or tail, a set_mask of 0 or with a bit at or above
 *     num_labels, score NULL.  The checks of the *_valued and *_constrained entries apply to attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_viterbi_run_length(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                 const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                                 const uint32_t *allowed /* NULL: no masks */, uint32_t set_mask, int32_t max_length,
                                 const double *length_score /* [max_length] */, double tail, int8_t *y /* [n_genes] */,
                                 double *score /* [n_contigs] */, double *lognorm_run_length /* [n_contigs] or NULL */,
                                 double *lognorm /* [n_contigs] or NULL */);

/* ---- run-length potentials: marginals and expected length counts (ABI 2.27.0, additive; gecco_crf_version() stays 340) ----------
 * marg[g][j] = P_g(gene g has label j | x), inside[g] = the sum of marg[g] over the labels of S, under the extended model of
 * gecco_crf_viterbi_run_length (the same arguments, the same lattice), and counts[c][0 .. M]: counts[c][d - 1] = the expected
 * number of runs with min(length, M) = d, d = 1 .. M, and counts[c][M] = the expected number of tail steps, sum of max(length - M,
 * 0).  These are the derivatives of log Z_g by g[d] and by tau: with observed counts they are the gradient of a convex fit of
 * the length scores.
 *   * A forward-backward on the run-counter lattice in log space, fp64 throughout.  The forward walk is the sum-semiring walk of
 *     gecco_crf_viterbi_run_length with its values kept: lognorm_run_length has that entry's bits.  Backward, per source i in S:
 *     the exit continuation E_t(i) = LSE over k outside S of (trans[i][k] + state_{t+1}[k]) + beta_{t+1}(k), 0 at the last gene;
 *     the stay continuation C_t(i, d) = LSE over k in S of (trans[i][k] + state_{t+1}[k]) + beta_{t+1}(k, min(d + 1, M));
 *     beta_t(i, d) = LSE(g[d] + E, C), at d = M LSE(g[M] + E, tau + C).  marg[g][j] = the sum over d, ascending, of exp((alpha +
 *     beta) - lognorm_run_length).  counts[d] adds exp(((alpha_t(i, d) + g[d]) + E_t(i)) - log Z_g), counts[M + 1] adds
 *     exp((alpha_t(i, M) + (tau + C_t(i, M))) - log Z_g), per lane in walk order, reduced across the labels once per contig.
 *   * Outputs.  marg double [n_genes][num_labels], inside double [n_genes], counts double [n_contigs][max_length + 1], each or
 *     NULL, at least one of them; asking for one changes no byte of another.  lognorm_run_length [n_contigs] is required;
 *     lognorm [n_contigs] is optional.  A disallowed (gene, label) pair gives exactly 0.0.  A contig without a feasible path
 *     gives 0.0 everywhere and lognorm_run_length -infinity; never NaN.  A contig without genes gets 0 for both log Z and zeros
 *     in counts.  With tau = -infinity counts[c][M] is exactly 0.0.
 *   * The forward values are workspace of 8 * n_genes * num_labels * max_length bytes.  Equal calls give equal bytes (no
 *     atomics), and a contig's bytes do not depend on the other contigs of the batch.
 *   * Limits: 1 <= max_length <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, every message prefixed "marginals_run_length:":
 *     max_length outside 1 .. 32, a NaN or +infinity in length_score or tail, a set_mask of 0 or with a bit at or above
 *     num_labels, marg, inside and counts all NULL, lognorm_run_length NULL.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form); contigs are not chunked. */
int gecco_crf_marginals_run_length(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                   const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                                   const uint32_t *allowed /* NULL: no masks */, uint32_t set_mask, int32_t max_length,
                                   const double *length_score /* [max_length] */, double tail,
                                   double *marg /* [n_genes][L] or NULL */, double *inside /* [n_genes] or NULL */,
                                   double *counts /* [n_contigs][max_length + 1] or NULL */,
                                   double *lognorm_run_length /* [n_contigs] */, double *lognorm /* [n_contigs] or NULL */);

/* ---- run counts (ABI 2.23.0, additive; gecco_crf_version() stays 340) --------------------------------------------------------------
 * How many runs a contig holds, and the best path with a given number of them, on the whole-contig lattice of gecco_crf_viterbi
 * and gecco_crf_marginals_full (not a windowed one).  set_mask names a label set S (bit y set: label y is inside; S may be every
 * label).  N_S(y) is the number of maximal runs of consecutive genes whose labels lie in S; runs that touch the contig's first or
 * last gene count like any other, and the labels inside a run may differ from gene to gene (gecco_crf_viterbi_min_run's notion
 * of a run).  With K = max_runs, for every contig c and k = 0 .. K:
 *     log_mass[c][k] = the log of the summed exp(score) over the paths with N_S = k for k < K, and with N_S >= K for k = K (the
 *                      saturating tail slot);
 *     score[c][k]    = the score of the best such path, and plane k of y its labels.
 * log P(N_S = k | x) = log_mass[c][k] - LSE over k' of log_mass[c][k']: normalised by the recursion's own total the probabilities
 * sum to 1 to rounding, and that total equals lognorm to rounding.  exp(score[c][k] - lognorm[c]) is the path's probability.
 * The best path with exactly one run is not the free Viterbi path with its surplus runs deleted, or with two runs merged by
 * hand.  With `allowed` (one mask per gene, as the *_constrained entries take them) a path with a disallowed label does not exist,
 * and lognorm is the restricted log Z.  attr_value and allowed may each be NULL.  The walk is parallel over contigs and labels and
 * sequential along a contig (contigs are not chunked).
 *   * The recursion runs on the lattice expanded by a run counter c = min(runs begun up to and including this gene, K).  A label
 *     outside S has the states (j, c), c = 0 .. K; a label inside S has (j, c), c = 1 .. K; states are ordered by label, then by
 *     c.  At gene 0 (j outside, 0) and (j inside, 1) start at state_0[j], the others at -infinity.  The sources of a destination
 *     at gene t: (j, c) with j outside S -- (i, c) for every label i; (j, c) with j inside S -- (i, c) for i inside S, (i, c - 1)
 *     for i outside S, and at c = K also (i, K) for i outside S (the counter saturates).  At the contig's end every state is
 *     admissible, and slot k collects the states (., k) of every label.
 *   * Max semiring: value = (delta[source] + trans[i][j]) + state_t[j] -- the operation order of gecco_crf_viterbi and
 *     gecco_crf_viterbi_min_run, so a score is the left-to-right sum of the path's terms, every addition rounded on its own.
 *     The largest of a contig's K + 1 scores has the bits of gecco_crf_viterbi_kbest's rank 0.
 *   * The tie rule is operational.  A destination scans its sources in ascending (source label, source slot) order with a strict
 *     `>` update; at the end the smaller label wins a tie within a slot.  This is a rule on expanded states and NOT "reversed
 *     path ascending" (at the tail slot two expanded states stand for one label).
 *   * Sum semiring: the same sources with a max-shifted log-sum-exp in place of the max, fp64 throughout; a destination all of
 *     whose sources are -infinity stays -infinity.
 *   * The sum launch runs only when log_mass is given; the max launch and the backtrack run only when score is given.  Asking
 *     for one changes no byte of the other.
 *   * Infeasible counts (k > ceil(T / 2) on a contig of T genes, k = 0 when S is every label, masks that forbid it): log_mass
 *     -infinity, score -infinity, label -1 at every gene of that plane; never NaN.
 *   * Outputs.  log_mass and score are double [n_contigs][K + 1], each optional; y is int8 [K + 1][n_genes] (plane k at
 *     y + k * n_genes), optional with score; lognorm [n_contigs] (optional) is the bytes gecco_crf_marginals_full (or its
 *     _valued / _constrained sibling, by the arguments given) writes for the batch.  (A 2-label model without values and masks
 *     has kernels of its own for that: asking for lognorm there costs a second pass.)  A contig without genes gets
 *     log_mass[c][0] = 0 and score[c][0] = 0, gecco_crf_viterbi's convention, -infinity at every other slot, and 0 for lognorm.
 *     contig_ptr[0] > 0 works as in the other one-shots.  The back-pointers are workspace of n_genes * L * (K + 1) bytes, one
 *     byte per (gene, label, slot): the source label and one bit "the source slot was K, not K - 1"; sizes are computed in
 *     size_t; a failed allocation is GECCO_CRF_ENOMEM.  Equal calls give equal bytes (no atomics).
 *   * Limits: 1 <= max_runs <= 32 and num_labels <= 32.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL, every message prefixed "run_counts:": max_runs
 *     outside 1 .. 32 ("run_counts: max_runs = ... is outside 1 .. 32"), a set_mask of 0 or with a bit at or above num_labels,
 *     y given without score, log_mass, score and y all NULL.  The checks of the *_valued and *_constrained entries apply to
 *     attr_value and allowed.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_run_counts(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                         const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                         const uint32_t *allowed /* NULL: no masks */, uint32_t set_mask, int32_t max_runs,
                         double *log_mass /* [n_contigs][K + 1] or NULL */, double *score /* [n_contigs][K + 1] or NULL */,
                         int8_t *y /* [K + 1][n_genes] or NULL */, double *lognorm /* [n_contigs] or NULL */);

/* ---- run posteriors (ABI 2.21.0, additive; gecco_crf_version() stays 340) --------------------------------------------------------
 * The exact distribution of where a run starts and ends, on the whole-contig lattice of gecco_crf_marginals_full and
 * gecco_crf_viterbi (not a windowed one).  Fix a gene a and a label set S; "the run through a" is the maximal stretch of genes
 * around a whose labels all lie in S.  With `allowed` (one mask per gene, as the *_constrained entries take them) the lattice is
 * the restricted one.  attr_value and allowed may each be NULL.  All outputs are natural logarithms, <= 0.0, -infinity where the
 * probability is zero, never NaN.  T is the contig's number of genes.
 *   * Anchor query q is (anchor_contig[q], anchor_item[q], anchor_mask[q]): a contig of the batch, a gene offset a from that
 *     contig's first gene, and a mask with bit y set when label y is in S.  With the call-wide reach >= 0 it gives
 *       log_anchor[q]                  = log P(y_a in S | x);
 *       log_start[q * (reach+1) + r]   = log P(the run through a starts at gene a - r | x)
 *                                      = log P(y_{a-r} .. y_a in S, and a - r = 0 or y_{a-r-1} not in S | x), -infinity for r > a;
 *       log_start_beyond[q]            = log P(y_{a-reach-1} .. y_a in S | x), the run starts before the reach; -infinity when
 *                                        a - reach - 1 < 0;
 *       log_end[q * (reach+1) + r]     = log P(the run's last gene is a + r | x), -infinity for a + r >= T;
 *       log_end_beyond[q]              = log P(y_a .. y_{a+reach+1} in S | x); -infinity when a + reach + 1 >= T.
 *     logsumexp(log_start[q][:]) (+) log_start_beyond[q] = log_anchor[q] up to rounding, and the same for the ends.  S may hold
 *     every label: every start but gene 0 and every end but gene T - 1 is then -infinity, and log_anchor is exactly 0.0.
 *   * Closed-run query q is (run_contig[q], run_begin[q], run_end[q], run_mask[q]), the end exclusive:
 *       log_run[q] = log P(y_begin .. y_{end-1} in S, begin = 0 or y_{begin-1} not in S, end = T or y_end not in S | x),
 *     the probability that a run is EXACTLY the range: one entry of the joint (start, end) distribution of the run through any
 *     gene of the range.  The joint is NOT the product of the two marginals above; sum_e P(start = s, end = e) = P(start = s).
 *   * CRFsuite has no begin or end features: at a contig's first gene the entering vector is the emission alone.
 *   * One forward-backward pass over the batch serves every query.  An anchor then costs two sequential walks of at most
 *     reach + 2 genes, a closed run one walk of its genes, each by one group of lanes (crf_runs.hip); walks are not chunked.
 *     Inside a walk the state scores are shifted by their maximum over S, so a label outside S that leads by hundreds costs its
 *     exact, finite amount, and the vector is rescaled at every gene: a start hundreds of genes away with probability 1e-250 is
 *     reported with relative accuracy.  The genes bordering the run enter through the pass's forward vector and marginals and
 *     inherit its range, as in gecco_crf_span_probabilities.  A walk that loses all mass (a gene that allows no label of S,
 *     zero transitions, an empty complement) writes -infinity for the rest.
 *   * Equal calls give equal bytes (no atomics); a query's result depends neither on the other queries nor on reach: entry r
 *     is the same bits at every reach >= r.
 *   * marg [n_genes][L] and lognorm [n_contigs], each optional, are the bytes gecco_crf_marginals_full (or its _valued /
 *     _constrained sibling, by the arguments given) writes for the batch.  (A 2-label model without values and masks has kernels
 *     of its own for those: asking for marg or lognorm there costs a second pass.)  Either list of queries may be empty; with
 *     both empty the call fills marg and lognorm.
 *   * Refused on the host before the device is looked at, GECCO_CRF_EINVAL with a message: a negative n_anchors or n_runs; reach
 *     outside 0 .. 65536; n_anchors * (reach + 1) >= 2^31; a NULL array of a non-empty list ("null buffer"); and, naming the
 *     query ("anchor q: ...", "run q: ..."): a contig index outside the batch, an item outside its contig, begin < 0, begin >=
 *     end, end beyond the contig's length, a mask of 0, a mask with a bit at or above the model's label count.  The checks of
 *     the *_valued and *_constrained entries apply to attr_value and allowed.
 *   * Refused with GECCO_CRF_EINVAL when there are queries and the largest |transition weight| among those whose exp is not 0
 *     exceeds 150 (the whole-contig pass itself takes -700 <= max <= 700): beyond it the stored forward vectors no longer hold
 *     the labels the walks read, and runs that need them came back -infinity.  Subtracting a constant from every transition
 *     weight leaves the model unchanged.
 * One device per call, one plan over the whole batch (no session, batch-driver or multi-device form). */
int gecco_crf_run_posteriors(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                             const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value /* NULL: no values */,
                             const uint32_t *allowed /* NULL: no masks */, const int32_t *anchor_contig, const int32_t *anchor_item,
                             const uint32_t *anchor_mask, int32_t n_anchors, int32_t reach, double *log_anchor /* [n_anchors] */,
                             double *log_start /* [n_anchors][reach+1] */, double *log_start_beyond /* [n_anchors] */,
                             double *log_end /* [n_anchors][reach+1] */, double *log_end_beyond /* [n_anchors] */,
                             const int32_t *run_contig, const int32_t *run_begin, const int32_t *run_end, const uint32_t *run_mask,
                             int32_t n_runs, double *log_run /* [n_runs] */, double *marg /* [n_genes][L] or NULL */,
                             double *lognorm /* [n_contigs] or NULL */);

/* ---- feature selection (ABI 2.4.0): two-sided Fisher exact test over 2x2 tables, in fp64 -------------------------
 * What GECCO's Fisher feature selection (gecco/crf/select.py) asks scipy.stats.fisher_exact(table, "two-sided") for, once
 * per domain name.  tables: n rows of {a, b, c, d} (int64, row-major, = [[a, b], [c, d]]); pvalue[n] out.  Synchronous.
 * Semantics (scipy 1.15): a zero row or column sum gives exactly 1.0; a pmf(a) within a relative 1e-14 of the pmf at the
 * mode int((a + c + 1) * (a + b + 1) / (N + 2)) gives exactly 1.0; otherwise p is the hypergeometric mass from a outward on
 * its side of the mode plus the mass of every term on the other side whose pmf is at most pmf(a) * (1 + 1e-14), clamped to
 * 1.0.  Terms that are mathematically equal to pmf(a) (every symmetric table) are included.
 * Range and accuracy: cells >= 0 and a total <= 2^31 - 1 (GECCO_CRF_EINVAL otherwise, before any device work; n = 0 is
 * valid and touches no device).  Relative error <= 1e-10 against scipy wherever scipy's p >= 1e-280; below that both are
 * < 1e-250 (p underflows to 0 where pmf(a) < e^-720 pmf(mode)); where scipy is itself off (up to ~3e-9 at N ~ 10^7) the
 * value matches the exact one to 1e-12.  A table's value depends on that table alone. */
int gecco_crf_fisher_exact(int32_t device, const int64_t *tables, int64_t n, double *pvalue);

/* ---- interval join of genes and clusters (ABI 2.6.0) ----------------------------------------------------------------
 * What GECCO's `label_genes` (gecco/cli/commands/_common.py) and `gecco train`'s `_assign_clusters` ask: which clusters of
 * its sequence does every gene overlap, bounds inclusive (cluster_start <= gene_end and gene_start <= cluster_end).
 * Genes: n_genes rows of (gene_seq, gene_start, gene_end), grouped by sequence code (0 <= code < n_seqs, non-decreasing) and
 * sorted by start inside a sequence (GECCO_CRF_EINVAL otherwise; equal starts may come in any order).  Clusters: those of
 * sequence s are cluster_start / cluster_end[cluster_ptr[s] .. cluster_ptr[s + 1]), sorted by start; a sequence may have
 * no genes or no clusters.  Coordinates are below 2^60 in magnitude.
 * Out: label_out[n_genes] = 1 where the gene overlaps any cluster, else 0; member_ptr_out[n_clusters + 1] /
 * member_gene_out = the genes of every cluster in gene order (CSR; a gene in several clusters is listed in each).  The
 * member count is written to *n_members; when it exceeds max_members, labels and member_ptr_out are still written, the
 * call returns GECCO_CRF_EINVAL, and the caller retries with a larger member_gene_out.  Deterministic; synchronous. */
int gecco_crf_cluster_overlaps(int32_t device, int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start,
                               const int64_t *gene_end, int32_t n_seqs, const int32_t *cluster_ptr,
                               const int64_t *cluster_start, const int64_t *cluster_end, uint8_t *label_out,
                               int32_t *member_ptr_out, int32_t *member_gene_out, int64_t max_members, int64_t *n_members);

/* gecco_crf_domain_composition with clusters given as member lists instead of contiguous gene ranges: cluster k is the
 * genes member_gene[member_ptr[k] .. member_ptr[k + 1]) in that order (any genes, repeats allowed), each contributing its
 * domain rows dom_ptr[g] .. dom_ptr[g + 1].  comp_out[n_clusters][n_cols]: the same sums, in the same order, as
 * gecco_crf_domain_composition gives for the concatenated rows.  Synchronous. */
int gecco_crf_domain_composition_members(int32_t device, const int32_t *member_ptr, int32_t n_clusters,
                                         const int32_t *member_gene, const int32_t *dom_ptr, int32_t n_genes,
                                         const int32_t *dom_col, const double *dom_weight, int32_t n_cols,
                                         int32_t normalize, double *comp_out);

/* ---- cluster type classifier (ABI 2.7.0): random forest fit and predict ---------------------------------------------
 * What GECCO's TypeClassifier (gecco/types/__init__.py) asks sklearn.ensemble.RandomForestClassifier for: fit with
 * criterion "gini", max_features = max_features, bootstrap, no depth limit, min_samples_split 2, min_samples_leaf 1, no
 * class weights; every tree equals sklearn 1.7's node for node and bit for bit (the 1.7.2 build's behaviour: two sorted
 * float32 neighbours are distinct values when the second is greater at all; the 1e-7 FEATURE_THRESHOLD of sklearn's
 * source acts as 0 in that build).  The caller draws the random streams as
 * sklearn does: rand_state[t] = RandomState(seed_t).randint(0, 2^31 - 1) and sample_counts[t] = bincount of
 * RandomState(seed_t).randint(0, n, n) for the per-tree seeds seed_t = RandomState(random_state).randint(2^31 - 1, n_trees).
 * X: n_samples x n_features CSC float32 (col_ptr[n_features + 1], row_idx strictly increasing within a column, finite values;
 * stored zeros count as zeros).  y[n_samples][n_outputs]: class index per output, n_classes[k] in {1, 2}.
 * Range: n_samples <= 4096, n_features <= 8192, n_outputs <= 64, n_trees <= 65535 (GECCO_CRF_EINVAL before any device
 * work otherwise).  Synchronous.  The forest lives on `device` until gecco_crf_forest_free. */
typedef struct gecco_crf_forest gecco_crf_forest;
int gecco_crf_forest_fit(int32_t device, int32_t n_samples, int32_t n_features, const int32_t *col_ptr, const int32_t *row_idx,
                         const float *values, int32_t n_outputs, const uint8_t *n_classes, const uint8_t *y, int32_t n_trees,
                         const int32_t *sample_counts, const uint32_t *rand_state, int32_t max_features,
                         gecco_crf_forest **out);
/* n_trees, n_outputs, max_n_classes (2 if any output has 2 classes, else 1); node_count / max_depth: [n_trees] (may be
 * NULL). */
int gecco_crf_forest_info(const gecco_crf_forest *f, int32_t *n_trees, int32_t *n_outputs, int32_t *max_n_classes,
                          int32_t *node_count, int32_t *max_depth);
/* Tree `tree` as sklearn's Tree arrays, node_count entries each (value: node_count x n_outputs x max_n_classes); any
 * pointer may be NULL. */
int gecco_crf_forest_export(const gecco_crf_forest *f, int32_t tree, int32_t *children_left, int32_t *children_right,
                            int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                            double *weighted_n_node_samples, double *value);
/* posit[n_rows][n_outputs] = 1 - predict_proba(x)[k][:, 0]: rows rounded to float32, leaf values normalised per tree,
 * summed in tree order in fp64 and divided by n_trees.  x: n_rows x n_features row-major fp64 (host).  n_rows = 0 is valid
 * and touches no device.  Synchronous. */
int gecco_crf_forest_predict(const gecco_crf_forest *f, int32_t n_rows, const double *x, double *posit);
void gecco_crf_forest_free(gecco_crf_forest *f);

/* ---- cluster type classifier, several forests at once (ABI 2.9.0) ----------------------------------------------------
 * n_problems (1 .. 1024) independent fits in one launch of n_problems x n_trees workgroups: the folds of a
 * cross-validation.  n_features, n_outputs, n_trees and max_features are shared; problem k brings its own n_samples[k], CSC
 * matrix (col_ptr[k], row_idx[k], values[k]), n_classes[k][n_outputs], y[k], sample_counts[k] and rand_state[k], each as
 * gecco_crf_forest_fit takes them (n_classes, hence max_n_classes, may differ between problems).  out[k] is an ordinary
 * forest handle, node for node and bit for bit what gecco_crf_forest_fit returns for problem k alone, whatever the other
 * problems are and whatever their order; gecco_crf_forest_fit is the batch of one.  Every argument is checked before any
 * device work, with gecco_crf_forest_fit's ranges per problem; the message names the problem.  On any failure every out[k]
 * is NULL and nothing stays allocated.  Memory: per problem 2 n - 1 node slots per tree of 40 + 8 n_outputs max_n_classes
 * bytes each, which stay with the handle, and 24 (n + 1) + 4 n bytes per tree of work space.  Synchronous. */
int gecco_crf_forest_fit_batch(int32_t device, int32_t n_problems, int32_t n_features, int32_t n_outputs, int32_t n_trees,
                               int32_t max_features, const int32_t *n_samples, const int32_t *const *col_ptr,
                               const int32_t *const *row_idx, const float *const *values, const uint8_t *const *n_classes,
                               const uint8_t *const *y, const int32_t *const *sample_counts,
                               const uint32_t *const *rand_state, gecco_crf_forest **out /* [n_problems] */);
/* Forest f[k] scores its own n_rows[k] rows x[k] (n_rows[k] x n_features, row-major fp64) into posit[k]
 * (n_rows[k] x n_outputs): one launch and one download for all problems (every non-empty block of rows is copied to the
 * device straight from x[k], the forests' table in one more copy), each posit[k] bit for bit what
 * gecco_crf_forest_predict gives.  n_rows[k] = 0 is valid (x[k] and posit[k] are then not read).  All forests must be on
 * one device, otherwise GECCO_CRF_EINVAL.  Synchronous. */
int gecco_crf_forest_predict_batch(const gecco_crf_forest *const *f, int32_t n_problems, const int32_t *n_rows,
                                   const double *const *x, double *const *posit);

#ifdef __cplusplus
}
#endif
#endif /* GECCO_CRF_H */
