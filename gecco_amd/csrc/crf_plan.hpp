// Batch plan: host-side layout of one batch of contigs in "slot space" + the device copies
// the kernels need.  Mirrors the bookkeeping half of gecco/crf/__init__.py:209-240
// (which contigs are scored, how they are padded, how many windows there are).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "crf_device.hpp"
#include "crf_hip_own.hpp"
#include "crf_model.hpp"

namespace gecco {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Carves one block into parts that start at multiples of 256 bytes: take() gives the offset of the next part, `off` is the
// size of the block so far.  Every pinned / device block of the plan and of the batch driver is laid out with it.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    }
};

// Per-device copies of a model's tables (owned by the Model, created on first use).
struct DeviceTables {
    int device = -1;
    DeviceBlock<double> wtab;     // [A*L]
    DeviceBlock<double2> wtab2[2];  // L == 2: [A] (other, label) for label = 0 / 1
    DeviceBlock<double> exp_trans;  // [L*L]
    DeviceBlock<double> trans;      // [L*L] raw weights (general-L Viterbi)
    double wmax_abs = 0.0, tmax_abs = 0.0;  // largest |state weight| / |transition weight| (bounds of the Viterbi exactness margin)
    double tmax = 0.0;              // largest transition weight: what exp_trans has to keep inside the range (check_exp_trans_range)
    double tmax_abs_live = 0.0;     // largest |transition weight| among those whose exp is not 0 (the range run posteriors take)
    DeviceBlock<double> rtab[2];  // L == 2: [32] mu01(label) * 2^(j/32), the exp table of the window kernel's slot constants
    // L == 2: [A + 1] (delta_a, exp(delta_a)) for label = 0 / 1, the factor table of the product-form slot constants
    // (build_slot_table); slot_dmax / slot_prod_max_cnt: its two model constants
    DeviceBlock<double2> ptab[2];
    double slot_dmax = 0.0;
    int32_t slot_prod_max_cnt = 0;
    // Host-side constants of the kernels' argument blocks that depend on the model alone (L == 2), computed ONCE here: a launch
    // used to recompute them (17 exp calls, 36 divisions, three getenv scans per pipelined decode call: ~1 us of a 5 us
    // launch-bound step, tools/host_issue_probe.py).
    struct WinConsts {
        double mu01, rho, kappa_over_mu01, inv_kappa, g00, g01, g10, g11, expc[12], ratio_zmax;
        int32_t prod_cnt;  // attributes up to which a slot's constant is the running product (slot_prod_max_cnt; 0 when mu01 itself is extreme)
    } win[2];  // by queried label
    struct SeqConsts {
        double mx, m00, m01, m10, m11, v_lo, v_hi, v_k, expc[12];
        int32_t raw_fold, v_exact;
    } seq;
    bool consts_ok = false;
};

// A pinned host block mirrored by a device block: plan tables are written on the host side and reach
// the device with ONE asynchronous copy.  Grow-only, so a plan that is rebuilt for the next chunk of a
// batch (crf_session.cpp) allocates nothing once it has seen its largest chunk.
struct Arena {
    char *h = nullptr, *d = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes, const char *what);  // the plan's device must be current
    void release();
};

// One batch's CSR arrays on the device, as every run call takes them: the row pointers and attribute ids, and for a plan laid
// out with `valued` the value of every attribute entry (parallel to attr_id) with the largest |value| among them, which scales
// the Viterbi margin's bound on a state score; for a plan laid out with `masked`, one mask of allowed labels
// per gene.  The caller keeps the arrays alive until the work is done.
struct DeviceCsr {
    const int32_t *gene_ptr = nullptr, *attr_id = nullptr;
    const double *attr_value = nullptr;
    double vmax_abs = 1.0;
    const uint32_t *allowed = nullptr;
};

struct Plan {
    DeviceScope home{DeviceScope::kLater};  // (first member: see ~Plan)
    const Model *model = nullptr;
    int device = -1;  // -1: host-only plan (layout queries work, launches return ENODEV)
    int32_t W = 0, step = 1, pad = 1;
    int32_t n_contigs = 0, n_genes = 0, n_max = 0;  // (n_max: genes of the longest contig)
    int64_t n_windows = 0;
    // slot-space layout (host)
    int32_t K = 0, S = 0, ntiles = 0, tile_out = 0, tiles_per_wg = 1;
    std::vector<int32_t> c_slot, c_gene, c_n;
    std::vector<int4> tile_desc;
    std::vector<uint64_t> start_bits;
    std::vector<int2> skipped;  // gene ranges of contigs skipped by pad == 0
    std::vector<int32_t> contig_ptr;
    std::vector<int32_t> irr_prefix;  // scratch of plan_build (kept for its capacity)
    uint32_t rescale_mask = 0;
    bool all_regular = false;   // no padded or skipped contig: every tile maps slots to genes by the identity
    bool fast_ok = false;       // the register-resident kernel takes this shape
    bool force_generic = false; // GECCO_CRF_FORCE_GENERIC=1 (tests): always use the generic kernel
    bool general = false;       // any-L kernels (crf_general.hip): L != 2, or GECCO_CRF_FORCE_GENERAL=1 (tests)
    bool gen_small = false;     // ... 3 or 4 labels: the lane-per-window kernel (gl_windowed_small) and its tile geometry
    std::string kernel_name;
    // device copies (all inside `tables`)
    Arena tables;
    int32_t *d_c_slot = nullptr, *d_c_gene = nullptr, *d_c_n = nullptr, *d_contig_ptr = nullptr;
    int4 *d_tile_desc = nullptr;
    uint64_t *d_start_bits = nullptr;
    int2 *d_skipped = nullptr;
    const DeviceTables *tables_model = nullptr;
    // whole-contig scans (rows F, V) and the segmenter: contig flags + scan block table, built on first use
    Arena seq;
    bool seq_ready = false;
    uint8_t *d_seq_flags = nullptr;
    const uint16_t *d_seq_flat_bits = nullptr;  // [ceil(n / 2048) * 256] the same bits for the flat layout (lane l owns genes 8 l ..)
    const uint16_t *d_seq_lane_bits = nullptr;  // [n_cblocks * 256] contig start / end bits of the 8 genes of every lane (short contigs)
    int32_t *d_seq_cblk = nullptr;    // short contigs: first gene of every workgroup of whole contigs (<= 2048 genes), [n_cblocks+1]
    int32_t n_cblocks = 0;
    int32_t *d_seq_cblk_rank = nullptr, *d_seq_ne_contig = nullptr;  // non-empty contigs before every workgroup; their indices
    int32_t n_empty_contigs = 0;
    bool seq_short = false;           // no contig longer than one scan block: whole contigs per workgroup, one launch per decoder
    Stream side_stream;  // (Viterbi of 17-32 labels, below; declared before the work spaces its kernels use)
    // workspaces, reserved on first use, grow-only
    DeviceBlock<char> seq_ws, gen_ws, seg_ws;
    size_t vbound_sig = 0;  // layout for which the exactness test's bound / counter / contig flags were last zeroed
    DeviceBlock<double> win_scratch;
    // chunk tables of the any-L whole-contig kernels (first gene / contig of every chunk, chunks of every contig): they
    // depend on the plan's contigs and the chunk length only, so they are built and uploaded on first use
    // Two sets: every contig (marginals, Viterbi of small models), and the contigs longer than `min_len` only (Viterbi of
    // 17-32 labels: the long tail of a batch whose other contigs take the wave-per-contig kernel).
    struct GenTab {
        DeviceBlock<char> d;
        int32_t chunk = 0, min_len = -1;  // (chunk == 0: not built)
        size_t nch = 0, off1 = 0, off2 = 0;
    } gen_tab[2];
    // Viterbi of 17-32 labels: the chunked kernels of a batch's long contigs run on a stream of the plan's own next to the
    // wave-per-contig kernel of the others (forked from and joined to the caller's stream by events)
    int32_t gen_wave_tmax = INT32_MIN, gen_wave_tmax_f = INT32_MIN;  // the splits chosen for this layout (Viterbi, marginals; INT32_MIN: not yet)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Pipelined decode (plan_run_decode_pipelined): what the last call left for the next one -- the batch's score differences
    // in buffer `parity` of the workspace (pending) and the batch's arrays, which the caller keeps alive until then.
    struct Pipe {
        bool pending = false;
        int parity = 0;
        DeviceCsr csr;
    } pipe;
    bool async_tables = false;  // the owner launches everything on ONE stream (batch driver): table uploads are not waited for
    bool tables_by_kernel = false;  // copied tables are fetched from the pinned block by a small launch on the upload stream, not by
                                    // the copy engine (batch driver: the engine is busy with the next chunk's arrays by then)
    bool tables_in_host_memory = false;  // the window kernel reads the plan tables from the pinned block itself (batch driver:
                                         // one copy and one inter-copy gap less per chunk; they are ~0.1 MB, read once)
    int64_t csr_begin = -1, csr_end = -1;  // gene_ptr[0] / gene_ptr[n_genes] when the owner knows them (batch driver's direct path), else -1
    // Reference-bits mode (crf_exact.hip): windowed marginals in CRFsuite's own operation order with a correctly rounded exp --
    // the reference's output files bit for bit, at about six times the fast kernels' time.  Set by the owner before
    // plan_build (batch driver: gecco_crf_session_set_reference_bits); GECCO_CRF_REFERENCE_BITS=1 sets it for every 2-label plan that runs windowed marginals.
    bool reference_bits = false;
    bool windowed_use = true;  // the owner runs windowed marginals on this layout (batch driver: false for Viterbi-only and
                               // whole-contig-marginal requests): the environment switch applies to such layouts only
    bool reference_now = false;  // (this layout runs in reference-bits mode: reference_bits, or the environment)
    // Real-valued attributes (the *_valued one-shots).  `valued` is set by the owner before plan_build: the layout
    // takes the any-L kernels at every label count, 2 included, and reference-bits mode does not apply.  The values themselves
    // belong to a batch, not to the layout: they come with every run call (DeviceCsr), which is refused when it brings values
    // to a layout without `valued`, or none to one with it.
    bool valued = false;
    // Allowed-label sets (the *_constrained one-shots).  `masked` is set by the owner before plan_build, and works
    // as `valued` does: the any-L kernels at every label count, no reference-bits mode, and the masks come with every run call
    // (DeviceCsr::allowed), which is refused when it brings masks to a layout without `masked`, or none to one with it.
    bool masked = false;
    // Lattice queries (plan_run_span_probabilities, plan_run_span_conditionals, plan_run_sample_paths, plan_run_viterbi_kbest, plan_run_edge_posteriors,
    // plan_run_viterbi_min_run, plan_run_run_posteriors, plan_run_marginals_min_run, plan_run_run_counts, plan_run_max_marginals).  `lattice` is
    // set by the owner before plan_build: the layout takes the any-L kernels at every label count, as `valued` and `masked` do --
    // the queries' kernels read the forward vectors and raw state scores of their workspace, which a 2-label plan does not have
    // otherwise.  Nothing else changes: reference-bits mode is decided as ever.
    bool lattice = false;
    bool seq_in_host_memory = false;     // small batches (batch driver's direct path): the whole-contig tables AND the contig flags
                                         // stay in the pinned block, flags built by the host -- no copy, no launch in front of the decoder
    // every label's windowed marginals (crf_general_windowed.hip): the tile table of the lane-per-window tier when the plan's own
    // table has another geometry (2-label plans), built on first use
    DeviceBlock<int4> all_tiles;
    int32_t all_ntiles = -1;  // (-1: not built for this layout)
    std::mutex ws_mutex;  // guards the lazy workspace / table creation: launches of one plan may come from several threads
    ~Plan();
};

// `upload_stream` / `sync`: the device copy of the tables is ONE asynchronous copy on that stream; with
// sync it is waited for before returning (the caller may then launch on any stream).  `p` may be a plan
// that has been built before: its allocations are reused.
int plan_build(const Model &m, int device, const int32_t *contig_ptr, int32_t n_contigs, int32_t W, int32_t step,
               int32_t pad, Plan &p, hipStream_t upload_stream = nullptr, bool sync = true);
// contig flags / scan block table on the device (what rows F, V and R need), uploaded on `stream`
int plan_ensure_seq(Plan &p, hipStream_t stream, bool sync = true);
// row R chained behind the marginals on the same stream: d_p and d_annotated are device arrays over the
// plan's genes; rows go to d_seg (device-accessible memory), their number to d_total
int plan_run_segment(Plan &p, const double *d_p, const uint8_t *d_annotated, const SegParams &params, int32_t *d_seg,
                     int32_t max_seg, int32_t *d_seg_off, int32_t *d_total, hipStream_t stream, double *d_gather = nullptr,
                     int32_t gather_cap = 0);
int plan_run_windowed(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                      hipStream_t stream);
// every label's windowed marginal in one pass: d_p_all [n_genes][L]; d_p_any [n_genes] = the windowed probability of any label
// but `background`, or null with background == -1 (crf_general_windowed.hip)
int plan_run_windowed_all(Plan &p, const DeviceCsr &csr, int32_t background, double *d_p_all,
                          double *d_p_any, hipStream_t stream);
const char *plan_all_kernel_name(const Plan &p);
// windowed marginals + whole-contig Viterbi of the same batch in one pass over the CSR
// Decode pipelined over batches: enqueue the windowed marginals of `cur`'s batch (cur may be null: flush) and the Viterbi
// labels of the batch the previous call scored on `prev` (null on the first call; may be the same plan) -- in ONE launch
// when both sides qualify (2-label model, W = 20, short contigs: crf_decode_pipelined), in separate launches otherwise.
int plan_run_decode_pipelined(Plan *cur, const DeviceCsr &csr, int32_t label, double *d_p_out,
                              Plan *prev, int8_t *d_prev_y, hipStream_t stream);
int plan_run_decode(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                    int8_t *d_y, double *d_score, hipStream_t stream);
int plan_run_marginals_full(Plan &p, const DeviceCsr &csr, double *d_marg,
                            double *d_lognorm, hipStream_t stream);
int plan_run_viterbi(Plan &p, const DeviceCsr &csr, int8_t *d_y, double *d_score,
                     hipStream_t stream);
// Region posteriors of a plan laid out with `lattice`: the whole-contig marginals of the batch (d_marg [n_genes][L], which the span
// kernel reads back, and d_lognorm [n_contigs] or null, both as plan_run_marginals_full writes them), then d_logp[q] = log P(every
// gene of span q carries a label of its set | x) for the n_spans checked queries of d_spans (crf_spans.hip), all on `stream`
int plan_run_span_probabilities(Plan &p, const DeviceCsr &csr, const SpanQuery *d_spans, int32_t n_spans, double *d_logp,
                                double *d_marg, double *d_lognorm, hipStream_t stream);
// Marginals given a region and knock-out attributions of a plan laid out with `lattice`: the whole-contig marginals of the batch
// and the region posteriors d_logp [n_spans], both exactly as plan_run_span_probabilities runs them, then what `q` asks for (device
// pointers; crf_device.hpp: its logp and attr_value are set here) for its checked queries (crf_conditionals.hip), all on `stream`
int plan_run_span_conditionals(Plan &p, const DeviceCsr &csr, const ConditionalArgs &q, double *d_logp, double *d_marg,
                               double *d_lognorm, hipStream_t stream);
// Run posteriors of a plan laid out with `lattice`: the whole-contig marginals of the batch (d_marg [n_genes][L], which the walks
// read back, and d_lognorm [n_contigs] or null, both as plan_run_marginals_full writes them), then what `q` asks for (device
// pointers; crf_device.hpp) for its checked anchors and closed runs (crf_runs.hip), all on `stream`
int plan_run_run_posteriors(Plan &p, const DeviceCsr &csr, const RunPosteriorArgs &q, double *d_marg, double *d_lognorm,
                            hipStream_t stream);
// Label paths drawn from p(y | x), a plan laid out with `lattice`: the whole-contig marginals of the batch exactly as
// plan_run_marginals_full runs them (d_marg [n_genes][L], d_lognorm [n_contigs] or null), then d_y[g * n_samples + s] = the label
// of gene g in sample s (crf_sample.hip: Philox counters (gene offset, sample, contig, 0) under `seed`), then, for the n_runs
// checked queries of d_queries, d_runs [n_runs][n_samples][2]: the run of labels of the query's set around its anchor in every
// sample.  All on `stream`.
int plan_run_sample_paths(Plan &p, const DeviceCsr &csr, int32_t n_samples, uint64_t seed, const RunQuery *d_queries, int32_t n_runs,
                          int8_t *d_y, int32_t *d_runs, double *d_marg, double *d_lognorm, hipStream_t stream);
// The K best label paths of every contig, a plan laid out with `lattice`: the whole-contig marginals of the batch exactly as
// plan_run_marginals_full runs them (d_marg [n_genes][L], d_lognorm [n_contigs] or null; gl_state also keeps the raw state scores),
// then the list recursion and its backtrack (crf_kbest.hip): d_y [n_genes][k], d_score [n_contigs][k], d_n_paths [n_contigs].
// d_back (kbest_back_bytes) and d_fin (kbest_fin_bytes) are the kernel's workspace.  A contig is one sequential walk: not
// chunked, like the spans' and the samples'.  All on `stream`.
int plan_run_viterbi_kbest(Plan &p, const DeviceCsr &csr, int32_t k, uint16_t *d_back, uint16_t *d_fin, int8_t *d_y, double *d_score,
                           int32_t *d_n_paths, double *d_marg, double *d_lognorm, hipStream_t stream);
// Decoding under a minimum run length, a plan laid out with `lattice`: the whole-contig marginals of the batch exactly as
// plan_run_marginals_full runs them (d_marg [n_genes][L], d_lognorm [n_contigs] or null; gl_state also keeps the raw state scores),
// then the run-counter recursion and its backtrack (crf_minrun.hip): d_y [n_genes], d_score [n_contigs], and d_lognorm_min_run
// [n_contigs] or null (not asked for: the sum-semiring launch does not run).  d_back (minrun_back_bytes) is the kernel's
// workspace.  A contig is one sequential walk: not chunked.  All on `stream`.
int plan_run_viterbi_min_run(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t min_run, uint8_t *d_back, int8_t *d_y,
                             double *d_score, double *d_lognorm_min_run, double *d_marg, double *d_lognorm, hipStream_t stream);
// Marginals under a minimum run length, a plan laid out with `lattice`: the whole-contig marginals of the batch as above (d_marg,
// d_lognorm), then the sum-semiring forward walk of the run-counter lattice with its values kept in d_fwd (minrun_forward_bytes)
// and the backward walk (crf_minrun.hip): d_lognorm_min_run [n_contigs], d_marg_min_run [n_genes][L] or null,
// d_inside [n_genes] or null, at least one of the two.  Not chunked.  All on `stream`.
int plan_run_marginals_min_run(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t min_run, double *d_fwd, double *d_marg_min_run,
                               double *d_inside, double *d_lognorm_min_run, double *d_marg, double *d_lognorm, hipStream_t stream);
// Decoding under run-length potentials, a plan laid out with `lattice`: the whole-contig marginals of the batch as above (d_marg,
// d_lognorm), then the run-counter recursion with the length scores `sc` and its backtrack (crf_runlength.hip):
// d_y [n_genes], d_score [n_contigs], and d_lognorm_run_length [n_contigs] or null (the sum-semiring launch does not run).  d_back
// (runlen_back_bytes) is the kernel's workspace.  Not chunked.  All on `stream`.
int plan_run_viterbi_run_length(Plan &p, const DeviceCsr &csr, uint32_t set_mask, const RunLengthScores &sc, uint8_t *d_back, int8_t *d_y,
                                double *d_score, double *d_lognorm_run_length, double *d_marg, double *d_lognorm, hipStream_t stream);
// Marginals and expected run-length counts under run-length potentials, a plan laid out with `lattice`: the whole-contig marginals as
// above, then the sum-semiring forward walk with its values kept in d_fwd (runlen_forward_bytes) and the backward walk
// (crf_runlength.hip): d_lognorm_run_length [n_contigs], d_marg_run_length [n_genes][L] or null, d_inside [n_genes] or null,
// d_counts [n_contigs][M + 1] or null, at least one of the three.  Not chunked.  All on `stream`.
int plan_run_marginals_run_length(Plan &p, const DeviceCsr &csr, uint32_t set_mask, const RunLengthScores &sc, double *d_fwd,
                                  double *d_marg_run_length, double *d_inside, double *d_counts, double *d_lognorm_run_length,
                                  double *d_marg, double *d_lognorm, hipStream_t stream);
// Run counts, a plan laid out with `lattice`: the whole-contig marginals of the batch as above (d_marg, d_lognorm), then the
// recursion on the lattice expanded by a saturating run counter (crf_counts.hip): d_log_mass [n_contigs][K + 1] or
// null (the sum-semiring launch does not run); d_score [n_contigs][K + 1] or null (the max-semiring launch and the backtrack do
// not run) with d_y [K + 1][n_genes] and the workspace d_back (counts_back_bytes); at least one of the two.  Not chunked.  All
// on `stream`.
int plan_run_run_counts(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t max_runs, uint8_t *d_back, double *d_log_mass,
                        double *d_score, int8_t *d_y, double *d_marg, double *d_lognorm, hipStream_t stream);
// Edge posteriors of a plan laid out with `lattice`: the whole-contig marginals of the batch exactly as plan_run_marginals_full
// runs them (d_marg [n_genes][L], d_lognorm [n_contigs] or null), then the edge marginals and their sums that `q` asks for
// (crf_edges.hip; crf_device.hpp: EdgeQuery -- device pointers throughout, the run table that of this layout's contigs), all on
// `stream`.  An edge is independent of every other: the query is parallel over genes, a contig of any length included.
int plan_run_edge_posteriors(Plan &p, const DeviceCsr &csr, const EdgeQuery &q, double *d_marg, double *d_lognorm, hipStream_t stream);
// Max-marginals, a plan laid out with `lattice`: gl_state with the raw state scores kept, then the max-plus forward and backward
// walks, the epilogue over the genes and the span walks that `q` asks for (crf_maxmarg.hip; crf_device.hpp: MaxMargArgs -- device
// pointers throughout, its workspace of maxmarg_workspace_bytes included).  The max walks read the state scores alone: the
// whole-contig marginals of the batch run (exactly as plan_run_marginals_full runs them, into d_marg [n_genes][L] and d_lognorm
// [n_contigs]) only when d_lognorm is given, and a call without it takes models whose transitions lie outside the sum-product
// kernels' range.  Not chunked.  All on `stream`.
int plan_run_max_marginals(Plan &p, const DeviceCsr &csr, const MaxMargArgs &q, double *d_marg, double *d_lognorm, hipStream_t stream);
// Circular contigs, a plan laid out with `lattice`: gl_state with the raw state scores kept, then the walks of the lattice expanded
// by the start label that `q` asks for (crf_ring.hip; crf_device.hpp: RingArgs -- device pointers throughout, its workspaces
// included).  Every contig of the plan is a ring.  The walks run in log space on the state scores alone: no
// exp(trans) is read, the whole-contig marginals of the chain do not run, and no transition range applies.  Not chunked.  All on
// `stream`.
int plan_run_ring(Plan &p, const DeviceCsr &csr, const RingArgs &q, hipStream_t stream);
// counters of the 2-label Viterbi decoder (crf_device.hpp: SeqArgs::vd_stats); waits for the device
int plan_viterbi_stats(Plan &p, int64_t out[4], bool reset);
int get_device_tables(const Model &m, int device, const DeviceTables **out);

}  // namespace gecco
