// Training objective and gradient of the 2-label linear-chain CRF (gecco_crf_trainer_*; DESIGN.md "Training").
//
// What it computes is [EXT] CRFsuite crf1d_encode's objective over the training instances GECCO's `fit` builds
// (every sliding window of every sequence, gecco/crf/__init__.py:364-367):
//     f(w) = sum over windows of (log Z(window) - score(gold labels of the window))
//     g(w) = expected feature counts - empirical feature counts
// for the features the host generated (state features (attribute, label), transition features (label, label)).
// The regularisation terms are the host optimiser's business.
//
// The training set is uploaded once.  One evaluation is six launches on the trainer's stream:
//   1. item scores     one thread per item: s[i][y] = sum of the state weights of its attributes (CSR order)
//   2. windows         one thread per window: scaled fp64 forward-backward; alpha and the normalisers live in LDS;
//                      writes the window's node marginals [W][2] and one row (log Z - gold score, four pairwise sums).
//                      Transitions travel max-shifted (exp(t - t_max)).  The scaled form is used while its intermediates
//                      stay normal fp64 numbers; a window where they do not is redone in log space by the same thread,
//                      so the results are right for any finite weights (train_windows has the exact conditions)
//   3. item marginals  one thread per item: the node marginals of the windows covering it, in window order
//   4. attr counts     one workgroup per attribute: the item marginals over the attribute -> items transpose
//   5/6. row sums      fixed-geometry two-stage tree over the window rows
// No float atomics anywhere: every sum has one fixed order, so two evaluations give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cfloat>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_model.hpp"
#include "crf_plan.hpp"
#include "crf_train.hpp"

namespace gecco {

namespace {

constexpr int kTrainWinThreads = 64;     // windows per workgroup of the forward-backward kernel (one wave)
constexpr int kTrainThreads = 256;       // threads per workgroup of the other kernels
constexpr int kTrainRowCols = 5;         // log Z - gold, xi00, xi01, xi10, xi11
constexpr int kTrainReduceBlocks = 256;  // first stage of the row sums: a fixed number of slabs, independent of the device
constexpr int kTrainMaxW = 32;           // = kWinMaxW of the inference kernels

struct TransArgs {
    double t00, t01, t10, t11;  // transition weights
    double e00, e01, e10, e11;  // exp(t - tmax)
    double tmax;                // the largest of the four weights
    int log_space;              // 1 when an exp(t - tmax) is not a normal number: every window goes to log space
};

// Where one problem of the batch lives in the concatenated device arrays (uploaded once).  Every array of a problem is
// exactly what a lone trainer of it would hold: indices inside it (item_ptr, win_start, iw_first, attr_ptr, attr_items)
// are local to the problem.
struct ProbDev {
    int64_t item0;  // items: score, label, iw_first/cnt/off, item_marg
    int64_t iptr0;  // item_ptr (n_items + 1 entries)
    int64_t nnz0;   // attr_id, attr_items
    int64_t win0;   // windows: win_start, rows; node marginals from win0 * W
    int64_t aptr0;  // attr_ptr (A + 1 entries)
    int64_t ws0;    // state weights in the upload ([A][2] doubles)
    int64_t out0;   // outputs in the download: 5 row sums, then the expected state counts [A][2]
    int64_t n_win;
    int32_t n_items, A;
};

// One problem of one evaluation (uploaded with the weights): its transitions and the first block it owns in the
// item grid (kernels 1, 3), the window grid (2) and the attribute grid (4).  Kernels 5 and 6 give every slot 256 and 1
// blocks.  Only active problems with windows get a slot, so every slot owns at least one block of every grid.
struct Slot {
    TransArgs T;
    int32_t prob;
    int32_t blk[3];
};
enum { kGridItems = 0, kGridWindows = 1, kGridAttrs = 2 };

// The slot that owns this block of grid G: the last slot whose first block is at or before it (slots ascend).
template <int G>
__device__ __forceinline__ int slot_of(const Slot *__restrict__ slots, int n_slots) {
    const int32_t b = static_cast<int32_t>(blockIdx.x);
    int lo = 0, hi = n_slots - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (slots[mid].blk[G] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kTrainThreads) train_item_scores(const Slot *__restrict__ slots, int n_slots,
                                                                   const ProbDev *__restrict__ probs,
                                                                   const int32_t *__restrict__ item_ptr_all,
                                                                   const int32_t *__restrict__ attr_id_all,
                                                                   const double *__restrict__ wstate_all,
                                                                   double2 *__restrict__ score_all) {
    const Slot &sl = slots[slot_of<kGridItems>(slots, n_slots)];
    const ProbDev &P = probs[sl.prob];
    const int32_t i = (static_cast<int32_t>(blockIdx.x) - sl.blk[kGridItems]) * blockDim.x + threadIdx.x;
    if (i >= P.n_items) return;
    const int32_t *__restrict__ item_ptr = item_ptr_all + P.iptr0;
    const int32_t *__restrict__ attr_id = attr_id_all + P.nnz0;
    const double *__restrict__ wstate = wstate_all + P.ws0;
    double s0 = 0.0, s1 = 0.0;
    for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
        const int32_t a = attr_id[k];
        s0 += wstate[2 * a];
        s1 += wstate[2 * a + 1];
    }
    score_all[P.item0 + i] = make_double2(s0, s1);
}

// Natural log of exp(a) + exp(b), fp64, for the log-space recomputation of a flagged window.
__device__ __forceinline__ double lse2(double a, double b) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    return hi + log1p(exp(lo - hi));
}

// The window at i0 once more in log space (fp64 log-sum-exp), for a window the scaled pass flagged: same outputs as
// that pass (node marginals, log Z, the four pairwise sums), correct for any finite scores and transition weights.
// log alpha lives in the LDS slots of alpha; log beta is carried backward in registers.
__device__ __forceinline__ void train_window_logspace(const double2 *__restrict__ score, int64_t i0, int32_t W,
                                                   const TransArgs &T, double2 *__restrict__ la_lds, int lane,
                                                   double2 *__restrict__ mw, double *__restrict__ logz_out,
                                                   double *__restrict__ x_out) {
    double2 s = score[i0];
    double l0 = s.x, l1 = s.y;
    la_lds[lane] = make_double2(l0, l1);
    for (int t = 1; t < W; ++t) {
        s = score[i0 + t];
        const double n0 = lse2(l0 + T.t00, l1 + T.t10) + s.x;
        const double n1 = lse2(l0 + T.t01, l1 + T.t11) + s.y;
        l0 = n0;
        l1 = n1;
        la_lds[t * kTrainWinThreads + lane] = make_double2(l0, l1);
    }
    const double logz = lse2(l0, l1);
    mw[W - 1] = make_double2(exp(l0 - logz), exp(l1 - logz));
    double b0 = 0.0, b1 = 0.0;  // log beta
    double x00 = 0.0, x01 = 0.0, x10 = 0.0, x11 = 0.0;
    for (int t = W - 1; t >= 1; --t) {
        s = score[i0 + t];
        const double q0 = s.x + b0, q1 = s.y + b1;  // log of exp(s_t) beta_t
        const double2 ap = la_lds[(t - 1) * kTrainWinThreads + lane];
        x00 += exp(ap.x + T.t00 + q0 - logz);
        x01 += exp(ap.x + T.t01 + q1 - logz);
        x10 += exp(ap.y + T.t10 + q0 - logz);
        x11 += exp(ap.y + T.t11 + q1 - logz);
        b0 = lse2(T.t00 + q0, T.t01 + q1);
        b1 = lse2(T.t10 + q0, T.t11 + q1);
        mw[t - 1] = make_double2(exp(ap.x + b0 - logz), exp(ap.y + b1 - logz));
    }
    *logz_out = logz;
    x_out[0] = x00;
    x_out[1] = x01;
    x_out[2] = x10;
    x_out[3] = x11;
}


// One window per thread.  Forward: alpha_t = normalised (alpha_{t-1} E) * exp(s_t - m_t), c_t its normaliser,
// E = exp(t - t_max), log Z = sum (log c_t + m_t) + (W - 1) t_max.  Backward with the same normalisers: beta_{W-1} = 1,
// beta_{t-1}[i] = sum_j E[i][j] exp(s_t[j] - m_t) beta_t[j] / c_t; marginal_t = alpha_t * beta_t;
// pairwise (t-1, t) = alpha_{t-1}[i] E[i][j] exp(s_t[j] - m_t) beta_t[j] / c_t.
// The scaled form is exact up to rounding while every exp(s - m), alpha (before and after normalising), u and beta stays
// a normal fp64 number.  With E <= 1, exp(s - m) <= 1 and alpha_{t-1} summing to 1, n_j = (alpha E)_j exp(s_j - m) <= 1
// and c <= 2, so one test per step covers the forward pass: min(n0, n1) >= 2 DBL_MIN implies exp(s - m), n and alpha
// all normal.  It also bounds the backward pass from above: marginal <= 1 gives beta_j <= c / n_j and
// u_j <= 1 / (alpha E)_j <= 1 / (2 DBL_MIN), so only underflow of u and beta is tested there.  A window that fails
// (a state-score gap of some 708 nats or more, a label whose alpha underflows), or every window when a shifted
// transition E is not normal (T.log_space), is recomputed in log space by the same thread (train_window_logspace);
// nothing changes for the other windows.
// (waves_per_eu(6): keeps the VGPR count, and so the occupancy, of the kernel without the log-space branch.)
// The transitions (and the log-space flag) are the problem's own, read from its slot.
__global__ void __launch_bounds__(kTrainWinThreads) __attribute__((amdgpu_waves_per_eu(6)))
train_windows(const Slot *__restrict__ slots, int n_slots, const ProbDev *__restrict__ probs,
              const double2 *__restrict__ score_all, const int32_t *__restrict__ label_all,
              const int32_t *__restrict__ win_start_all, int32_t W, double2 *__restrict__ marg_all,
              double *__restrict__ rows_all) {
    extern __shared__ double lds[];
    double2 *alpha = reinterpret_cast<double2 *>(lds);                 // [W][kTrainWinThreads]
    double *cnorm = lds + 2 * static_cast<size_t>(W) * kTrainWinThreads;  // [W][kTrainWinThreads]
    const Slot &sl = slots[slot_of<kGridWindows>(slots, n_slots)];
    const ProbDev &P = probs[sl.prob];
    const int lane = threadIdx.x;
    const int64_t w = static_cast<int64_t>(static_cast<int32_t>(blockIdx.x) - sl.blk[kGridWindows]) * kTrainWinThreads + lane;
    if (w >= P.n_win) return;
    const TransArgs T = sl.T;
    const double2 *__restrict__ score = score_all + P.item0;
    const int32_t *__restrict__ label = label_all + P.item0;
    const int32_t *__restrict__ win_start = win_start_all + P.win0;
    double2 *__restrict__ marg = marg_all + P.win0 * W;
    double *__restrict__ rows = rows_all + P.win0 * kTrainRowCols;
    const int64_t i0 = win_start[w];

    double2 s = score[i0];
    double m = fmax(s.x, s.y);
    double e0 = exp(s.x - m), e1 = exp(s.y - m);
    double c = e0 + e1;
    double a0 = e0 / c, a1 = e1 / c;
    double logz = m + log(c);
    constexpr double kMinN = 2 * DBL_MIN;
    bool ok = !T.log_space & (fmin(e0, e1) >= kMinN);  // (c = e0 + e1 >= 1 here)
    int y = label[i0];
    double gold = y ? s.y : s.x;
    alpha[lane] = make_double2(a0, a1);
    cnorm[lane] = c;
    for (int t = 1; t < W; ++t) {
        s = score[i0 + t];
        m = fmax(s.x, s.y);
        e0 = exp(s.x - m);
        e1 = exp(s.y - m);
        const double n0 = (a0 * T.e00 + a1 * T.e10) * e0;
        const double n1 = (a0 * T.e01 + a1 * T.e11) * e1;
        c = n0 + n1;
        a0 = n0 / c;
        a1 = n1 / c;
        logz += m + log(c) + T.tmax;
        ok &= fmin(n0, n1) >= kMinN;
        const int yn = label[i0 + t];
        gold += (yn ? s.y : s.x) + (y ? (yn ? T.t11 : T.t10) : (yn ? T.t01 : T.t00));
        y = yn;
        alpha[t * kTrainWinThreads + lane] = make_double2(a0, a1);
        cnorm[t * kTrainWinThreads + lane] = c;
    }
    double2 *mw = marg + w * W;
    double *r = rows + w * kTrainRowCols;
    if (ok) {
        mw[W - 1] = make_double2(a0, a1);
        double b0 = 1.0, b1 = 1.0;
        double x00 = 0.0, x01 = 0.0, x10 = 0.0, x11 = 0.0;
        for (int t = W - 1; t >= 1; --t) {
            s = score[i0 + t];
            m = fmax(s.x, s.y);
            const double ct = cnorm[t * kTrainWinThreads + lane];
            const double u0 = exp(s.x - m) * b0 / ct, u1 = exp(s.y - m) * b1 / ct;
            const double2 ap = alpha[(t - 1) * kTrainWinThreads + lane];
            x00 += ap.x * T.e00 * u0;
            x01 += ap.x * T.e01 * u1;
            x10 += ap.y * T.e10 * u0;
            x11 += ap.y * T.e11 * u1;
            b0 = T.e00 * u0 + T.e01 * u1;
            b1 = T.e10 * u0 + T.e11 * u1;
            ok &= fmin(fmin(u0, u1), fmin(b0, b1)) >= DBL_MIN;
            mw[t - 1] = make_double2(ap.x * b0, ap.y * b1);
        }
        r[1] = x00;
        r[2] = x01;
        r[3] = x10;
        r[4] = x11;
    }
    if (!ok) {
        // (overwrites whatever the scaled pass stored for this window: marginals, log Z, pairwise sums)
        train_window_logspace(score, i0, W, T, alpha, lane, mw, &logz, r + 1);
    }
    r[0] = logz - gold;
}

// Item i is covered by the windows first .. first + cnt - 1, at position off, off - step, ... in them.
__global__ void __launch_bounds__(kTrainThreads) train_item_marginals(const Slot *__restrict__ slots, int n_slots,
                                                                      const ProbDev *__restrict__ probs,
                                                                      const double2 *__restrict__ marg_all,
                                                                      const int32_t *__restrict__ iw_first_all,
                                                                      const int32_t *__restrict__ iw_cnt_all,
                                                                      const int32_t *__restrict__ iw_off_all, int32_t W,
                                                                      int32_t step, double2 *__restrict__ item_marg_all) {
    const Slot &sl = slots[slot_of<kGridItems>(slots, n_slots)];
    const ProbDev &P = probs[sl.prob];
    const int32_t i = (static_cast<int32_t>(blockIdx.x) - sl.blk[kGridItems]) * blockDim.x + threadIdx.x;
    if (i >= P.n_items) return;
    const double2 *__restrict__ marg = marg_all + P.win0 * W;
    const int64_t first = iw_first_all[P.item0 + i];
    const int32_t cnt = iw_cnt_all[P.item0 + i];
    int32_t off = iw_off_all[P.item0 + i];
    double p0 = 0.0, p1 = 0.0;
    for (int32_t k = 0; k < cnt; ++k, off -= step) {
        const double2 v = marg[(first + k) * W + off];
        p0 += v.x;
        p1 += v.y;
    }
    item_marg_all[P.item0 + i] = make_double2(p0, p1);
}

template <int NT>
__device__ __forceinline__ double2 block_sum2(double2 v, double2 *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h) {
            sh[threadIdx.x].x += sh[threadIdx.x + h].x;
            sh[threadIdx.x].y += sh[threadIdx.x + h].y;
        }
        __syncthreads();
    }
    return sh[0];
}

// Expected state counts: one workgroup per attribute, thread j sums the items j, j + NT, ... of its list, then a tree.
__global__ void __launch_bounds__(kTrainThreads) train_attr_counts(const Slot *__restrict__ slots, int n_slots,
                                                                   const ProbDev *__restrict__ probs,
                                                                   const int32_t *__restrict__ attr_ptr_all,
                                                                   const int32_t *__restrict__ attr_items_all,
                                                                   const double2 *__restrict__ item_marg_all,
                                                                   double *__restrict__ out_all) {
    __shared__ double2 sh[kTrainThreads];
    const Slot &sl = slots[slot_of<kGridAttrs>(slots, n_slots)];
    const ProbDev &P = probs[sl.prob];
    const int32_t a = static_cast<int32_t>(blockIdx.x) - sl.blk[kGridAttrs];
    if (a >= P.A) return;
    const int32_t *__restrict__ attr_ptr = attr_ptr_all + P.aptr0;
    const int32_t *__restrict__ attr_items = attr_items_all + P.nnz0;
    const double2 *__restrict__ item_marg = item_marg_all + P.item0;
    double2 acc = make_double2(0.0, 0.0);
    for (int32_t k = attr_ptr[a] + threadIdx.x; k < attr_ptr[a + 1]; k += kTrainThreads) {
        const double2 v = item_marg[attr_items[k]];
        acc.x += v.x;
        acc.y += v.y;
    }
    const double2 tot = block_sum2<kTrainThreads>(acc, sh);
    if (threadIdx.x == 0) {
        double *expected = out_all + P.out0 + kTrainRowCols;
        expected[2 * a] = tot.x;
        expected[2 * a + 1] = tot.y;
    }
}

// Row sums, stage 1: slot s owns the blocks [s * kTrainReduceBlocks, (s + 1) * kTrainReduceBlocks); its slab b = rows
// [b * chunk, (b + 1) * chunk) of its problem, chunk = ceil(n_win / kTrainReduceBlocks).
__global__ void __launch_bounds__(kTrainThreads) train_reduce_rows(const Slot *__restrict__ slots,
                                                                   const ProbDev *__restrict__ probs,
                                                                   const double *__restrict__ rows_all,
                                                                   double *__restrict__ partial_all) {
    __shared__ double sh[kTrainRowCols][kTrainThreads];
    const int s = blockIdx.x / kTrainReduceBlocks, b = blockIdx.x % kTrainReduceBlocks;
    const ProbDev &P = probs[slots[s].prob];
    const double *__restrict__ rows = rows_all + P.win0 * kTrainRowCols;
    const int64_t n = P.n_win;
    const int64_t chunk = (n + kTrainReduceBlocks - 1) / kTrainReduceBlocks;
    const int64_t lo = b * chunk, hi = std::min(n, lo + chunk);
    double acc[kTrainRowCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = lo + threadIdx.x; r < hi; r += kTrainThreads)
        for (int k = 0; k < kTrainRowCols; ++k) acc[k] += rows[r * kTrainRowCols + k];
    for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int h = kTrainThreads / 2; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h)
            for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < kTrainRowCols) partial_all[blockIdx.x * kTrainRowCols + threadIdx.x] = sh[threadIdx.x][0];
}

// Stage 2: one workgroup per slot, thread j holds slab j, then a tree.
__global__ void __launch_bounds__(kTrainReduceBlocks) train_reduce_final(const Slot *__restrict__ slots,
                                                                         const ProbDev *__restrict__ probs,
                                                                         const double *__restrict__ partial_all,
                                                                         double *__restrict__ out_all) {
    __shared__ double sh[kTrainRowCols][kTrainReduceBlocks];
    const double *__restrict__ partial = partial_all + static_cast<size_t>(blockIdx.x) * kTrainReduceBlocks * kTrainRowCols;
    for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] = partial[threadIdx.x * kTrainRowCols + k];
    __syncthreads();
    for (int h = kTrainReduceBlocks / 2; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h)
            for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < kTrainRowCols) out_all[probs[slots[blockIdx.x].prob].out0 + threadIdx.x] = sh[threadIdx.x][0];
}

template <class T>
int dev_upload(T **d, const std::vector<T> &h, const char *what) {
    int rc = check_hip(hipMalloc(reinterpret_cast<void **>(d), std::max<size_t>(h.size(), 1) * sizeof(T)), what);
    if (rc) return rc;
    if (h.empty()) return GECCO_CRF_OK;
    return check_hip(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice), what);
}

template <class T>
int dev_alloc(T **d, size_t n, const char *what) {
    return check_hip(hipMalloc(reinterpret_cast<void **>(d), std::max<size_t>(n, 1) * sizeof(T)), what);
}

int fail(const std::string &msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

// One problem's training set as a lone trainer builds it: the host arrays it uploads and what eval needs afterwards.
struct HostProblem {
    int32_t A = 0, n_items = 0, K = 0;
    int64_t n_win = 0;
    std::vector<int32_t> state_fid, trans_fid;  // [A*2], [4]: feature id of every dense slot, or -1
    std::vector<double> empirical;              // [K] observed feature counts over all windows
    std::vector<int32_t> item_ptr, attr_id, label, win_start, iw_first, iw_cnt, iw_off, attr_ptr, attr_items;
};

// Checks one problem (the lone trainer's checks and messages) and builds its windows, coverage, empirical counts and
// attribute -> items transpose.
int build_problem(const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                  const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                  const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, HostProblem *hp) {
    if (!seq_ptr || n_seqs < 0 || !state_fid || !trans_fid) return fail("trainer: null argument");
    if (num_labels != 2) {
        set_error("trainer: only 2-label models can be trained (GECCO's protein and domain modes are binary)");
        return GECCO_CRF_EUNSUPPORTED;
    }
    if (window < 1 || window > kTrainMaxW) {
        set_error("trainer: window of " + std::to_string(window) + " items; windows of 1 to 32 items are supported");
        return GECCO_CRF_EUNSUPPORTED;
    }
    if (step < 1 || step > window) return fail("Window step must be strictly positive and under `window_size`");
    if (num_attrs < 1 || num_features < 0) return fail("trainer: bad attribute or feature count");
    if (seq_ptr[0] != 0) return fail("trainer: seq_ptr[0] must be 0");
    for (int32_t s = 0; s < n_seqs; ++s) {
        if (seq_ptr[s + 1] - seq_ptr[s] < window)
            return fail("trainer: sequence " + std::to_string(s) + " has fewer items than the window");
    }
    const int32_t n_items = seq_ptr[n_seqs];
    if (n_items > 0 && (!item_ptr || !labels)) return fail("trainer: null argument");
    if (n_items > 0 && item_ptr[0] != 0) return fail("trainer: item_ptr[0] must be 0");
    for (int32_t i = 0; i < n_items; ++i) {
        if (item_ptr[i + 1] < item_ptr[i]) return fail("trainer: item_ptr is not monotone");
        if (labels[i] != 0 && labels[i] != 1) return fail("trainer: labels must be 0 or 1");
    }
    const int32_t nnz = n_items > 0 ? item_ptr[n_items] : 0;
    if (nnz > 0 && !attr_id) return fail("trainer: null argument");
    for (int32_t k = 0; k < nnz; ++k)
        if (attr_id[k] < 0 || attr_id[k] >= num_attrs) return fail("trainer: attribute id out of range");
    for (int64_t k = 0; k < int64_t(num_attrs) * 2; ++k)
        if (state_fid[k] < -1 || state_fid[k] >= num_features) return fail("trainer: state feature id out of range");
    for (int k = 0; k < 4; ++k)
        if (trans_fid[k] < -1 || trans_fid[k] >= num_features) return fail("trainer: transition feature id out of range");

    hp->A = num_attrs;
    hp->n_items = n_items;
    hp->K = num_features;
    hp->state_fid.assign(state_fid, state_fid + int64_t(num_attrs) * 2);
    hp->trans_fid.assign(trans_fid, trans_fid + 4);

    // windows (gecco/_meta.py sliding_window, no padding) and, per item, the windows covering it
    std::vector<int32_t> &win_start = hp->win_start, &iw_first = hp->iw_first, &iw_cnt = hp->iw_cnt, &iw_off = hp->iw_off;
    iw_first.assign(n_items, 0);
    iw_cnt.assign(n_items, 0);
    iw_off.assign(n_items, 0);
    for (int32_t s = 0; s < n_seqs; ++s) {
        const int32_t base = seq_ptr[s], n = seq_ptr[s + 1] - base;
        const int64_t w0 = int64_t(win_start.size());
        const int32_t nw = (n - window) / step + 1;
        for (int32_t k = 0; k < nw; ++k) win_start.push_back(base + k * step);
        for (int32_t p = 0; p < n; ++p) {
            const int32_t klo = p < window ? 0 : (p - window + step) / step;  // smallest k with k*step + W > p
            const int32_t khi = std::min(nw - 1, p / step);
            if (khi < klo) continue;
            if (w0 + klo > INT32_MAX) return fail("trainer: more than 2^31 windows");
            iw_first[base + p] = int32_t(w0 + klo);
            iw_cnt[base + p] = khi - klo + 1;
            iw_off[base + p] = p - klo * step;
        }
    }
    hp->n_win = int64_t(win_start.size());

    // empirical counts, exact (integers in doubles): state (a, y_i) once per window covering item i, transitions per window
    hp->empirical.assign(size_t(num_features), 0.0);
    for (int32_t i = 0; i < n_items; ++i)
        for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
            const int32_t fid = hp->state_fid[size_t(attr_id[k]) * 2 + labels[i]];
            if (fid >= 0) hp->empirical[fid] += iw_cnt[i];
        }
    for (int32_t i0 : win_start)
        for (int32_t j = 1; j < window; ++j) {
            const int32_t fid = hp->trans_fid[labels[i0 + j - 1] * 2 + labels[i0 + j]];
            if (fid >= 0) hp->empirical[fid] += 1.0;
        }

    // attribute -> items transpose (items ascending within every attribute)
    std::vector<int32_t> &attr_ptr = hp->attr_ptr, &attr_items = hp->attr_items;
    attr_ptr.assign(size_t(num_attrs) + 1, 0);
    attr_items.assign(static_cast<size_t>(nnz), 0);
    for (int32_t k = 0; k < nnz; ++k) ++attr_ptr[attr_id[k] + 1];
    for (int32_t a = 0; a < num_attrs; ++a) attr_ptr[a + 1] += attr_ptr[a];
    {
        std::vector<int32_t> fill(attr_ptr.begin(), attr_ptr.end() - 1);
        for (int32_t i = 0; i < n_items; ++i)
            for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) attr_items[fill[attr_id[k]]++] = i;
    }
    hp->item_ptr.assign(1, 0);
    if (n_items > 0) {
        hp->item_ptr.assign(item_ptr, item_ptr + n_items + 1);
        hp->attr_id.assign(attr_id, attr_id + nnz);
        hp->label.assign(labels, labels + n_items);
    }
    return GECCO_CRF_OK;
}

// Transition weights of w as the window kernel takes them.
TransArgs trans_args(const std::vector<int32_t> &trans_fid, const double *w) {
    TransArgs T;
    double tw[4];
    for (int k = 0; k < 4; ++k) tw[k] = trans_fid[k] >= 0 ? w[trans_fid[k]] : 0.0;
    T.t00 = tw[0], T.t01 = tw[1], T.t10 = tw[2], T.t11 = tw[3];
    T.tmax = std::max(std::max(tw[0], tw[1]), std::max(tw[2], tw[3]));
    T.e00 = std::exp(tw[0] - T.tmax), T.e01 = std::exp(tw[1] - T.tmax);
    T.e10 = std::exp(tw[2] - T.tmax), T.e11 = std::exp(tw[3] - T.tmax);
    T.log_space = 0;
    for (double e : {T.e00, T.e01, T.e10, T.e11})
        if (!(e >= DBL_MIN && e <= DBL_MAX)) T.log_space = 1;
    return T;
}

template <class T>
void append(std::vector<T> &dst, const std::vector<T> &src) {
    dst.insert(dst.end(), src.begin(), src.end());
}

static_assert(sizeof(Slot) % alignof(double) == 0, "the state weights follow the slots in the upload");

}  // namespace

// K problems resident on one device; a lone trainer is the case K = 1.  Each problem's arrays are concatenated into
// one device array per kind (ProbDev has the offsets).  Per evaluation, one upload carries the slots of the active
// problems and the state weights ([Slot][P] then the weights), one download brings back the row sums and expected
// counts of the span of problems from the first active one to the last.
struct Trainer {
    int device = 0;
    int32_t W = 0, step = 1;
    struct Meta {
        int32_t A, n_items, K;
        int64_t n_win;
        std::vector<int32_t> state_fid, trans_fid;
        std::vector<double> empirical;
    };
    std::vector<Meta> probs;
    std::vector<ProbDev> layout;
    size_t slots_bytes = 0;
    std::vector<unsigned char> h_in;  // host staging of the upload
    std::vector<double> h_out;        // host staging of the download
    hipStream_t stream = nullptr;
    // device: training sets (uploaded once) and per-evaluation work space
    ProbDev *d_probs = nullptr;
    int32_t *d_item_ptr = nullptr, *d_attr_id = nullptr, *d_label = nullptr, *d_win_start = nullptr;
    int32_t *d_iw_first = nullptr, *d_iw_cnt = nullptr, *d_iw_off = nullptr;
    int32_t *d_attr_ptr = nullptr, *d_attr_items = nullptr;
    unsigned char *d_in = nullptr;
    double *d_out = nullptr, *d_rows = nullptr, *d_partial = nullptr;
    double2 *d_score = nullptr, *d_marg = nullptr, *d_item_marg = nullptr;

    ~Trainer() {
        int prev = -1;
        const bool restore = hipGetDevice(&prev) == hipSuccess && prev != device;
        (void)hipSetDevice(device);
        for (void *p : {(void *)d_probs, (void *)d_item_ptr, (void *)d_attr_id, (void *)d_label, (void *)d_win_start,
                        (void *)d_iw_first, (void *)d_iw_cnt, (void *)d_iw_off, (void *)d_attr_ptr, (void *)d_attr_items,
                        (void *)d_in, (void *)d_out, (void *)d_rows, (void *)d_partial, (void *)d_score, (void *)d_marg,
                        (void *)d_item_marg})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (restore && prev >= 0) (void)hipSetDevice(prev);
    }
};

namespace {

// `batch`: errors name the problem ("problem k: ..."); a lone trainer keeps its own messages.
int create_impl(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                const int32_t *num_attrs, const int32_t *num_labels, int32_t window, int32_t step,
                const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features, bool batch,
                Trainer **out) {
    auto t = std::make_unique<Trainer>();
    t->device = device;
    t->W = window;
    t->step = step;
    std::vector<int32_t> item_ptr_c, attr_id_c, label_c, win_start_c, iw_first_c, iw_cnt_c, iw_off_c, attr_ptr_c, attr_items_c;
    int64_t ws_total = 0, out_total = 0, blocks[3] = {0, 0, 0};
    for (int32_t k = 0; k < n_problems; ++k) {
        HostProblem hp;
        int rc = build_problem(seq_ptr[k], n_seqs[k], item_ptr[k], attr_id[k], labels[k], num_attrs[k], num_labels[k],
                               window, step, state_fid[k], trans_fid[k], num_features[k], &hp);
        if (rc) {
            if (batch) set_error("trainer batch: problem " + std::to_string(k) + ": " + last_error());
            return rc;
        }
        ProbDev d;
        d.item0 = int64_t(label_c.size());
        d.iptr0 = int64_t(item_ptr_c.size());
        d.nnz0 = int64_t(attr_id_c.size());
        d.win0 = int64_t(win_start_c.size());
        d.aptr0 = int64_t(attr_ptr_c.size());
        d.ws0 = ws_total;
        d.out0 = out_total;
        d.n_win = hp.n_win;
        d.n_items = hp.n_items;
        d.A = hp.A;
        ws_total += int64_t(hp.A) * 2;
        out_total += kTrainRowCols + int64_t(hp.A) * 2;
        blocks[kGridItems] += (hp.n_items + kTrainThreads - 1) / kTrainThreads;
        blocks[kGridWindows] += (hp.n_win + kTrainWinThreads - 1) / kTrainWinThreads;
        blocks[kGridAttrs] += hp.A;
        append(item_ptr_c, hp.item_ptr);
        append(attr_id_c, hp.attr_id);
        append(label_c, hp.label);
        append(win_start_c, hp.win_start);
        append(iw_first_c, hp.iw_first);
        append(iw_cnt_c, hp.iw_cnt);
        append(iw_off_c, hp.iw_off);
        append(attr_ptr_c, hp.attr_ptr);
        append(attr_items_c, hp.attr_items);
        t->layout.push_back(d);
        t->probs.push_back({hp.A, hp.n_items, hp.K, hp.n_win, std::move(hp.state_fid), std::move(hp.trans_fid),
                            std::move(hp.empirical)});
    }
    for (int64_t b : blocks)
        if (b > INT32_MAX) return fail("trainer batch: the problems need more than 2^31 workgroups in one launch");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return GECCO_CRF_ENODEV;
    }
    if (device < 0 || device >= ndev) {
        set_error("device index out of range");
        return GECCO_CRF_ENODEV;
    }
    t->slots_bytes = size_t(n_problems) * sizeof(Slot);
    t->h_in.assign(t->slots_bytes + size_t(ws_total) * sizeof(double), 0);
    t->h_out.assign(size_t(out_total), 0.0);
    const size_t n_win = win_start_c.size(), n_items = label_c.size();

    int rc = check_hip(hipSetDevice(device), "hipSetDevice");
    if (rc) return rc;
    if ((rc = check_hip(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking), "hipStreamCreate"))) return rc;
    if ((rc = dev_upload(&t->d_probs, t->layout, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_item_ptr, item_ptr_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_id, attr_id_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_label, label_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_win_start, win_start_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_first, iw_first_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_cnt, iw_cnt_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_off, iw_off_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_ptr, attr_ptr_c, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_items, attr_items_c, "trainer upload"))) return rc;
    if ((rc = dev_alloc(&t->d_in, t->h_in.size(), "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_out, t->h_out.size(), "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_rows, n_win * kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_partial, size_t(n_problems) * kTrainReduceBlocks * kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_score, n_items, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_marg, n_win * size_t(window), "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_item_marg, n_items, "trainer alloc"))) return rc;
    *out = t.release();
    return GECCO_CRF_OK;
}

}  // namespace

int trainer_create(int32_t device, const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                   const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                   const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, Trainer **out) {
    if (!out) return fail("trainer: null argument");
    *out = nullptr;
    return create_impl(device, 1, &seq_ptr, &n_seqs, &item_ptr, &attr_id, &labels, &num_attrs, &num_labels, window, step,
                       &state_fid, &trans_fid, &num_features, false, out);
}

int trainer_batch_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                         const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                         const int32_t *num_attrs, const int32_t *num_labels, int32_t window, int32_t step,
                         const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                         Trainer **out) {
    if (!out) return fail("trainer batch: null argument");
    *out = nullptr;
    if (n_problems < 1) return fail("trainer batch: at least one problem is needed");
    if (!seq_ptr || !n_seqs || !item_ptr || !attr_id || !labels || !num_attrs || !num_labels || !state_fid || !trans_fid ||
        !num_features)
        return fail("trainer batch: null argument");
    return create_impl(device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels, window, step,
                       state_fid, trans_fid, num_features, true, out);
}

int trainer_batch_eval(Trainer *t, const uint8_t *active, const double *const *w, double *f, double *const *g) {
    if (!t || !active || !w || !f || !g) return fail("trainer_batch_eval: null argument");
    const int32_t P = int32_t(t->probs.size());
    for (int32_t k = 0; k < P; ++k)
        if (active[k] && (!g[k] || (t->probs[k].K > 0 && !w[k])))
            return fail("trainer_batch_eval: null argument for problem " + std::to_string(k));
    Slot *slots = reinterpret_cast<Slot *>(t->h_in.data());
    double *wstate = reinterpret_cast<double *>(t->h_in.data() + t->slots_bytes);
    int n_slots = 0;
    int32_t blk[3] = {0, 0, 0};
    size_t in_hi = 0;
    int64_t out_lo = INT64_MAX, out_hi = 0;
    for (int32_t k = 0; k < P; ++k) {
        if (!active[k]) continue;
        const Trainer::Meta &p = t->probs[k];
        const ProbDev &d = t->layout[k];
        if (p.n_win == 0) continue;
        double *ws = wstate + d.ws0;
        for (size_t j = 0; j < p.state_fid.size(); ++j) ws[j] = p.state_fid[j] >= 0 ? w[k][p.state_fid[j]] : 0.0;
        in_hi = t->slots_bytes + size_t(d.ws0 + 2 * int64_t(p.A)) * sizeof(double);
        Slot &s = slots[n_slots++];
        s.T = trans_args(p.trans_fid, w[k]);
        s.prob = k;
        for (int G = 0; G < 3; ++G) s.blk[G] = blk[G];
        blk[kGridItems] += (p.n_items + kTrainThreads - 1) / kTrainThreads;
        blk[kGridWindows] += int32_t((p.n_win + kTrainWinThreads - 1) / kTrainWinThreads);
        blk[kGridAttrs] += p.A;
        out_lo = std::min(out_lo, d.out0);
        out_hi = d.out0 + kTrainRowCols + 2 * int64_t(p.A);
    }

    int rc = check_hip(hipSetDevice(t->device), "hipSetDevice");
    if (rc) return rc;
    hipStream_t st = t->stream;
    if (n_slots > 0) {
        const Slot *d_slots = reinterpret_cast<const Slot *>(t->d_in);
        const double *d_wstate = reinterpret_cast<const double *>(t->d_in + t->slots_bytes);
        if ((rc = check_hip(hipMemcpyAsync(t->d_in, t->h_in.data(), in_hi, hipMemcpyHostToDevice, st), "trainer weights upload")))
            return rc;
        train_item_scores<<<blk[kGridItems], kTrainThreads, 0, st>>>(d_slots, n_slots, t->d_probs, t->d_item_ptr,
                                                                     t->d_attr_id, d_wstate, t->d_score);
        const size_t lds = size_t(t->W) * kTrainWinThreads * 3 * sizeof(double);
        train_windows<<<dim3(unsigned(blk[kGridWindows])), kTrainWinThreads, lds, st>>>(
            d_slots, n_slots, t->d_probs, t->d_score, t->d_label, t->d_win_start, t->W, t->d_marg, t->d_rows);
        train_item_marginals<<<blk[kGridItems], kTrainThreads, 0, st>>>(d_slots, n_slots, t->d_probs, t->d_marg,
                                                                        t->d_iw_first, t->d_iw_cnt, t->d_iw_off, t->W,
                                                                        t->step, t->d_item_marg);
        train_attr_counts<<<blk[kGridAttrs], kTrainThreads, 0, st>>>(d_slots, n_slots, t->d_probs, t->d_attr_ptr,
                                                                     t->d_attr_items, t->d_item_marg, t->d_out);
        train_reduce_rows<<<n_slots * kTrainReduceBlocks, kTrainThreads, 0, st>>>(d_slots, t->d_probs, t->d_rows,
                                                                                  t->d_partial);
        train_reduce_final<<<n_slots, kTrainReduceBlocks, 0, st>>>(d_slots, t->d_probs, t->d_partial, t->d_out);
        if ((rc = check_hip(hipGetLastError(), "trainer kernels"))) return rc;
        if ((rc = check_hip(hipMemcpyAsync(t->h_out.data() + out_lo, t->d_out + out_lo,
                                           size_t(out_hi - out_lo) * sizeof(double), hipMemcpyDeviceToHost, st),
                            "trainer download")))
            return rc;
        if ((rc = check_hip(hipStreamSynchronize(st), "trainer synchronize"))) return rc;
    }
    std::vector<double> zeros;
    for (int32_t k = 0; k < P; ++k) {
        if (!active[k]) continue;
        const Trainer::Meta &p = t->probs[k];
        const double *o = t->h_out.data() + t->layout[k].out0;  // row sums, then expected state counts
        if (p.n_win == 0) {
            zeros.assign(kTrainRowCols + 2 * size_t(p.A), 0.0);
            o = zeros.data();
        }
        const double *expected = o + kTrainRowCols;
        double *gk = g[k];
        f[k] = o[0];
        for (int32_t j = 0; j < p.K; ++j) gk[j] = -p.empirical[j];
        for (size_t j = 0; j < p.state_fid.size(); ++j)
            if (p.state_fid[j] >= 0) gk[p.state_fid[j]] += expected[j];
        for (int j = 0; j < 4; ++j)
            if (p.trans_fid[j] >= 0) gk[p.trans_fid[j]] += o[1 + j];
    }
    return GECCO_CRF_OK;
}

int trainer_eval(Trainer *t, const double *w, double *f, double *g) {
    if (!t || !f || !g || (t->probs[0].K > 0 && !w)) return fail("trainer_eval: null argument");
    const uint8_t active = 1;
    return trainer_batch_eval(t, &active, &w, f, &g);
}

int32_t trainer_num_problems(const Trainer *t) { return t ? int32_t(t->probs.size()) : -1; }

int64_t trainer_num_windows(const Trainer *t, int32_t k) {
    return (t && k >= 0 && k < int32_t(t->probs.size())) ? t->probs[k].n_win : -1;
}

void trainer_destroy(Trainer *t) { delete t; }

}  // namespace gecco
