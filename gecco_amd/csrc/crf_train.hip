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
#include "crf_train_host.hpp"

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

constexpr int kTrainSetProbs = 8;        // problems of one set whose item scores one thread forms from one read

// One training set as the device holds it (uploaded once).  Indices inside it (item_ptr, win_start, iw_first, attr_ptr,
// attr_items) are local to the set: exactly what a lone trainer of it holds.  Every problem on the set reads these.
struct SetDev {
    int64_t item0;  // items: label, iw_first/cnt/off
    int64_t iptr0;  // item_ptr (n_items + 1 entries)
    int64_t nnz0;   // attr_id, attr_items
    int64_t win0;   // win_start
    int64_t aptr0;  // attr_ptr (A + 1 entries)
    int64_t n_win;
    int32_t n_items, A, W, step;
};

// One problem of one evaluation group (uploaded with the weights): its set, transitions, state weights, scratch and
// outputs, and the first block it owns in the window grid (kernel 2) and the attribute grid (4).  Kernels 5 and 6 give
// every slot 256 and 1 blocks.  Only active problems with windows get a slot, so every slot owns at least one block of
// every grid.
struct Slot {
    TransArgs T;
    int64_t ws0;   // state weights in the upload ([A][2] doubles)
    int64_t sc0;   // scratch, in bytes (16-aligned): see scratch_bytes
    int64_t out0;  // outputs in the download: 5 row sums, then the expected state counts [A][2]
    int32_t set;
    int32_t blk[2];
};
enum { kGridWindows = 0, kGridAttrs = 1 };

// Kernels 1 and 3 cover the items of one set for up to kTrainSetProbs of its problems (slot indices in the group).
struct ItemGroup {
    int32_t set, n, blk;
    int32_t slot[kTrainSetProbs];
};

// A problem's scratch: item scores [n_items], item marginals [n_items], node marginals [n_win][W], rows [n_win][5].
__host__ __device__ __forceinline__ int64_t scratch_bytes(int64_t n_items, int64_t n_win, int32_t W) {
    return (32 * n_items + 16 * n_win * W + 8 * kTrainRowCols * n_win + 15) / 16 * 16;
}
__device__ __forceinline__ double2 *scratch_score(unsigned char *sc, const Slot &sl) {
    return reinterpret_cast<double2 *>(sc + sl.sc0);
}
__device__ __forceinline__ double2 *scratch_item_marg(unsigned char *sc, const Slot &sl, const SetDev &S) {
    return scratch_score(sc, sl) + S.n_items;
}
__device__ __forceinline__ double2 *scratch_marg(unsigned char *sc, const Slot &sl, const SetDev &S) {
    return scratch_score(sc, sl) + 2 * static_cast<int64_t>(S.n_items);
}
__device__ __forceinline__ double *scratch_rows(unsigned char *sc, const Slot &sl, const SetDev &S) {
    return reinterpret_cast<double *>(scratch_marg(sc, sl, S) + S.n_win * S.W);
}

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

// The same for the item grid of kernels 1 and 3.
__device__ __forceinline__ int item_group_of(const ItemGroup *__restrict__ igs, int n_igs) {
    const int32_t b = static_cast<int32_t>(blockIdx.x);
    int lo = 0, hi = n_igs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (igs[mid].blk <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One thread per item of a set: the item's attribute ids are read once, and each problem of the item group (at most
// NP) sums its own state weights over them in CSR order, as a lone trainer does.
template <int NP>
__global__ void __launch_bounds__(kTrainThreads) train_item_scores(const ItemGroup *__restrict__ igs, int n_igs,
                                                                   const Slot *__restrict__ slots,
                                                                   const SetDev *__restrict__ sets,
                                                                   const int32_t *__restrict__ item_ptr_all,
                                                                   const int32_t *__restrict__ attr_id_all,
                                                                   const double *__restrict__ wstate_all,
                                                                   unsigned char *__restrict__ scratch) {
    const ItemGroup &ig = igs[item_group_of(igs, n_igs)];
    const SetDev &S = sets[ig.set];
    const int32_t i = (static_cast<int32_t>(blockIdx.x) - ig.blk) * blockDim.x + threadIdx.x;
    if (i >= S.n_items) return;
    const int n = ig.n;
    const int32_t *__restrict__ item_ptr = item_ptr_all + S.iptr0;
    const int32_t *__restrict__ attr_id = attr_id_all + S.nnz0;
    const double *wstate[NP];
    double s0[NP], s1[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        wstate[j] = wstate_all + slots[ig.slot[j < n ? j : 0]].ws0;
        s0[j] = 0.0;
        s1[j] = 0.0;
    }
    for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
        const int32_t a = attr_id[k];
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (j < n) {
                s0[j] += wstate[j][2 * a];
                s1[j] += wstate[j][2 * a + 1];
            }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j)
        if (j < n) scratch_score(scratch, slots[ig.slot[j]])[i] = make_double2(s0[j], s1[j]);
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
// The transitions (and the log-space flag) are the problem's own, read from its slot; W is its set's.  The LDS holds
// lds_w >= W steps (the largest W of the group).
__global__ void __launch_bounds__(kTrainWinThreads) __attribute__((amdgpu_waves_per_eu(6)))
train_windows(const Slot *__restrict__ slots, int n_slots, const SetDev *__restrict__ sets,
              const int32_t *__restrict__ label_all, const int32_t *__restrict__ win_start_all, int32_t lds_w,
              unsigned char *__restrict__ scratch) {
    extern __shared__ double lds[];
    double2 *alpha = reinterpret_cast<double2 *>(lds);                        // [W][kTrainWinThreads]
    double *cnorm = lds + 2 * static_cast<size_t>(lds_w) * kTrainWinThreads;  // [W][kTrainWinThreads]
    const Slot &sl = slots[slot_of<kGridWindows>(slots, n_slots)];
    const SetDev &S = sets[sl.set];
    const int lane = threadIdx.x;
    const int64_t w = static_cast<int64_t>(static_cast<int32_t>(blockIdx.x) - sl.blk[kGridWindows]) * kTrainWinThreads + lane;
    if (w >= S.n_win) return;
    const int32_t W = S.W;
    const TransArgs T = sl.T;
    const double2 *__restrict__ score = scratch_score(scratch, sl);
    const int32_t *__restrict__ label = label_all + S.item0;
    const int32_t *__restrict__ win_start = win_start_all + S.win0;
    double2 *__restrict__ marg = scratch_marg(scratch, sl, S);
    double *__restrict__ rows = scratch_rows(scratch, sl, S);
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

// Item i is covered by the windows first .. first + cnt - 1, at position off, off - step, ... in them.  The coverage is
// read once for the item group; each problem sums its own node marginals in window order.
__global__ void __launch_bounds__(kTrainThreads) train_item_marginals(const ItemGroup *__restrict__ igs, int n_igs,
                                                                      const Slot *__restrict__ slots,
                                                                      const SetDev *__restrict__ sets,
                                                                      const int32_t *__restrict__ iw_first_all,
                                                                      const int32_t *__restrict__ iw_cnt_all,
                                                                      const int32_t *__restrict__ iw_off_all,
                                                                      unsigned char *__restrict__ scratch) {
    const ItemGroup &ig = igs[item_group_of(igs, n_igs)];
    const SetDev &S = sets[ig.set];
    const int32_t i = (static_cast<int32_t>(blockIdx.x) - ig.blk) * blockDim.x + threadIdx.x;
    if (i >= S.n_items) return;
    const int32_t W = S.W, step = S.step;
    const int64_t first = iw_first_all[S.item0 + i];
    const int32_t cnt = iw_cnt_all[S.item0 + i];
    const int32_t off0 = iw_off_all[S.item0 + i];
    for (int j = 0; j < ig.n; ++j) {
        const Slot &sl = slots[ig.slot[j]];
        const double2 *__restrict__ marg = scratch_marg(scratch, sl, S);
        int32_t off = off0;
        double p0 = 0.0, p1 = 0.0;
        for (int32_t k = 0; k < cnt; ++k, off -= step) {
            const double2 v = marg[(first + k) * W + off];
            p0 += v.x;
            p1 += v.y;
        }
        scratch_item_marg(scratch, sl, S)[i] = make_double2(p0, p1);
    }
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
                                                                   const SetDev *__restrict__ sets,
                                                                   const int32_t *__restrict__ attr_ptr_all,
                                                                   const int32_t *__restrict__ attr_items_all,
                                                                   unsigned char *__restrict__ scratch,
                                                                   double *__restrict__ out_all) {
    __shared__ double2 sh[kTrainThreads];
    const Slot &sl = slots[slot_of<kGridAttrs>(slots, n_slots)];
    const SetDev &S = sets[sl.set];
    const int32_t a = static_cast<int32_t>(blockIdx.x) - sl.blk[kGridAttrs];
    if (a >= S.A) return;
    const int32_t *__restrict__ attr_ptr = attr_ptr_all + S.aptr0;
    const int32_t *__restrict__ attr_items = attr_items_all + S.nnz0;
    const double2 *__restrict__ item_marg = scratch_item_marg(scratch, sl, S);
    double2 acc = make_double2(0.0, 0.0);
    for (int32_t k = attr_ptr[a] + threadIdx.x; k < attr_ptr[a + 1]; k += kTrainThreads) {
        const double2 v = item_marg[attr_items[k]];
        acc.x += v.x;
        acc.y += v.y;
    }
    const double2 tot = block_sum2<kTrainThreads>(acc, sh);
    if (threadIdx.x == 0) {
        double *expected = out_all + sl.out0 + kTrainRowCols;
        expected[2 * a] = tot.x;
        expected[2 * a + 1] = tot.y;
    }
}

// Row sums, stage 1: slot s owns the blocks [s * kTrainReduceBlocks, (s + 1) * kTrainReduceBlocks); its slab b = rows
// [b * chunk, (b + 1) * chunk) of its problem, chunk = ceil(n_win / kTrainReduceBlocks).
__global__ void __launch_bounds__(kTrainThreads) train_reduce_rows(const Slot *__restrict__ slots,
                                                                   const SetDev *__restrict__ sets,
                                                                   unsigned char *__restrict__ scratch,
                                                                   double *__restrict__ partial_all) {
    __shared__ double sh[kTrainRowCols][kTrainThreads];
    const int s = blockIdx.x / kTrainReduceBlocks, b = blockIdx.x % kTrainReduceBlocks;
    const Slot &sl = slots[s];
    const SetDev &S = sets[sl.set];
    const double *__restrict__ rows = scratch_rows(scratch, sl, S);
    const int64_t n = S.n_win;
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
    if (threadIdx.x < kTrainRowCols) out_all[slots[blockIdx.x].out0 + threadIdx.x] = sh[threadIdx.x][0];
}

}  // namespace

int build_problem(const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                  const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                  const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, int32_t max_labels,
                  HostProblem *hp, bool whole_sequences, const double *attr_value, const double *seq_weight) {
    if (!seq_ptr || n_seqs < 0 || !state_fid || !trans_fid) return fail("trainer: null argument");
    if (max_labels == 2 && num_labels != 2) {
        set_error("trainer: only 2-label models can be trained (GECCO's protein and domain modes are binary)");
        return GECCO_CRF_EUNSUPPORTED;
    }
    if (num_labels < 2 || num_labels > max_labels) {
        set_error("trainer: " + std::to_string(num_labels) + " labels; models of 2 to " + std::to_string(max_labels) +
                  " labels can be trained");
        return GECCO_CRF_EUNSUPPORTED;
    }
    const int32_t L = num_labels;
    if (!whole_sequences) {
        if (window < 1 || window > kTrainMaxW) {
            set_error("trainer: window of " + std::to_string(window) + " items; windows of 1 to 32 items are supported");
            return GECCO_CRF_EUNSUPPORTED;
        }
        if (step < 1 || step > window) return fail("Window step must be strictly positive and under `window_size`");
    }
    if (num_attrs < 1 || num_features < 0) return fail("trainer: bad attribute or feature count");
    if (seq_ptr[0] != 0) return fail("trainer: seq_ptr[0] must be 0");
    for (int32_t s = 0; s < n_seqs; ++s) {
        const int64_t n = int64_t(seq_ptr[s + 1]) - seq_ptr[s];
        if (whole_sequences && n < 0) return fail("trainer: seq_ptr is not monotone");
        if (whole_sequences && n == 0) return fail("trainer: sequence " + std::to_string(s) + " has no items");
        if (!whole_sequences && n < window)
            return fail("trainer: sequence " + std::to_string(s) + " has fewer items than the window");
    }
    const int32_t n_items = seq_ptr[n_seqs];
    if (n_items > 0 && (!item_ptr || !labels)) return fail("trainer: null argument");
    if (n_items > 0 && item_ptr[0] != 0) return fail("trainer: item_ptr[0] must be 0");
    for (int32_t i = 0; i < n_items; ++i) {
        if (item_ptr[i + 1] < item_ptr[i]) return fail("trainer: item_ptr is not monotone");
        if (labels[i] < 0 || labels[i] >= L)
            return fail(max_labels == 2 ? "trainer: labels must be 0 or 1" : "trainer: labels must lie in [0, num_labels)");
    }
    const int32_t nnz = n_items > 0 ? item_ptr[n_items] : 0;
    if (nnz > 0 && !attr_id) return fail("trainer: null argument");
    for (int32_t k = 0; k < nnz; ++k)
        if (attr_id[k] < 0 || attr_id[k] >= num_attrs) return fail("trainer: attribute id out of range");
    for (int32_t k = 0; attr_value && k < nnz; ++k)
        if (!std::isfinite(attr_value[k]))
            return fail("trainer: attribute value " + std::to_string(k) + " is not finite (NaN or infinite)");
    for (int64_t k = 0; k < int64_t(num_attrs) * L; ++k)
        if (state_fid[k] < -1 || state_fid[k] >= num_features) return fail("trainer: state feature id out of range");
    for (int k = 0; k < L * L; ++k)
        if (trans_fid[k] < -1 || trans_fid[k] >= num_features) return fail("trainer: transition feature id out of range");

    hp->A = num_attrs;
    hp->n_items = n_items;
    hp->K = num_features;
    hp->state_fid.assign(state_fid, state_fid + int64_t(num_attrs) * L);
    hp->trans_fid.assign(trans_fid, trans_fid + L * L);

    // windows (gecco/_meta.py sliding_window, no padding) and, per item, the windows covering it
    std::vector<int32_t> &win_start = hp->win_start, &iw_first = hp->iw_first, &iw_cnt = hp->iw_cnt, &iw_off = hp->iw_off;
    iw_first.assign(n_items, 0);
    iw_cnt.assign(n_items, 0);
    iw_off.assign(n_items, 0);
    if (whole_sequences) {
        // one instance per sequence, in slot order: longest first, ties by index (the sequence kernel runs neighbours of
        // this order side by side); every item lies in exactly one instance
        std::vector<int32_t> order(static_cast<size_t>(n_seqs));
        for (int32_t s = 0; s < n_seqs; ++s) order[s] = s;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return seq_ptr[a + 1] - seq_ptr[a] > seq_ptr[b + 1] - seq_ptr[b];
        });
        for (int32_t s : order) {
            win_start.push_back(seq_ptr[s]);
            hp->win_len.push_back(seq_ptr[s + 1] - seq_ptr[s]);
            if (seq_weight) hp->inst_weight.push_back(seq_weight[s]);  // (the weight follows its sequence into the slot order)
        }
        iw_cnt.assign(n_items, 1);
    }
    for (int32_t s = 0; s < n_seqs && !whole_sequences; ++s) {
        const int32_t base = seq_ptr[s], n = seq_ptr[s + 1] - base;
        const int64_t w0 = int64_t(win_start.size());
        const int32_t nw = (n - window) / step + 1;
        for (int32_t k = 0; k < nw; ++k) win_start.push_back(base + k * step);
        if (seq_weight) hp->inst_weight.insert(hp->inst_weight.end(), size_t(nw), seq_weight[s]);
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
    for (int32_t i = 0, s = 0; i < n_items; ++i) {
        while (seq_weight && i >= seq_ptr[s + 1]) ++s;  // (the sequence of item i: only a weighted problem asks)
        for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
            const int32_t fid = hp->state_fid[size_t(attr_id[k]) * L + labels[i]];
            if (fid < 0) continue;
            // (with values: value x coverage, in this one order; a value of 1 adds the integer it always added.  With sequence
            // weights: that term times the weight of the item's sequence)
            const double term = attr_value ? attr_value[k] * iw_cnt[i] : iw_cnt[i];
            hp->empirical[fid] += seq_weight ? term * seq_weight[s] : term;
        }
    }
    for (size_t q = 0; q < win_start.size(); ++q)
        for (int32_t i0 = win_start[q], j = 1; j < (whole_sequences ? hp->win_len[q] : window); ++j) {
            const int32_t fid = hp->trans_fid[labels[i0 + j - 1] * L + labels[i0 + j]];
            if (fid >= 0) hp->empirical[fid] += seq_weight ? hp->inst_weight[q] : 1.0;
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
    if (attr_value) {  // the transpose carries the value beside the item index
        hp->attr_value.assign(attr_value, attr_value + nnz);
        hp->attr_item_value.assign(static_cast<size_t>(nnz), 0.0);
        std::vector<int32_t> fill(attr_ptr.begin(), attr_ptr.end() - 1);
        for (int32_t k = 0; k < nnz; ++k) hp->attr_item_value[fill[attr_id[k]]++] = attr_value[k];
    }
    hp->item_ptr.assign(1, 0);
    if (n_items > 0) {
        hp->item_ptr.assign(item_ptr, item_ptr + n_items + 1);
        hp->attr_id.assign(attr_id, attr_id + nnz);
        hp->label.assign(labels, labels + n_items);
    }
    return GECCO_CRF_OK;
}

namespace {

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

static_assert(sizeof(Slot) % alignof(double) == 0 && sizeof(ItemGroup) % alignof(int32_t) == 0, "upload layout");

}  // namespace

// Training sets and problems resident on one device.  A set is a training set, uploaded once (every set's arrays
// concatenated into one device array per kind, SetDev has the offsets); a problem is a set with its own weights,
// scratch and outputs.  A lone trainer is one set with one problem, a batch K sets with problem k on set k.
// Per evaluation, the active problems are cut, in order, into groups whose scratch fits the work space; one upload
// carries every group's slots and item groups and the active problems' state weights, every group runs the six
// kernels, and one download brings back the row sums and expected counts of the span of problems from the first active
// one to the last.
struct Trainer {
    DeviceScope home{DeviceScope::kLater};  // (first member: see ~Trainer)
    int device = -1;  // set once the device has been checked
    std::string family;  // "batch" / "grid" in error messages; empty: a lone trainer, which keeps its own messages
    struct Set {
        int32_t A, n_items, K, W;
        int64_t n_win;
        std::vector<int32_t> state_fid, trans_fid;
        std::vector<double> empirical;
    };
    struct Prob {
        int32_t set;
        int64_t ws0, out0, scratch;  // state weights in the upload, outputs in the download, scratch bytes
    };
    std::vector<Set> sets;
    std::vector<Prob> probs;
    size_t igs_off = 0, ws_off = 0;  // upload: [Slot][ItemGroup] (at most one of each per problem), then the weights
    int64_t scratch_cap = 0;         // bytes of d_scratch: the most one group may use
    std::vector<unsigned char> h_in;  // host staging of the upload
    std::vector<double> h_out;        // host staging of the download
    Stream stream;
    // device: training sets (uploaded once) and per-evaluation work space
    DeviceBlock<SetDev> d_sets;
    DeviceBlock<int32_t> d_item_ptr, d_attr_id, d_label, d_win_start, d_iw_first, d_iw_cnt, d_iw_off, d_attr_ptr, d_attr_items;
    DeviceBlock<unsigned char> d_in, d_scratch;
    DeviceBlock<double> d_out, d_partial;

    // The members free themselves, in reverse order, after this body: with the trainer's device current, and `home` hands the
    // caller's device back at the end.
    ~Trainer() { home.enter(device); }
};

// Sets as build_problem takes them.  A set's error names it after what the caller numbers: the set where problems pick
// their sets (problem_set), the problem where problem k is set k.
int trainer_create(int32_t device, int32_t n_sets, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                   const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                   const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                   const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                   int32_t n_problems, const int32_t *problem_set, int64_t scratch_budget, const char *family,
                   Trainer **out) {
    auto t = std::make_unique<Trainer>();
    if (family) t->family = family;
    std::vector<int32_t> item_ptr_c, attr_id_c, label_c, win_start_c, iw_first_c, iw_cnt_c, iw_off_c, attr_ptr_c, attr_items_c;
    std::vector<SetDev> layout;
    for (int32_t k = 0; k < n_sets; ++k) {
        HostProblem hp;
        int rc = build_problem(seq_ptr[k], n_seqs[k], item_ptr[k], attr_id[k], labels[k], num_attrs[k], num_labels[k],
                               window[k], step[k], state_fid[k], trans_fid[k], num_features[k], 2, &hp);
        if (rc) {
            if (family)
                set_error("trainer " + t->family + (problem_set ? ": set " : ": problem ") + std::to_string(k) + ": " +
                          last_error());
            return rc;
        }
        SetDev d;
        d.item0 = int64_t(label_c.size());
        d.iptr0 = int64_t(item_ptr_c.size());
        d.nnz0 = int64_t(attr_id_c.size());
        d.win0 = int64_t(win_start_c.size());
        d.aptr0 = int64_t(attr_ptr_c.size());
        d.n_win = hp.n_win;
        d.n_items = hp.n_items;
        d.A = hp.A;
        d.W = window[k];
        d.step = step[k];
        append(item_ptr_c, hp.item_ptr);
        append(attr_id_c, hp.attr_id);
        append(label_c, hp.label);
        append(win_start_c, hp.win_start);
        append(iw_first_c, hp.iw_first);
        append(iw_cnt_c, hp.iw_cnt);
        append(iw_off_c, hp.iw_off);
        append(attr_ptr_c, hp.attr_ptr);
        append(attr_items_c, hp.attr_items);
        layout.push_back(d);
        t->sets.push_back({hp.A, hp.n_items, hp.K, window[k], hp.n_win, std::move(hp.state_fid), std::move(hp.trans_fid),
                           std::move(hp.empirical)});
    }
    int64_t ws_total = 0, out_total = 0, scratch_total = 0, scratch_max = 0, blocks[3] = {0, 0, 0};
    for (int32_t k = 0; k < n_problems; ++k) {
        const int32_t s = problem_set ? problem_set[k] : k;
        if (s < 0 || s >= n_sets)
            return fail("trainer grid: problem " + std::to_string(k) + ": set " + std::to_string(s) + " out of range");
        const Trainer::Set &S = t->sets[size_t(s)];
        const int64_t sc = scratch_bytes(S.n_items, S.n_win, S.W);
        t->probs.push_back({s, ws_total, out_total, sc});
        ws_total += int64_t(S.A) * 2;
        out_total += kTrainRowCols + int64_t(S.A) * 2;
        scratch_total += sc;
        scratch_max = std::max(scratch_max, sc);
        blocks[0] += blocks_of(S.n_items, kTrainThreads);
        blocks[1] += blocks_of(S.n_win, kTrainWinThreads);
        blocks[2] += S.A;
    }
    // (with a scratch budget the evaluation runs in groups, and cuts them at 2^31 workgroups as well)
    if (!problem_set)
        for (int64_t b : blocks)
            if (b > INT32_MAX) return fail("trainer batch: the problems need more than 2^31 workgroups in one launch");
    t->scratch_cap = scratch_total;
    if (scratch_budget > 0) t->scratch_cap = std::max(scratch_max, std::min(scratch_budget, scratch_total));
    int rc = check_device(device);
    if (rc) return rc;
    t->device = device;
    t->igs_off = size_t(n_problems) * sizeof(Slot);
    t->ws_off = (t->igs_off + size_t(n_problems) * sizeof(ItemGroup) + 15) / 16 * 16;
    t->h_in.assign(t->ws_off + size_t(ws_total) * sizeof(double), 0);
    t->h_out.assign(size_t(out_total), 0.0);

    if ((rc = set_device(device))) return rc;
    if ((rc = t->stream.create())) return rc;
    if ((rc = t->d_sets.upload(layout, "trainer upload"))) return rc;
    if ((rc = t->d_item_ptr.upload(item_ptr_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_id.upload(attr_id_c, "trainer upload"))) return rc;
    if ((rc = t->d_label.upload(label_c, "trainer upload"))) return rc;
    if ((rc = t->d_win_start.upload(win_start_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_first.upload(iw_first_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_cnt.upload(iw_cnt_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_off.upload(iw_off_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_ptr.upload(attr_ptr_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_items.upload(attr_items_c, "trainer upload"))) return rc;
    if ((rc = t->d_in.alloc(t->h_in.size(), "trainer alloc"))) return rc;
    if ((rc = t->d_out.alloc(t->h_out.size(), "trainer alloc"))) return rc;
    if ((rc = t->d_partial.alloc(size_t(n_problems) * kTrainReduceBlocks * kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = t->d_scratch.alloc(size_t(t->scratch_cap), "trainer alloc"))) return rc;
    *out = t.release();
    return GECCO_CRF_OK;
}

namespace {

// One group of an evaluation: slots [s0, s1) and item groups [g0, g1) of the upload, its grids, the largest W and the
// most problems of one item group.
struct Group {
    int s0, s1, g0, g1;
    int64_t blk_items, blk_win, blk_attr;
    int32_t lds_w, np;
};

template <int NP>
void launch_item_scores(const Group &gr, const ItemGroup *igs, const Slot *slots, const Trainer *t, const double *wstate,
                        hipStream_t st) {
    train_item_scores<NP><<<dim3(unsigned(gr.blk_items)), kTrainThreads, 0, st>>>(
        igs, gr.g1 - gr.g0, slots, t->d_sets.get(), t->d_item_ptr.get(), t->d_attr_id.get(), wstate, t->d_scratch.get());
}

}  // namespace

int trainer_eval(Trainer *t, const uint8_t *active, const double *const *w, double *f, double *const *g) {
    const bool lone = !t || t->family.empty();
    const std::string name = lone ? "trainer_eval" : "trainer_" + t->family + "_eval";
    if (!t || !active || !w || !f || !g) return fail(name + ": null argument");
    const int32_t P = int32_t(t->probs.size());
    for (int32_t k = 0; k < P; ++k)
        if (active[k] && (!g[k] || (t->sets[size_t(t->probs[k].set)].K > 0 && !w[k])))
            return fail(name + ": null argument" + (lone ? "" : " for problem " + std::to_string(k)));
    Slot *slots = reinterpret_cast<Slot *>(t->h_in.data());
    ItemGroup *igs = reinterpret_cast<ItemGroup *>(t->h_in.data() + t->igs_off);
    double *wstate = reinterpret_cast<double *>(t->h_in.data() + t->ws_off);
    std::vector<Group> groups;
    int n_slots = 0, n_igs = 0;
    size_t in_hi = 0;
    int64_t out_lo = INT64_MAX, out_hi = 0, used = 0, items_bound = 0;
    // A group's item groups: its slots of one set, up to kTrainSetProbs at a time, in order of their first slot.
    auto close = [&](Group &gr) {
        std::vector<std::pair<int32_t, int>> last;  // set -> its latest item group
        for (int si = gr.s0; si < gr.s1; ++si) {
            const int32_t set = slots[si].set;
            int gi = -1;
            for (const auto &e : last)
                if (e.first == set) gi = e.second;
            if (gi < 0 || igs[gi].n == kTrainSetProbs) {
                gi = n_igs++;
                igs[gi].set = set;
                igs[gi].n = 0;
                igs[gi].blk = int32_t(gr.blk_items);
                gr.blk_items += blocks_of(t->sets[size_t(set)].n_items, kTrainThreads);
                bool found = false;
                for (auto &e : last)
                    if (e.first == set) e.second = gi, found = true;
                if (!found) last.emplace_back(set, gi);
            }
            igs[gi].slot[igs[gi].n++] = si - gr.s0;
            gr.np = std::max(gr.np, igs[gi].n);
        }
        gr.g1 = n_igs;
        groups.push_back(gr);
    };
    Group cur{};
    bool open = false;
    for (int32_t k = 0; k < P; ++k) {
        if (!active[k]) continue;
        const Trainer::Prob &p = t->probs[k];
        const Trainer::Set &S = t->sets[size_t(p.set)];
        if (S.n_win == 0) continue;
        const int64_t nb_items = blocks_of(S.n_items, kTrainThreads), nb_win = blocks_of(S.n_win, kTrainWinThreads);
        if (open && (used + p.scratch > t->scratch_cap || items_bound + nb_items > INT32_MAX ||
                     cur.blk_win + nb_win > INT32_MAX || cur.blk_attr + S.A > INT32_MAX)) {
            close(cur);
            open = false;
        }
        if (!open) {
            cur = Group{n_slots, n_slots, n_igs, n_igs, 0, 0, 0, 0, 1};
            used = items_bound = 0;
            open = true;
        }
        double *ws = wstate + p.ws0;
        for (size_t j = 0; j < S.state_fid.size(); ++j) ws[j] = S.state_fid[j] >= 0 ? w[k][S.state_fid[j]] : 0.0;
        in_hi = std::max(in_hi, t->ws_off + size_t(p.ws0 + 2 * int64_t(S.A)) * sizeof(double));
        Slot &s = slots[n_slots++];
        s.T = trans_args(S.trans_fid, w[k]);
        s.ws0 = p.ws0;
        s.sc0 = used;
        s.out0 = p.out0;
        s.set = p.set;
        s.blk[kGridWindows] = int32_t(cur.blk_win);
        s.blk[kGridAttrs] = int32_t(cur.blk_attr);
        cur.s1 = n_slots;
        cur.blk_win += nb_win;
        cur.blk_attr += S.A;
        cur.lds_w = std::max(cur.lds_w, S.W);
        used += p.scratch;
        items_bound += nb_items;
        out_lo = std::min(out_lo, p.out0);
        out_hi = std::max(out_hi, p.out0 + kTrainRowCols + 2 * int64_t(S.A));
    }
    if (open) close(cur);

    int rc = set_device(t->device);
    if (rc) return rc;
    hipStream_t st = t->stream.get();
    if (!groups.empty()) {
        const double *d_wstate = reinterpret_cast<const double *>(t->d_in.get() + t->ws_off);
        if ((rc = check_hip(hipMemcpyAsync(t->d_in.get(), t->h_in.data(), in_hi, hipMemcpyHostToDevice, st), "trainer weights upload")))
            return rc;
        // groups run one after another on the stream and share the work space
        for (const Group &gr : groups) {
            const Slot *d_slots = reinterpret_cast<const Slot *>(t->d_in.get()) + gr.s0;
            const ItemGroup *d_igs = reinterpret_cast<const ItemGroup *>(t->d_in.get() + t->igs_off) + gr.g0;
            const int ns = gr.s1 - gr.s0, ng = gr.g1 - gr.g0;
            if (gr.np <= 1) launch_item_scores<1>(gr, d_igs, d_slots, t, d_wstate, st);
            else if (gr.np <= 2) launch_item_scores<2>(gr, d_igs, d_slots, t, d_wstate, st);
            else if (gr.np <= 4) launch_item_scores<4>(gr, d_igs, d_slots, t, d_wstate, st);
            else launch_item_scores<kTrainSetProbs>(gr, d_igs, d_slots, t, d_wstate, st);
            const size_t lds = size_t(gr.lds_w) * kTrainWinThreads * 3 * sizeof(double);
            train_windows<<<dim3(unsigned(gr.blk_win)), kTrainWinThreads, lds, st>>>(d_slots, ns, t->d_sets.get(), t->d_label.get(),
                                                                                   t->d_win_start.get(), gr.lds_w, t->d_scratch.get());
            train_item_marginals<<<dim3(unsigned(gr.blk_items)), kTrainThreads, 0, st>>>(
                d_igs, ng, d_slots, t->d_sets.get(), t->d_iw_first.get(), t->d_iw_cnt.get(), t->d_iw_off.get(), t->d_scratch.get());
            train_attr_counts<<<dim3(unsigned(gr.blk_attr)), kTrainThreads, 0, st>>>(d_slots, ns, t->d_sets.get(), t->d_attr_ptr.get(),
                                                                                    t->d_attr_items.get(), t->d_scratch.get(), t->d_out.get());
            train_reduce_rows<<<ns * kTrainReduceBlocks, kTrainThreads, 0, st>>>(d_slots, t->d_sets.get(), t->d_scratch.get(),
                                                                                 t->d_partial.get());
            train_reduce_final<<<ns, kTrainReduceBlocks, 0, st>>>(d_slots, t->d_partial.get(), t->d_out.get());
        }
        if ((rc = check_hip(hipGetLastError(), "trainer kernels"))) return rc;
        if ((rc = check_hip(hipMemcpyAsync(t->h_out.data() + out_lo, t->d_out.get() + out_lo,
                                           size_t(out_hi - out_lo) * sizeof(double), hipMemcpyDeviceToHost, st),
                            "trainer download")))
            return rc;
        if ((rc = check_hip(hipStreamSynchronize(st), "trainer synchronize"))) return rc;
    }
    std::vector<double> zeros;
    for (int32_t k = 0; k < P; ++k) {
        if (!active[k]) continue;
        const Trainer::Set &p = t->sets[size_t(t->probs[k].set)];
        const double *o = t->h_out.data() + t->probs[k].out0;  // row sums, then expected state counts
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

int32_t trainer_num_problems(const Trainer *t) { return t ? int32_t(t->probs.size()) : -1; }

int64_t trainer_num_windows(const Trainer *t, int32_t k) {
    return (t && k >= 0 && k < int32_t(t->probs.size())) ? t->sets[size_t(t->probs[k].set)].n_win : -1;
}

int64_t trainer_scratch_bytes(const Trainer *t, int32_t k) {
    if (!t || k < -1 || k >= int32_t(t->probs.size())) return -1;
    return k < 0 ? t->scratch_cap : t->probs[k].scratch;
}

void trainer_destroy(Trainer *t) { delete t; }

}  // namespace gecco
