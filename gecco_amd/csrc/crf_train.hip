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

__global__ void __launch_bounds__(kTrainThreads) train_item_scores(const int32_t *__restrict__ item_ptr,
                                                                   const int32_t *__restrict__ attr_id,
                                                                   const double *__restrict__ wstate, int32_t n_items,
                                                                   double2 *__restrict__ score) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    double s0 = 0.0, s1 = 0.0;
    for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
        const int32_t a = attr_id[k];
        s0 += wstate[2 * a];
        s1 += wstate[2 * a + 1];
    }
    score[i] = make_double2(s0, s1);
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
__global__ void __launch_bounds__(kTrainWinThreads) __attribute__((amdgpu_waves_per_eu(6)))
train_windows(const double2 *__restrict__ score, const int32_t *__restrict__ label, const int32_t *__restrict__ win_start,
              int64_t n_win, int32_t W, const TransArgs T, double2 *__restrict__ marg, double *__restrict__ rows) {
    extern __shared__ double lds[];
    double2 *alpha = reinterpret_cast<double2 *>(lds);                 // [W][kTrainWinThreads]
    double *cnorm = lds + 2 * static_cast<size_t>(W) * kTrainWinThreads;  // [W][kTrainWinThreads]
    const int lane = threadIdx.x;
    const int64_t w = static_cast<int64_t>(blockIdx.x) * kTrainWinThreads + lane;
    if (w >= n_win) return;
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
__global__ void __launch_bounds__(kTrainThreads) train_item_marginals(const double2 *__restrict__ marg,
                                                                      const int32_t *__restrict__ iw_first,
                                                                      const int32_t *__restrict__ iw_cnt,
                                                                      const int32_t *__restrict__ iw_off, int32_t n_items,
                                                                      int32_t W, int32_t step,
                                                                      double2 *__restrict__ item_marg) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const int64_t first = iw_first[i];
    const int32_t cnt = iw_cnt[i];
    int32_t off = iw_off[i];
    double p0 = 0.0, p1 = 0.0;
    for (int32_t k = 0; k < cnt; ++k, off -= step) {
        const double2 v = marg[(first + k) * W + off];
        p0 += v.x;
        p1 += v.y;
    }
    item_marg[i] = make_double2(p0, p1);
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
__global__ void __launch_bounds__(kTrainThreads) train_attr_counts(const int32_t *__restrict__ attr_ptr,
                                                                   const int32_t *__restrict__ attr_items,
                                                                   const double2 *__restrict__ item_marg, int32_t A,
                                                                   double *__restrict__ expected) {
    __shared__ double2 sh[kTrainThreads];
    const int32_t a = blockIdx.x;
    if (a >= A) return;
    double2 acc = make_double2(0.0, 0.0);
    for (int32_t k = attr_ptr[a] + threadIdx.x; k < attr_ptr[a + 1]; k += kTrainThreads) {
        const double2 v = item_marg[attr_items[k]];
        acc.x += v.x;
        acc.y += v.y;
    }
    const double2 tot = block_sum2<kTrainThreads>(acc, sh);
    if (threadIdx.x == 0) {
        expected[2 * a] = tot.x;
        expected[2 * a + 1] = tot.y;
    }
}

// Row sums, stage 1: slab b = rows [b * chunk, (b + 1) * chunk), chunk = ceil(n / kTrainReduceBlocks).
__global__ void __launch_bounds__(kTrainThreads) train_reduce_rows(const double *__restrict__ rows, int64_t n,
                                                                   double *__restrict__ partial) {
    __shared__ double sh[kTrainRowCols][kTrainThreads];
    const int64_t chunk = (n + kTrainReduceBlocks - 1) / kTrainReduceBlocks;
    const int64_t lo = blockIdx.x * chunk, hi = std::min(n, lo + chunk);
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
    if (threadIdx.x < kTrainRowCols) partial[blockIdx.x * kTrainRowCols + threadIdx.x] = sh[threadIdx.x][0];
}

// Stage 2: one workgroup, thread j holds slab j, then a tree.
__global__ void __launch_bounds__(kTrainReduceBlocks) train_reduce_final(const double *__restrict__ partial,
                                                                         double *__restrict__ out) {
    __shared__ double sh[kTrainRowCols][kTrainReduceBlocks];
    for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] = partial[threadIdx.x * kTrainRowCols + k];
    __syncthreads();
    for (int h = kTrainReduceBlocks / 2; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h)
            for (int k = 0; k < kTrainRowCols; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < kTrainRowCols) out[threadIdx.x] = sh[threadIdx.x][0];
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

}  // namespace

struct Trainer {
    int device = 0;
    int32_t A = 0, W = 0, step = 1, n_items = 0, K = 0;
    int64_t n_win = 0;
    std::vector<int32_t> state_fid, trans_fid;  // [A*2], [4]: feature id of every dense slot, or -1
    std::vector<double> empirical;              // [K] observed feature counts over all windows
    std::vector<double> h_wstate, h_expected;   // [A*2] host staging
    hipStream_t stream = nullptr;
    // device: training set (uploaded once) and per-evaluation work space
    int32_t *d_item_ptr = nullptr, *d_attr_id = nullptr, *d_label = nullptr, *d_win_start = nullptr;
    int32_t *d_iw_first = nullptr, *d_iw_cnt = nullptr, *d_iw_off = nullptr;
    int32_t *d_attr_ptr = nullptr, *d_attr_items = nullptr;
    double *d_wstate = nullptr, *d_expected = nullptr, *d_rows = nullptr, *d_partial = nullptr, *d_sums = nullptr;
    double2 *d_score = nullptr, *d_marg = nullptr, *d_item_marg = nullptr;

    ~Trainer() {
        int prev = -1;
        const bool restore = hipGetDevice(&prev) == hipSuccess && prev != device;
        (void)hipSetDevice(device);
        for (void *p : {(void *)d_item_ptr, (void *)d_attr_id, (void *)d_label, (void *)d_win_start, (void *)d_iw_first,
                        (void *)d_iw_cnt, (void *)d_iw_off, (void *)d_attr_ptr, (void *)d_attr_items, (void *)d_wstate,
                        (void *)d_expected, (void *)d_rows, (void *)d_partial, (void *)d_sums, (void *)d_score,
                        (void *)d_marg, (void *)d_item_marg})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (restore && prev >= 0) (void)hipSetDevice(prev);
    }
};

int trainer_create(int32_t device, const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr, const int32_t *attr_id,
                   const int32_t *labels, int32_t num_attrs, int32_t num_labels, int32_t window, int32_t step,
                   const int32_t *state_fid, const int32_t *trans_fid, int32_t num_features, Trainer **out) {
    if (!out || !seq_ptr || n_seqs < 0 || !state_fid || !trans_fid) return fail("trainer: null argument");
    *out = nullptr;
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return GECCO_CRF_ENODEV;
    }
    if (device < 0 || device >= ndev) {
        set_error("device index out of range");
        return GECCO_CRF_ENODEV;
    }

    auto t = std::make_unique<Trainer>();
    t->device = device;
    t->A = num_attrs;
    t->W = window;
    t->step = step;
    t->n_items = n_items;
    t->K = num_features;
    t->state_fid.assign(state_fid, state_fid + int64_t(num_attrs) * 2);
    t->trans_fid.assign(trans_fid, trans_fid + 4);
    t->h_wstate.assign(size_t(num_attrs) * 2, 0.0);
    t->h_expected.assign(size_t(num_attrs) * 2, 0.0);

    // windows (gecco/_meta.py sliding_window, no padding) and, per item, the windows covering it
    std::vector<int32_t> win_start, iw_first(n_items, 0), iw_cnt(n_items, 0), iw_off(n_items, 0);
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
    t->n_win = int64_t(win_start.size());

    // empirical counts, exact (integers in doubles): state (a, y_i) once per window covering item i, transitions per window
    t->empirical.assign(size_t(num_features), 0.0);
    for (int32_t i = 0; i < n_items; ++i)
        for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) {
            const int32_t fid = t->state_fid[size_t(attr_id[k]) * 2 + labels[i]];
            if (fid >= 0) t->empirical[fid] += iw_cnt[i];
        }
    for (int32_t i0 : win_start)
        for (int32_t j = 1; j < window; ++j) {
            const int32_t fid = t->trans_fid[labels[i0 + j - 1] * 2 + labels[i0 + j]];
            if (fid >= 0) t->empirical[fid] += 1.0;
        }

    // attribute -> items transpose (items ascending within every attribute)
    std::vector<int32_t> attr_ptr(size_t(num_attrs) + 1, 0), attr_items(static_cast<size_t>(nnz));
    for (int32_t k = 0; k < nnz; ++k) ++attr_ptr[attr_id[k] + 1];
    for (int32_t a = 0; a < num_attrs; ++a) attr_ptr[a + 1] += attr_ptr[a];
    {
        std::vector<int32_t> fill(attr_ptr.begin(), attr_ptr.end() - 1);
        for (int32_t i = 0; i < n_items; ++i)
            for (int32_t k = item_ptr[i]; k < item_ptr[i + 1]; ++k) attr_items[fill[attr_id[k]]++] = i;
    }

    int rc = check_hip(hipSetDevice(device), "hipSetDevice");
    if (rc) return rc;
    if ((rc = check_hip(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking), "hipStreamCreate"))) return rc;
    std::vector<int32_t> h_item_ptr(1, 0), h_attr, h_label;
    if (n_items > 0) {
        h_item_ptr.assign(item_ptr, item_ptr + n_items + 1);
        h_attr.assign(attr_id, attr_id + nnz);
        h_label.assign(labels, labels + n_items);
    }
    if ((rc = dev_upload(&t->d_item_ptr, h_item_ptr, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_id, h_attr, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_label, h_label, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_win_start, win_start, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_first, iw_first, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_cnt, iw_cnt, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_iw_off, iw_off, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_ptr, attr_ptr, "trainer upload"))) return rc;
    if ((rc = dev_upload(&t->d_attr_items, attr_items, "trainer upload"))) return rc;
    if ((rc = dev_alloc(&t->d_wstate, size_t(num_attrs) * 2, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_expected, size_t(num_attrs) * 2, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_rows, size_t(t->n_win) * kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_partial, size_t(kTrainReduceBlocks) * kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_sums, kTrainRowCols, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_score, size_t(n_items), "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_marg, size_t(t->n_win) * window, "trainer alloc"))) return rc;
    if ((rc = dev_alloc(&t->d_item_marg, size_t(n_items), "trainer alloc"))) return rc;
    *out = t.release();
    return GECCO_CRF_OK;
}

int trainer_eval(Trainer *t, const double *w, double *f, double *g) {
    if (!t || !f || !g || (t->K > 0 && !w)) return fail("trainer_eval: null argument");
    for (size_t k = 0; k < t->state_fid.size(); ++k) t->h_wstate[k] = t->state_fid[k] >= 0 ? w[t->state_fid[k]] : 0.0;
    TransArgs T;
    double tw[4];
    for (int k = 0; k < 4; ++k) tw[k] = t->trans_fid[k] >= 0 ? w[t->trans_fid[k]] : 0.0;
    T.t00 = tw[0], T.t01 = tw[1], T.t10 = tw[2], T.t11 = tw[3];
    T.tmax = std::max(std::max(tw[0], tw[1]), std::max(tw[2], tw[3]));
    T.e00 = std::exp(tw[0] - T.tmax), T.e01 = std::exp(tw[1] - T.tmax);
    T.e10 = std::exp(tw[2] - T.tmax), T.e11 = std::exp(tw[3] - T.tmax);
    T.log_space = 0;
    for (double e : {T.e00, T.e01, T.e10, T.e11})
        if (!(e >= DBL_MIN && e <= DBL_MAX)) T.log_space = 1;

    int rc = check_hip(hipSetDevice(t->device), "hipSetDevice");
    if (rc) return rc;
    hipStream_t st = t->stream;
    const size_t A2 = size_t(t->A) * 2;
    if ((rc = check_hip(hipMemcpyAsync(t->d_wstate, t->h_wstate.data(), A2 * sizeof(double), hipMemcpyHostToDevice, st),
                        "trainer weights upload")))
        return rc;
    double sums[kTrainRowCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (t->n_win > 0) {
        const int32_t nb_items = (t->n_items + kTrainThreads - 1) / kTrainThreads;
        train_item_scores<<<nb_items, kTrainThreads, 0, st>>>(t->d_item_ptr, t->d_attr_id, t->d_wstate, t->n_items, t->d_score);
        const int64_t nb_win = (t->n_win + kTrainWinThreads - 1) / kTrainWinThreads;
        const size_t lds = size_t(t->W) * kTrainWinThreads * 3 * sizeof(double);
        train_windows<<<dim3(unsigned(nb_win)), kTrainWinThreads, lds, st>>>(t->d_score, t->d_label, t->d_win_start, t->n_win,
                                                                            t->W, T, t->d_marg, t->d_rows);
        train_item_marginals<<<nb_items, kTrainThreads, 0, st>>>(t->d_marg, t->d_iw_first, t->d_iw_cnt, t->d_iw_off,
                                                                 t->n_items, t->W, t->step, t->d_item_marg);
        train_attr_counts<<<t->A, kTrainThreads, 0, st>>>(t->d_attr_ptr, t->d_attr_items, t->d_item_marg, t->A, t->d_expected);
        train_reduce_rows<<<kTrainReduceBlocks, kTrainThreads, 0, st>>>(t->d_rows, t->n_win, t->d_partial);
        train_reduce_final<<<1, kTrainReduceBlocks, 0, st>>>(t->d_partial, t->d_sums);
        if ((rc = check_hip(hipGetLastError(), "trainer kernels"))) return rc;
        if ((rc = check_hip(hipMemcpyAsync(t->h_expected.data(), t->d_expected, A2 * sizeof(double), hipMemcpyDeviceToHost, st),
                            "trainer download")))
            return rc;
        if ((rc = check_hip(hipMemcpyAsync(sums, t->d_sums, sizeof(sums), hipMemcpyDeviceToHost, st), "trainer download")))
            return rc;
    } else {
        std::fill(t->h_expected.begin(), t->h_expected.end(), 0.0);
    }
    if ((rc = check_hip(hipStreamSynchronize(st), "trainer synchronize"))) return rc;
    *f = sums[0];
    for (int32_t k = 0; k < t->K; ++k) g[k] = -t->empirical[k];
    for (size_t k = 0; k < A2; ++k)
        if (t->state_fid[k] >= 0) g[t->state_fid[k]] += t->h_expected[k];
    for (int k = 0; k < 4; ++k)
        if (t->trans_fid[k] >= 0) g[t->trans_fid[k]] += sums[1 + k];
    return GECCO_CRF_OK;
}

int64_t trainer_num_windows(const Trainer *t) { return t ? t->n_win : -1; }

void trainer_destroy(Trainer *t) { delete t; }

}  // namespace gecco
