// Training objective and gradient of a linear-chain CRF with 2 to 32 labels (gecco_crf_trainer_general_*; DESIGN.md
// §4.9b).  The objective is crf_train.hip's:
//     f(w) = sum over windows of (log Z(window) - score(gold labels of the window))
//     g(w) = expected feature counts - empirical feature counts
// over the sliding windows of every sequence, without the regularisation terms.
//
// Every problem has its own label count L, window W and step, and runs its own launches on the trainer's stream (no
// kernel ever sees two problems, so a problem's bits cannot depend on its neighbours):
//   1. item scores     one thread per (item, label): s[i][y] = sum of the state weights of its attributes (CSR order)
//   2. instances       G = the power of two at or above L lanes per window, lane i owning label i; log-space
//                      forward-backward.  log alpha_t is stored in the window's node-marginal slots and overwritten by
//                      the marginals on the way back.  A workgroup runs a fixed 128 windows, keeps the pairwise
//                      expectations xi[i][.] of all of them in registers, and writes one block (f, xi[L][L])
//   3. item marginals  one thread per (item, label): the node marginals of the windows covering it, in window order
//   4. attr counts     one workgroup per attribute: the item marginals over the attribute -> items transpose
//   5/6. block sums    fixed-geometry two-stage sum over the workgroups' blocks
// Log space throughout: right for any finite weights, no second path.  No float atomics: every sum has one fixed order.
//
// Kernel 2 is two kernels with two parameters each, which share what can be shared at no cost in time: the transition load
// and the workgroup sum are device functions templated on G that both call, the forward step is one that gen_partial calls
// for both of its passes.  The other steps stay in the kernels' bodies (see forward_lse below for what was measured):
//   gen_labelled<G, kWhole>  the labelled problems.  kWhole = false: the windows above.  kWhole = true: the whole-sequence
//                            family (gecco_crf_trainer_sequences_*), the same objective with one instance
//                            per sequence, of that sequence's own length.  Every item then lies in exactly one instance, so
//                            the kernel writes its node marginals straight into the item marginals and kernel 3 does not run.
//   gen_partial<G, kWhole>   partially labelled problems (gecco_crf_trainer_{general, sequences}_create_partial; DESIGN.md
//                            §4.9e), which carry a mask of allowed labels per item and minimise log Z - log Z_A: the free and
//                            the restricted recursion in the same slot; it hands on their difference.
// Each has a third parameter, kWeighted (the *_create_weighted problems with sequence weights or a label-cost matrix; DESIGN.md
// §4.9q): the weighted instantiation hands on its sums already weighted.
// Every other kernel is shared by all of them as it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_model.hpp"
#include "crf_plan.hpp"
#include "crf_train.hpp"
#include "crf_train_host.hpp"

namespace gecco {

namespace {

constexpr int kTrainGenThreads = 256;          // threads per workgroup of every kernel
constexpr int kTrainGenWindowsPerBlock = 128;  // windows per workgroup of the window kernel, whatever L is
constexpr int kTrainGenReduceSlabs = 32;       // first stage of the block sums: a fixed number of slabs
constexpr int kTrainGenMaxL = 32;

// One problem as its kernels take it (by value).  The set arrays are the problem's own slices.
struct GenProb {
    const int32_t *item_ptr, *attr_id, *label, *win_start, *iw_first, *iw_cnt, *iw_off, *attr_ptr, *attr_items;
    const int32_t *win_len;  // whole sequences: the items of instance q, which starts at win_start[q]; else not read
    const double *wstate;  // [A][L] state weights of this evaluation
    const double *trans;   // [L][L] transition weights
    double *score;         // [n_items][L]
    double *item_marg;     // [n_items][L]
    double *marg;          // [n_win][W][L]: log alpha on the way forward, node marginals afterwards
    double *partial;       // [n_blocks][1 + L*L]: per workgroup of the window (or sequence) kernel, f then xi
    double *slab;          // [kTrainGenReduceSlabs][1 + L*L]
    double *out;           // [1 + L*L + A*L]: f, xi, expected state counts
    int64_t n_win;
    int32_t n_items, A, L, W, step, n_blocks;
};

// kValued (the *_create_valued problems that carry values): s[i][y] = sum of v * w over the item's attributes,
// attr_value parallel to attr_id, every term added as fma(v, w, acc) in CSR order.  That is the one multiply-add form of every
// valued kernel (gl_state and gen_attr_counts too): fma(1, w, acc) rounds acc + w once, so a problem whose values are all 1.0
// has the unvalued problem's bits.  The unvalued instantiation is the kernel as it was (attr_value, last, is not read there).
template <bool kValued>
__global__ void __launch_bounds__(kTrainGenThreads) gen_item_scores(GenProb P, const double *attr_value) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kTrainGenThreads + threadIdx.x;
    if (idx >= static_cast<int64_t>(P.n_items) * P.L) return;
    const int32_t i = static_cast<int32_t>(idx / P.L), y = static_cast<int32_t>(idx % P.L);
    double s = 0.0;
    for (int32_t k = P.item_ptr[i]; k < P.item_ptr[i + 1]; ++k) {
        if constexpr (kValued)
            s = fma(attr_value[k], P.wstate[static_cast<int64_t>(P.attr_id[k]) * P.L + y], s);
        else
            s += P.wstate[static_cast<int64_t>(P.attr_id[k]) * P.L + y];
    }
    P.score[idx] = s;
}

// The instance kernels.  G lanes per instance (G a power of two, L <= G), lane i owning label i; 256 / G instances run side by
// side, one per slot.  Everything is in log space:
//     forward   la_t[j] = s_t[j] + lse_i(la_{t-1}[i] + T[i][j])
//     backward  lb_{t-1}[i] = lse_j(T[i][j] + s_t[j] + lb_t[j]),   marginal_t[i] = exp(la_t[i] + lb_t[i] - log Z)
//     pairwise  xi_t[i][j] = marginal_{t-1}[i] * e_ij / sum_j e_ij,   e_ij = exp(T[i][j] + s_t[j] + lb_t[j] - max_j),
// so the pairwise term reuses the exponentials of the backward step (e_ij <= 1 and their sum >= 1: nothing overflows, and
// what underflows is below 1e-308 of a probability).  A lane reads its neighbours' values by shuffles inside its group
// of G lanes and the transitions from LDS (both orientations, so that either read is conflict-free).  Lanes at or above
// L compute on zeros and store nothing.  xi[i][.] accumulates in the registers of lane i over the positions and instances
// of its slot, in that order; the slots of a wave are then summed by a butterfly, the four waves in wave order.
// The instances of a wave may differ in length, so none of the steps below that run inside a loop over t has a workgroup
// barrier or a shuffle that leaves the group's own G lanes (all of which run the same trip count).

// The transitions into LDS: tT[i][j] = T[i][j], tTt[j][i] = T[i][j], zero at or above L.  Ends with the workgroup's barrier.
template <int G>
__device__ __forceinline__ void load_transitions(const double *trans, int L, double *tT, double *tTt) {
    for (int e = threadIdx.x; e < G * G; e += kTrainGenThreads) {
        const int a = e / G, b = e % G;
        const double v = (a < L && b < L) ? trans[a * L + b] : 0.0;
        tT[e] = v;
        tTt[b * G + a] = v;
    }
    __syncthreads();
}

// The forward step: lse over k < L of log alpha_{t-1}[k] (x of the group's lane k) + T[k][i], on the kernel's one array v.
// gen_partial calls it for both passes.  It is the only step of the recursion that is a function, by measurement on an
// MI355X (profiles/train_general_layouts.txt): gen_labelled with this step, or with the backward step, as a function ran 32
// labels on whole sequences 4 to 5 % slower than with both in its body; gen_partial with the backward step as a function
// ran windows at 2 labels 10 % slower, and with the log partition as one called twice windows at 32 labels 2 % slower.  The
// arithmetic is the same every time; what moves is the compiler's schedule and register allocation around the inlined
// code.  So a change to the recursion is made in gen_labelled's body, in gen_partial's (twice) and, for this step, here.
template <int G>
__device__ __forceinline__ double forward_lse(double x, const double *tT, int i, int L, double (&v)[G]) {
    double mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < G; ++k)
        if (k < L) {
            v[k] = __shfl(x, k, G) + tT[k * G + i];
            mx = fmax(mx, v[k]);
        }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k)
        if (k < L) sum += exp(v[k] - mx);
    return mx + log(sum);
}

// The workgroup's block (f, xi[L][L]) from every lane's sums, after every group has left its loops: the slots of a wave by a
// butterfly over the lanes that own the same label (both partners form the same sum), then the waves in wave order.
template <int G>
__device__ __forceinline__ void write_block(double (&xacc)[G], double facc, int L, double *xi_sh, double *f_sh, double *part) {
    const int tid = threadIdx.x;
    for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
        for (int k = 0; k < G; ++k) xacc[k] += __shfl_xor(xacc[k], off);
        facc += __shfl_xor(facc, off);
    }
    const int wave = tid / 64, lane = tid % 64;
    for (int wv = 0; wv < kTrainGenThreads / 64; ++wv) {
        if (wave == wv && lane < G) {
#pragma unroll
            for (int k = 0; k < G; ++k) xi_sh[k * G + lane] = (wv ? xi_sh[k * G + lane] : 0.0) + xacc[k];
            if (lane == 0) *f_sh = (wv ? *f_sh : 0.0) + facc;
        }
        __syncthreads();
    }
    for (int e = tid; e < G * G; e += kTrainGenThreads) {
        const int k = e / G, a = e % G;
        if (a < L && k < L) part[1 + a * L + k] = xi_sh[e];
    }
    if (tid == 0) part[0] = *f_sh;
}

// The labelled problems.  kWhole = false, windows: a workgroup runs its kTrainGenWindowsPerBlock windows, all of P.W items, in
// rounds of 256 / G, and the node marginals go to the window's own slots of P.marg.  kWhole = true, whole sequences: the
// instance's own length, and the node marginals go straight into item_marg (log alpha on the way forward, the marginal on the
// way back).  A workgroup then owns the 256 / G sequences it runs side by side, one per slot, so that an evaluation is as close
// to its bound, the longest sequence, as the sequence count allows: instance q of the problem's slot order (longest first, ties
// by index: computed on the host from the problem alone) runs in workgroup q / kSlots, slot q % kSlots, and the groups running
// side by side have neighbouring lengths.
// The windows index their scores and marginals with int, as their kernel always has (t * L + i < W * L <= 32 * window, and a
// 64-bit index costs the two-label group a wave per SIMD); a sequence has no such bound and indexes with int64_t.
//
// kWeighted (the *_create_weighted problems that carry sequence weights or a label-cost matrix): the instance's
// term of the objective is omega * (log Z_C - score(gold)), omega = inst_weight[w] the weight of the sequence it was cut from and
// Z_C the partition function of the lattice whose state scores are s_t[i] + C[gold_t][i].  C[gold][.] lies in LDS beside the
// transitions, [G][G] with zeros at or above L, and is added wherever the recursion reads a state score: the first item, the
// forward step and the backward step's q.  Its diagonal is exactly 0, so the gold path's score needs nothing.  omega multiplies
// what the instance hands on and nothing it keeps: its term of f, every node marginal at the store on the way back (never the
// log alpha the slot holds on the way forward) and, through the marginal m, the pairwise expectations.  cost == nullptr: weights
// only, a table of zeros.  inst_weight holds one weight per instance in the order of win_start, so a sequence's weight follows it
// through the slot order.  The unweighted instantiation reads neither argument and is the kernel as it was.
template <int G, bool kWhole, bool kWeighted>
__global__ void __launch_bounds__(kTrainGenThreads) gen_labelled(GenProb P, const double *inst_weight, const double *cost) {
    using Idx = std::conditional_t<kWhole, int64_t, int>;
    constexpr int kSlots = kTrainGenThreads / G;
    constexpr int kPerBlock = kWhole ? kSlots : kTrainGenWindowsPerBlock;
    __shared__ double tT[G * G];             // [i][j] = T[i][j]
    __shared__ double tTt[G * G];            // [j][i] = T[i][j]
    __shared__ double xi_sh[G * G];          // [j][i]
    __shared__ double f_sh;
    __shared__ double tC[kWeighted ? G * G : 1];  // [y][i] = C[y][i]: what predicting i costs at an item whose gold label is y
    const int tid = threadIdx.x;
    const int L = P.L;
    const int i = tid % G, slot = tid / G;
    const bool lab = i < L;
    if constexpr (kWeighted)  // (load_transitions ends with the barrier that covers these stores too)
        for (int e = tid; e < G * G; e += kTrainGenThreads) tC[e] = (cost && e / G < L && e % G < L) ? cost[(e / G) * L + e % G] : 0.0;
    load_transitions<G>(P.trans, L, tT, tTt);

    double xacc[G];
#pragma unroll
    for (int k = 0; k < G; ++k) xacc[k] = 0.0;
    double facc = 0.0;
    double v[G];
    const int64_t w_base = static_cast<int64_t>(blockIdx.x) * kPerBlock;
    for (int r = 0; r < kPerBlock / kSlots; ++r) {
        const int64_t w = w_base + r * kSlots + slot;
        if (w >= P.n_win) continue;  // (a whole group of G lanes: the shuffles below stay inside the group)
        const int64_t i0 = P.win_start[w];
        const int n = kWhole ? P.win_len[w] : P.W;
        const double *sc = P.score + i0 * L;
        const int32_t *label = P.label + i0;
        double *mw = kWhole ? P.item_marg + i0 * L : P.marg + w * n * L;

        double om = 1.0;
        if constexpr (kWeighted) om = inst_weight[w];
        double la = lab ? sc[i] : 0.0;
        int yprev = label[0];
        if constexpr (kWeighted) la += tC[yprev * G + i];
        double gold = (lab && yprev == i) ? la : 0.0;  // this label's share of the gold path's score
        if (lab) mw[i] = la;
        for (int t = 1; t < n; ++t) {
            double mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = __shfl(la, k, G) + tT[k * G + i];
                    mx = fmax(mx, v[k]);
                }
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) sum += exp(v[k] - mx);
            const double s = kWeighted ? (lab ? sc[static_cast<Idx>(t) * L + i] : 0.0) + tC[label[t] * G + i]
                                       : (lab ? sc[static_cast<Idx>(t) * L + i] : 0.0);
            la = mx + log(sum) + s;
            const int y = label[t];
            if (lab && y == i) gold += s + tT[yprev * G + i];
            yprev = y;
            if (lab) mw[static_cast<Idx>(t) * L + i] = la;
        }
        double mx = -INFINITY, gold_all = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < L) {
                v[k] = __shfl(la, k, G);
                mx = fmax(mx, v[k]);
                gold_all += __shfl(gold, k, G);
            }
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < L) sum += exp(v[k] - mx);
        const double logz = mx + log(sum);
        if constexpr (kWeighted) {
            if (i == 0) facc += om * (logz - gold_all);
            if (lab) mw[static_cast<Idx>(n - 1) * L + i] = om * exp(la - logz);
        } else {
            if (i == 0) facc += logz - gold_all;

            if (lab) mw[static_cast<Idx>(n - 1) * L + i] = exp(la - logz);
        }
        double lb = 0.0;
        for (int t = n - 1; t >= 1; --t) {
            // log of exp(s_t[i]) beta_t[i]
            const double q = kWeighted ? (lab ? sc[static_cast<Idx>(t) * L + i] : 0.0) + tC[label[t] * G + i] + lb
                                       : (lab ? sc[static_cast<Idx>(t) * L + i] : 0.0) + lb;
            const double lap = lab ? mw[static_cast<Idx>(t - 1) * L + i] : 0.0;  // log alpha_{t-1}[i], stored by this lane
            mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = tTt[k * G + i] + __shfl(q, k, G);
                    mx = fmax(mx, v[k]);
                }
            sum = 0.0;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = exp(v[k] - mx);
                    sum += v[k];
                }
            lb = mx + log(sum);
            const double m = kWeighted ? om * exp(lap + lb - logz) : exp(lap + lb - logz);
            const double c = m / sum;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) xacc[k] += c * v[k];
            if (lab) mw[static_cast<Idx>(t - 1) * L + i] = m;
        }
    }

    write_block<G>(xacc, facc, L, xi_sh, &f_sh, P.partial + static_cast<int64_t>(blockIdx.x) * (1 + L * L));
}

// Partially labelled problems (the *_create_partial problems that carry allowed-label sets): every item
// has a set of allowed labels, one uint32_t with bit y set when label y is allowed, and the objective is
//     f(w) = sum over instances of (log Z - log Z_A),   g(w) = E[feature counts] - E_A[feature counts],
// Z_A and E_A over the paths that stay inside the sets.  This is gen_labelled with a second, restricted recursion run beside
// the free one in the same slot, position by position: the same work decomposition, the same
// loops, and what the kernel hands on is the *difference* of the two passes (node marginals free - restricted in the slots
// the labelled kernels fill, xi free - restricted, f = log Z - log Z_A), so that the item-marginal, attribute-count and
// block-sum kernels run unchanged and the host's empirical vector is zero.
// A disallowed label is excluded, not penalised: its restricted log alpha is -inf, and so is what it offers to the backward
// step.  Every item has an allowed label (create refuses a mask of 0), so every maximum is taken over at least one finite
// term: the excluded terms are exp(-inf - finite) = 0 exactly and no -inf - (-inf) can form, however much of the free mass
// the excluded labels carry.  The restricted log alpha has its own storage, la_a, of the node marginals' shape
// ([n_win][W][L], whole sequences [n_items][L]).  Both families index with int64_t here.
// kWeighted: the instance's term is omega * (log Z - log Z_A), omega = inst_weight[w] as in gen_labelled: it multiplies the
// term of f, the difference of the node marginals at its store and both passes' marginals m and mr, and so the pairwise terms.
// There are no costs here: an item with a set of allowed labels has no single gold label to index C with.
template <int G, bool kWhole, bool kWeighted>
__global__ void __launch_bounds__(kTrainGenThreads) gen_partial(GenProb P, const uint32_t *allowed, double *la_a, const double *inst_weight) {
    constexpr int kSlots = kTrainGenThreads / G;  // instances side by side in a workgroup
    constexpr int kPerBlock = kWhole ? kSlots : kTrainGenWindowsPerBlock;
    __shared__ double tT[G * G];             // [i][j] = T[i][j]
    __shared__ double tTt[G * G];            // [j][i] = T[i][j]
    __shared__ double xi_sh[G * G];          // [j][i]
    __shared__ double f_sh;
    const int tid = threadIdx.x;
    const int L = P.L;
    const int i = tid % G, slot = tid / G;
    const bool lab = i < L;
    load_transitions<G>(P.trans, L, tT, tTt);

    double xacc[G];
#pragma unroll
    for (int k = 0; k < G; ++k) xacc[k] = 0.0;
    double facc = 0.0;
    double v[G];
    const int64_t w_base = static_cast<int64_t>(blockIdx.x) * kPerBlock;
    for (int r = 0; r < kPerBlock / kSlots; ++r) {
        const int64_t w = w_base + r * kSlots + slot;
        if (w >= P.n_win) continue;  // (a whole group of G lanes: the shuffles below stay inside the group)
        const int64_t i0 = P.win_start[w];
        const int n = kWhole ? P.win_len[w] : P.W;
        const double *sc = P.score + i0 * L;
        const uint32_t *al = allowed + i0;
        const int64_t m0 = kWhole ? i0 * L : w * n * L;
        double *mw = (kWhole ? P.item_marg : P.marg) + m0;  // free log alpha, then the difference of the marginals
        double *ma = la_a + m0;                              // restricted log alpha

        double om = 1.0;
        if constexpr (kWeighted) om = inst_weight[w];
        double la = lab ? sc[i] : 0.0;
        double lr = (lab && ((al[0] >> i) & 1u)) ? la : -INFINITY;
        if (lab) mw[i] = la, ma[i] = lr;
        for (int t = 1; t < n; ++t) {
            const double s = lab ? sc[static_cast<int64_t>(t) * L + i] : 0.0;
            const double lse = forward_lse<G>(la, tT, i, L, v);
            la = lse + s;
            const double lser = forward_lse<G>(lr, tT, i, L, v);
            lr = (lab && ((al[t] >> i) & 1u)) ? lser + s : -INFINITY;
            if (lab) mw[static_cast<int64_t>(t) * L + i] = la, ma[static_cast<int64_t>(t) * L + i] = lr;
        }
        double mx = -INFINITY, mxr = -INFINITY;
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < L) mx = fmax(mx, __shfl(la, k, G)), mxr = fmax(mxr, __shfl(lr, k, G));
        double sum = 0.0, sumr = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < L) sum += exp(__shfl(la, k, G) - mx), sumr += exp(__shfl(lr, k, G) - mxr);
        const double logz = mx + log(sum), logzr = mxr + log(sumr);
        if constexpr (kWeighted) {
            if (i == 0) facc += om * (logz - logzr);
            if (lab) mw[static_cast<int64_t>(n - 1) * L + i] = om * (exp(la - logz) - exp(lr - logzr));
        } else {
            if (i == 0) facc += logz - logzr;

            if (lab) mw[static_cast<int64_t>(n - 1) * L + i] = exp(la - logz) - exp(lr - logzr);
        }
        double lb = 0.0, lbr = 0.0;
        for (int t = n - 1; t >= 1; --t) {
            const double s = lab ? sc[static_cast<int64_t>(t) * L + i] : 0.0;
            const double q = s + lb;                                                // log of exp(s_t[i]) beta_t[i]
            const double qr = (lab && ((al[t] >> i) & 1u)) ? s + lbr : -INFINITY;  // the same, restricted
            const double lap = lab ? mw[static_cast<int64_t>(t - 1) * L + i] : 0.0;  // log alpha_{t-1}[i], stored by this lane
            const double lapr = lab ? ma[static_cast<int64_t>(t - 1) * L + i] : -INFINITY;
            mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = tTt[k * G + i] + __shfl(q, k, G);
                    mx = fmax(mx, v[k]);
                }
            sum = 0.0;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = exp(v[k] - mx);
                    sum += v[k];
                }
            lb = mx + log(sum);
            const double m = kWeighted ? om * exp(lap + lb - logz) : exp(lap + lb - logz);
            const double c = m / sum;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) xacc[k] += c * v[k];
            mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = tTt[k * G + i] + __shfl(qr, k, G);
                    mx = fmax(mx, v[k]);
                }
            sum = 0.0;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) {
                    v[k] = exp(v[k] - mx);
                    sum += v[k];
                }
            lbr = mx + log(sum);
            // (a label excluded at t - 1: exp(-inf) = 0)
            const double mr = kWeighted ? om * exp(lapr + lbr - logzr) : exp(lapr + lbr - logzr);
            const double cr = mr / sum;
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k < L) xacc[k] -= cr * v[k];
            if (lab) mw[static_cast<int64_t>(t - 1) * L + i] = m - mr;
        }
    }

    write_block<G>(xacc, facc, L, xi_sh, &f_sh, P.partial + static_cast<int64_t>(blockIdx.x) * (1 + L * L));
}

__global__ void __launch_bounds__(kTrainGenThreads) gen_item_marginals(GenProb P) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kTrainGenThreads + threadIdx.x;
    if (idx >= static_cast<int64_t>(P.n_items) * P.L) return;
    const int32_t i = static_cast<int32_t>(idx / P.L), y = static_cast<int32_t>(idx % P.L);
    const int64_t first = P.iw_first[i];
    const int32_t cnt = P.iw_cnt[i];
    int32_t off = P.iw_off[i];
    double p = 0.0;
    for (int32_t k = 0; k < cnt; ++k, off -= P.step) p += P.marg[((first + k) * P.W + off) * P.L + y];
    P.item_marg[idx] = p;
}

// Expected state counts: one workgroup per attribute, as 256 / G rows of G labels.  Row r sums the items r, r + rows, ...
// of the attribute's list, then the rows are summed by a tree.  kValued: every item's marginal times the value the attribute has
// on that item, attr_item_value parallel to attr_items (the transpose carries the value beside the item index), added as
// fma(v, marginal, acc) in the same order.
template <bool kValued>
__global__ void __launch_bounds__(kTrainGenThreads) gen_attr_counts(GenProb P, int32_t G, const double *attr_item_value) {
    __shared__ double sh[kTrainGenThreads];
    const int32_t a = static_cast<int32_t>(blockIdx.x);
    const int32_t y = threadIdx.x % G, r = threadIdx.x / G, rows = kTrainGenThreads / G;
    double acc = 0.0;
    if (y < P.L)
        for (int32_t k = P.attr_ptr[a] + r; k < P.attr_ptr[a + 1]; k += rows) {
            if constexpr (kValued)
                acc = fma(attr_item_value[k], P.item_marg[static_cast<int64_t>(P.attr_items[k]) * P.L + y], acc);
            else
                acc += P.item_marg[static_cast<int64_t>(P.attr_items[k]) * P.L + y];
        }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kTrainGenThreads / 2; h >= G; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (static_cast<int>(threadIdx.x) < P.L) P.out[1 + P.L * P.L + static_cast<int64_t>(a) * P.L + threadIdx.x] = sh[threadIdx.x];
}

// Block sums, stage 1: slab b = the window kernel's blocks [b * chunk, (b + 1) * chunk), chunk = ceil(n_blocks / slabs);
// a thread owns columns of the (f, xi) block and adds the slab's blocks in order.
__global__ void __launch_bounds__(kTrainGenThreads) gen_reduce_blocks(GenProb P) {
    const int cols = 1 + P.L * P.L;
    const int32_t chunk = (P.n_blocks + kTrainGenReduceSlabs - 1) / kTrainGenReduceSlabs;
    const int32_t lo = static_cast<int32_t>(blockIdx.x) * chunk, hi = min(P.n_blocks, lo + chunk);
    for (int e = threadIdx.x; e < cols; e += kTrainGenThreads) {
        double acc = 0.0;
        for (int32_t b = lo; b < hi; ++b) acc += P.partial[static_cast<int64_t>(b) * cols + e];
        P.slab[blockIdx.x * cols + e] = acc;
    }
}

// Stage 2: the slabs in order.
__global__ void __launch_bounds__(kTrainGenThreads) gen_reduce_final(GenProb P) {
    const int cols = 1 + P.L * P.L;
    for (int e = threadIdx.x; e < cols; e += kTrainGenThreads) {
        double acc = 0.0;
        for (int b = 0; b < kTrainGenReduceSlabs; ++b) acc += P.slab[b * cols + e];
        P.out[e] = acc;
    }
}

int group_of(int L) {
    int G = 2;
    while (G < L) G *= 2;
    return G;
}

// Calls fn with G (a group_of value) as a compile-time constant: fn(std::integral_constant<int, G>).
template <class F>
void with_group(int G, F &&fn) {
    switch (G) {
        case 2: fn(std::integral_constant<int, 2>{}); break;
        case 4: fn(std::integral_constant<int, 4>{}); break;
        case 8: fn(std::integral_constant<int, 8>{}); break;
        case 16: fn(std::integral_constant<int, 16>{}); break;
        default: fn(std::integral_constant<int, 32>{}); break;
    }
}

}  // namespace

// Problems resident on one device: every problem's arrays concatenated into one device array per kind, and one work
// space with every problem's scratch (so that the active problems of an evaluation run back to back on the stream).
struct TrainerGeneral {
    DeviceScope home{DeviceScope::kLater};  // (first member: see ~TrainerGeneral)
    int device = -1;  // set once the device has been checked
    bool whole = false;  // the whole-sequence family: every problem's instances are its sequences (W = step = 0)
    struct Prob {
        int32_t A, n_items, K, L, W, step, n_blocks;
        int64_t n_win;
        int64_t item0, iptr0, nnz0, win0, aptr0;  // the problem's slices of the set arrays
        int64_t in0, out0, sc0, scratch;          // weights in the upload, outputs in the download, scratch (doubles)
        // a problem with values: its slice of d_attr_value (parallel to attr_id); the values in transposed order (parallel to
        // attr_items) are the last nnz doubles of its scratch, written once by create.  val0 < 0: no values
        int64_t val0 = -1, nnz = 0;
        // a partially labelled problem: its slice of d_allowed (one mask per item), and the doubles of its second log alpha
        // array, which lies behind the slabs.  allow0 < 0: a labelled problem
        int64_t allow0 = -1, la_a = 0;
        // a weighted problem (sequence weights or label costs): one weight per instance at wt0 of its scratch, in the order of
        // win_start, and the cost matrix [L][L] at cost0 (cost0 < 0: weights only), both written once by create.  wt0 < 0: none
        int64_t wt0 = -1, cost0 = -1;
        std::vector<int32_t> state_fid, trans_fid;
        std::vector<double> empirical;
    };
    std::vector<Prob> probs;
    std::vector<double> h_in, h_out;
    Stream stream;
    DeviceBlock<int32_t> d_item_ptr, d_attr_id, d_label, d_win_start, d_win_len, d_iw_first, d_iw_cnt, d_iw_off, d_attr_ptr, d_attr_items;
    DeviceBlock<double> d_in, d_out, d_scratch, d_attr_value;
    DeviceBlock<uint32_t> d_allowed;

    // The members free themselves, in reverse order, after this body: with the trainer's device current, and `home` hands the
    // caller's device back at the end.  Refused before the device was checked (device < 0): nothing to free, and no HIP call.
    ~TrainerGeneral() { home.enter(device); }
};

namespace {

// Both families' create: window == nullptr is the whole-sequence family.  attr_value: null, or per problem the values of its
// attribute entries (entry k null: problem k has none, and runs the unvalued kernels).  allowed: null, or per problem one mask
// per item (entry k null: problem k is labelled, and runs the labelled kernels); labels[k] of a problem with masks is not read.
// seq_weight / label_cost: null, or per problem one weight per sequence / the cost matrix [L][L], row = gold (entry k null:
// weights of 1 / no costs); a problem with either runs the weighted kernels, a problem with neither is built as it always was.
int trainer_general_open(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                         const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                         const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                         const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                         const double *const *attr_value, const uint32_t *const *allowed, const double *const *seq_weight,
                         const double *const *label_cost, TrainerGeneral **out) {
    auto t = std::make_unique<TrainerGeneral>();
    const bool whole = t->whole = window == nullptr;
    const std::string family = whole ? "trainer sequences: problem " : "trainer general: problem ";
    std::vector<int32_t> item_ptr_c, attr_id_c, label_c, win_start_c, win_len_c, iw_first_c, iw_cnt_c, iw_off_c, attr_ptr_c,
        attr_items_c;
    std::vector<double> attr_value_c;
    std::vector<uint32_t> allowed_c;
    std::vector<std::vector<double>> transposed(static_cast<size_t>(n_problems));  // (attr_item_value of the valued problems)
    std::vector<std::vector<double>> weighting(static_cast<size_t>(n_problems));   // (instance weights, then costs, of the weighted)
    int64_t in_total = 0, out_total = 0, scratch_total = 0;
    for (int32_t k = 0; k < n_problems; ++k) {
        HostProblem hp;
        const uint32_t *masks = allowed ? allowed[k] : nullptr;
        const double *omega = seq_weight ? seq_weight[k] : nullptr, *cost = label_cost ? label_cost[k] : nullptr;
        if (omega && n_seqs[k] > 0)
            for (int32_t s = 0; s < n_seqs[k]; ++s)
                if (!(omega[s] >= 0.0) || std::isinf(omega[s]))
                    return fail(family + std::to_string(k) + ": weight of sequence " + std::to_string(s) +
                                " is negative or not finite (" + std::to_string(omega[s]) + ")");
        if (cost && num_labels[k] >= 2 && num_labels[k] <= kTrainGenMaxL) {
            const int32_t L = num_labels[k];
            if (masks)
                return fail(family + std::to_string(k) + ": label costs on a problem with allowed-label masks (no gold label to cost against)");
            for (int32_t e = 0; e < L * L; ++e) {
                const std::string at = "cost [" + std::to_string(e / L) + "][" + std::to_string(e % L) + "]";
                if (!(cost[e] >= 0.0) || std::isinf(cost[e]))
                    return fail(family + std::to_string(k) + ": " + at + " is negative or not finite (" + std::to_string(cost[e]) + ")");
                if (e / L == e % L && cost[e] != 0.0)
                    return fail(family + std::to_string(k) + ": " + at + " is on the diagonal and not 0 (" + std::to_string(cost[e]) + ")");
            }
        }
        // (a problem with masks has no gold path: build_problem gets label 0 on every item, and the counts it takes from them
        // are dropped below)
        std::vector<int32_t> no_labels;
        if (masks && seq_ptr[k] && n_seqs[k] >= 0) no_labels.assign(size_t(std::max(seq_ptr[k][n_seqs[k]], 1)), 0);
        int rc = build_problem(seq_ptr[k], n_seqs[k], item_ptr[k], attr_id[k], masks ? no_labels.data() : labels[k], num_attrs[k], num_labels[k],
                               whole ? 0 : window[k], whole ? 0 : step[k], state_fid[k], trans_fid[k], num_features[k],
                               kTrainGenMaxL, &hp, whole, attr_value ? attr_value[k] : nullptr, omega);
        if (rc) {
            set_error(family + std::to_string(k) + ": " + last_error());
            return rc;
        }
        if (masks) {
            const uint32_t beyond = num_labels[k] >= 32 ? 0u : ~0u << num_labels[k];  // the bits at or above L
            for (int32_t i = 0; i < hp.n_items; ++i) {
                if (masks[i] == 0)
                    return fail(family + std::to_string(k) + ": item " + std::to_string(i) + " allows no label (a mask of 0)");
                if (masks[i] & beyond)
                    return fail(family + std::to_string(k) + ": item " + std::to_string(i) + " allows a label at or above num_labels = " +
                                std::to_string(num_labels[k]) + " (mask " + std::to_string(masks[i]) + ")");
            }
            std::fill(hp.empirical.begin(), hp.empirical.end(), 0.0);  // both passes are expectations: nothing is observed
        }
        TrainerGeneral::Prob p;
        p.A = hp.A, p.n_items = hp.n_items, p.K = hp.K, p.L = num_labels[k];
        p.W = whole ? 0 : window[k], p.step = whole ? 0 : step[k];
        p.n_win = hp.n_win;
        const int64_t nb = blocks_of(hp.n_win, whole ? kTrainGenThreads / group_of(p.L) : kTrainGenWindowsPerBlock);
        const int64_t cols = 1 + int64_t(p.L) * p.L;
        if (nb > INT32_MAX || blocks_of(int64_t(p.n_items) * p.L, kTrainGenThreads) > INT32_MAX)
            return fail(family + std::to_string(k) + ": more than 2^31 workgroups in one launch");
        p.n_blocks = int32_t(nb);
        p.item0 = int64_t(label_c.size());
        p.iptr0 = int64_t(item_ptr_c.size());
        p.nnz0 = int64_t(attr_id_c.size());
        p.win0 = int64_t(win_start_c.size());
        p.aptr0 = int64_t(attr_ptr_c.size());
        p.in0 = in_total, p.out0 = out_total, p.sc0 = scratch_total;
        // scratch: item scores and item marginals [n_items][L], node marginals [n_win][W][L] (none for whole sequences:
        // W = 0), blocks and slabs of (f, xi); with masks, a second log alpha array; with values, one double per attribute entry
        // (the transposed values); a weighted problem, one double per instance and, with costs, L * L more
        p.scratch = 2 * int64_t(p.n_items) * p.L + hp.n_win * p.W * p.L + (nb + kTrainGenReduceSlabs) * cols;
        if (masks) {  // the restricted pass's log alpha, of the node marginals' shape
            p.allow0 = int64_t(allowed_c.size());
            p.la_a = whole ? int64_t(p.n_items) * p.L : hp.n_win * p.W * p.L;
            p.scratch += p.la_a;
            allowed_c.insert(allowed_c.end(), masks, masks + hp.n_items);
        }
        if (omega || cost) {  // a weighted problem: the instance weights (1 without sequence weights), then the costs
            p.wt0 = p.scratch;
            p.scratch += hp.n_win;
            std::vector<double> &up = weighting[size_t(k)];
            up = std::move(hp.inst_weight);
            if (!omega) up.assign(size_t(hp.n_win), 1.0);
            if (cost) {
                p.cost0 = p.scratch;
                p.scratch += int64_t(p.L) * p.L;
                up.insert(up.end(), cost, cost + int64_t(p.L) * p.L);
            }
        }
        if (attr_value && attr_value[k]) {  // a problem with values: the transposed values behind everything else
            p.val0 = int64_t(attr_value_c.size());
            p.nnz = int64_t(hp.attr_value.size());
            p.scratch += p.nnz;
            append(attr_value_c, hp.attr_value);
            transposed[size_t(k)] = std::move(hp.attr_item_value);
        }
        in_total += int64_t(p.A) * p.L + int64_t(p.L) * p.L;
        out_total += cols + int64_t(p.A) * p.L;
        scratch_total += p.scratch;
        append(item_ptr_c, hp.item_ptr);
        append(attr_id_c, hp.attr_id);
        append(label_c, hp.label);
        append(win_start_c, hp.win_start);
        append(win_len_c, hp.win_len);
        if (!whole) {  // (the coverage of an item: only the windowed family's kernel 3 reads it)
            append(iw_first_c, hp.iw_first);
            append(iw_cnt_c, hp.iw_cnt);
            append(iw_off_c, hp.iw_off);
        }
        append(attr_ptr_c, hp.attr_ptr);
        append(attr_items_c, hp.attr_items);
        p.state_fid = std::move(hp.state_fid);
        p.trans_fid = std::move(hp.trans_fid);
        p.empirical = std::move(hp.empirical);
        t->probs.push_back(std::move(p));
    }
    int rc = check_device(device);
    if (rc) return rc;
    t->device = device;
    t->h_in.assign(size_t(in_total), 0.0);
    t->h_out.assign(size_t(out_total), 0.0);
    if ((rc = set_device(device))) return rc;
    if ((rc = t->stream.create())) return rc;
    if ((rc = t->d_item_ptr.upload(item_ptr_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_id.upload(attr_id_c, "trainer upload"))) return rc;
    if ((rc = t->d_label.upload(label_c, "trainer upload"))) return rc;
    if ((rc = t->d_win_start.upload(win_start_c, "trainer upload"))) return rc;
    if ((rc = t->d_win_len.upload(win_len_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_first.upload(iw_first_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_cnt.upload(iw_cnt_c, "trainer upload"))) return rc;
    if ((rc = t->d_iw_off.upload(iw_off_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_ptr.upload(attr_ptr_c, "trainer upload"))) return rc;
    if ((rc = t->d_attr_items.upload(attr_items_c, "trainer upload"))) return rc;
    if ((rc = t->d_in.upload(t->h_in, "trainer alloc"))) return rc;
    if ((rc = t->d_out.upload(t->h_out, "trainer alloc"))) return rc;
    if ((rc = t->d_scratch.alloc(size_t(scratch_total), "trainer alloc"))) return rc;
    if ((rc = t->d_attr_value.upload(attr_value_c, "trainer upload"))) return rc;
    if ((rc = t->d_allowed.upload(allowed_c, "trainer upload"))) return rc;
    for (int32_t k = 0; k < n_problems; ++k) {
        const TrainerGeneral::Prob &p = t->probs[size_t(k)];
        if (p.wt0 < 0 || weighting[size_t(k)].empty()) continue;
        if ((rc = check_hip(hipMemcpy(t->d_scratch.get() + p.sc0 + p.wt0, weighting[size_t(k)].data(),
                                      weighting[size_t(k)].size() * sizeof(double), hipMemcpyHostToDevice),
                            "trainer upload")))
            return rc;
    }
    for (int32_t k = 0; k < n_problems; ++k) {
        const TrainerGeneral::Prob &p = t->probs[size_t(k)];
        if (p.val0 < 0 || p.nnz == 0) continue;
        if ((rc = check_hip(hipMemcpy(t->d_scratch.get() + p.sc0 + p.scratch - p.nnz, transposed[size_t(k)].data(),
                                      size_t(p.nnz) * sizeof(double), hipMemcpyHostToDevice),
                            "trainer upload")))
            return rc;
    }
    *out = t.release();
    return GECCO_CRF_OK;
}

}  // namespace

int trainer_general_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                           const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                           const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                           const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                           TrainerGeneral **out, const double *const *attr_value, const uint32_t *const *allowed,
                           const double *const *seq_weight, const double *const *label_cost) {
    if (!window || !step) return fail("trainer general: null argument");
    return trainer_general_open(device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels, window,
                                step, state_fid, trans_fid, num_features, attr_value, allowed, seq_weight, label_cost, out);
}

int trainer_sequences_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                             const int32_t *const *item_ptr, const int32_t *const *attr_id, const int32_t *const *labels,
                             const int32_t *num_attrs, const int32_t *num_labels, const int32_t *const *state_fid,
                             const int32_t *const *trans_fid, const int32_t *num_features, TrainerGeneral **out,
                             const double *const *attr_value, const uint32_t *const *allowed,
                             const double *const *seq_weight, const double *const *label_cost) {
    return trainer_general_open(device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels, nullptr,
                                nullptr, state_fid, trans_fid, num_features, attr_value, allowed, seq_weight, label_cost, out);
}

int trainer_general_eval(TrainerGeneral *t, const uint8_t *active, const double *const *w, double *f, double *const *g) {
    const std::string name = (t && t->whole) ? "trainer_sequences_eval" : "trainer_general_eval";
    if (!t || !active || !w || !f || !g) return fail(name + ": null argument");
    const int32_t P = int32_t(t->probs.size());
    for (int32_t k = 0; k < P; ++k)
        if (active[k] && (!g[k] || (t->probs[k].K > 0 && !w[k])))
            return fail(name + ": null argument for problem " + std::to_string(k));
    int64_t in_lo = INT64_MAX, in_hi = 0, out_lo = INT64_MAX, out_hi = 0;
    for (int32_t k = 0; k < P; ++k) {
        const TrainerGeneral::Prob &p = t->probs[k];
        if (!active[k] || p.n_win == 0) continue;
        double *ws = t->h_in.data() + p.in0, *tr = ws + p.state_fid.size();
        for (size_t j = 0; j < p.state_fid.size(); ++j) ws[j] = p.state_fid[j] >= 0 ? w[k][p.state_fid[j]] : 0.0;
        for (size_t j = 0; j < p.trans_fid.size(); ++j) tr[j] = p.trans_fid[j] >= 0 ? w[k][p.trans_fid[j]] : 0.0;
        const int64_t cols = 1 + int64_t(p.L) * p.L;
        in_lo = std::min(in_lo, p.in0);
        in_hi = std::max(in_hi, p.in0 + int64_t(p.state_fid.size() + p.trans_fid.size()));
        out_lo = std::min(out_lo, p.out0);
        out_hi = std::max(out_hi, p.out0 + cols + int64_t(p.A) * p.L);
    }
    int rc = set_device(t->device);
    if (rc) return rc;
    hipStream_t st = t->stream.get();
    if (in_hi > 0) {
        if ((rc = check_hip(hipMemcpyAsync(t->d_in.get() + in_lo, t->h_in.data() + in_lo, size_t(in_hi - in_lo) * sizeof(double),
                                           hipMemcpyHostToDevice, st),
                            "trainer weights upload")))
            return rc;
        for (int32_t k = 0; k < P; ++k) {
            const TrainerGeneral::Prob &p = t->probs[k];
            if (!active[k] || p.n_win == 0) continue;
            const int64_t cols = 1 + int64_t(p.L) * p.L, nl = int64_t(p.n_items) * p.L;
            GenProb a;
            a.item_ptr = t->d_item_ptr.get() + p.iptr0;
            a.attr_id = t->d_attr_id.get() + p.nnz0;
            a.label = t->d_label.get() + p.item0;
            a.win_start = t->d_win_start.get() + p.win0;
            a.win_len = t->d_win_len.get() + (t->whole ? p.win0 : 0);
            // (the item coverage is the windowed family's alone: in a whole-sequence trainer the arrays are empty)
            a.iw_first = t->d_iw_first.get() + (t->whole ? 0 : p.item0);
            a.iw_cnt = t->d_iw_cnt.get() + (t->whole ? 0 : p.item0);
            a.iw_off = t->d_iw_off.get() + (t->whole ? 0 : p.item0);
            a.attr_ptr = t->d_attr_ptr.get() + p.aptr0;
            a.attr_items = t->d_attr_items.get() + p.nnz0;
            a.wstate = t->d_in.get() + p.in0;
            a.trans = a.wstate + int64_t(p.A) * p.L;
            a.score = t->d_scratch.get() + p.sc0;
            a.item_marg = a.score + nl;
            a.marg = a.item_marg + nl;
            a.partial = a.marg + p.n_win * p.W * p.L;
            a.slab = a.partial + int64_t(p.n_blocks) * cols;
            a.out = t->d_out.get() + p.out0;
            a.n_win = p.n_win;
            a.n_items = p.n_items, a.A = p.A, a.L = p.L, a.W = p.W, a.step = p.step, a.n_blocks = p.n_blocks;
            const unsigned nb_items = unsigned(blocks_of(nl, kTrainGenThreads));
            const int G = group_of(p.L);
            // (a problem has values or has none: the branch is the same for every thread of its launches)
            const bool valued = p.val0 >= 0;
            const double *attr_value = valued ? t->d_attr_value.get() + p.val0 : nullptr;
            const double *attr_item_value = valued ? t->d_scratch.get() + p.sc0 + p.scratch - p.nnz : nullptr;
            if (valued)
                gen_item_scores<true><<<nb_items, kTrainGenThreads, 0, st>>>(a, attr_value);
            else
                gen_item_scores<false><<<nb_items, kTrainGenThreads, 0, st>>>(a, nullptr);
            // kernel 2: the instantiation of the problem's group size and family; a problem with masks runs both passes in
            // one kernel, which hands on their difference
            const bool masked = p.allow0 >= 0;
            const uint32_t *al = masked ? t->d_allowed.get() + p.allow0 : nullptr;
            double *la_a = masked ? a.slab + kTrainGenReduceSlabs * cols : nullptr;
            // (a weighted problem: its instance weights and, with costs, its cost matrix, where create put them)
            const double *inst_weight = p.wt0 >= 0 ? t->d_scratch.get() + p.sc0 + p.wt0 : nullptr;
            const double *cost = p.cost0 >= 0 ? t->d_scratch.get() + p.sc0 + p.cost0 : nullptr;
            const unsigned nb = unsigned(p.n_blocks);
            with_group(G, [&](auto g) {
                constexpr int kG = decltype(g)::value;
                auto launch = [&](auto whole) {
                    constexpr bool kWhole = decltype(whole)::value;
                    if (masked && inst_weight)
                        gen_partial<kG, kWhole, true><<<nb, kTrainGenThreads, 0, st>>>(a, al, la_a, inst_weight);
                    else if (masked)
                        gen_partial<kG, kWhole, false><<<nb, kTrainGenThreads, 0, st>>>(a, al, la_a, nullptr);
                    else if (inst_weight)
                        gen_labelled<kG, kWhole, true><<<nb, kTrainGenThreads, 0, st>>>(a, inst_weight, cost);
                    else
                        gen_labelled<kG, kWhole, false><<<nb, kTrainGenThreads, 0, st>>>(a, nullptr, nullptr);
                };
                if (t->whole)
                    launch(std::true_type{});
                else
                    launch(std::false_type{});
            });
            if (!t->whole) gen_item_marginals<<<nb_items, kTrainGenThreads, 0, st>>>(a);
            if (valued)
                gen_attr_counts<true><<<unsigned(p.A), kTrainGenThreads, 0, st>>>(a, G, attr_item_value);
            else
                gen_attr_counts<false><<<unsigned(p.A), kTrainGenThreads, 0, st>>>(a, G, nullptr);
            gen_reduce_blocks<<<kTrainGenReduceSlabs, kTrainGenThreads, 0, st>>>(a);
            gen_reduce_final<<<1, kTrainGenThreads, 0, st>>>(a);
        }
        if ((rc = check_hip(hipGetLastError(), "trainer kernels"))) return rc;
        if ((rc = check_hip(hipMemcpyAsync(t->h_out.data() + out_lo, t->d_out.get() + out_lo, size_t(out_hi - out_lo) * sizeof(double),
                                           hipMemcpyDeviceToHost, st),
                            "trainer download")))
            return rc;
        if ((rc = check_hip(hipStreamSynchronize(st), "trainer synchronize"))) return rc;
    }
    for (int32_t k = 0; k < P; ++k) {
        if (!active[k]) continue;
        const TrainerGeneral::Prob &p = t->probs[k];
        double *gk = g[k];
        if (p.n_win == 0) {  // no windows: nothing ran
            f[k] = 0.0;
            for (int32_t j = 0; j < p.K; ++j) gk[j] = 0.0;
            continue;
        }
        const double *o = t->h_out.data() + p.out0;  // f, xi [L][L], expected state counts [A][L]
        const double *expected = o + 1 + p.trans_fid.size();
        f[k] = o[0];
        for (int32_t j = 0; j < p.K; ++j) gk[j] = -p.empirical[j];
        for (size_t j = 0; j < p.state_fid.size(); ++j)
            if (p.state_fid[j] >= 0) gk[p.state_fid[j]] += expected[j];
        for (size_t j = 0; j < p.trans_fid.size(); ++j)
            if (p.trans_fid[j] >= 0) gk[p.trans_fid[j]] += o[1 + j];
    }
    return GECCO_CRF_OK;
}

int32_t trainer_general_num_problems(const TrainerGeneral *t) { return t ? int32_t(t->probs.size()) : -1; }

int64_t trainer_general_num_windows(const TrainerGeneral *t, int32_t k) {
    return (t && k >= 0 && k < int32_t(t->probs.size())) ? t->probs[k].n_win : -1;
}

int64_t trainer_general_scratch_bytes(const TrainerGeneral *t, int32_t k) {
    if (!t || k < -1 || k >= int32_t(t->probs.size())) return -1;
    if (k >= 0) return t->probs[k].scratch * int64_t(sizeof(double));
    int64_t total = 0;
    for (const TrainerGeneral::Prob &p : t->probs) total += p.scratch;
    return total * int64_t(sizeof(double));
}

void trainer_general_destroy(TrainerGeneral *t) { delete t; }

}  // namespace gecco
