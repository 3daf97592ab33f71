// Run-length potentials: the best label path, the log-mass, the marginals and the expected run-length counts of every contig under
// a score on the length of a run.  A label set S, a table g[1 .. M] (1 <= M <= 32, every entry finite or
// -infinity) and a tail score tau (finite or -infinity).  A run is crf_minrun.hip's: a maximal stretch of genes with labels in S,
// runs at a contig's first or last gene like any other, the labels inside a run free to differ.  A path y with runs of n_r genes has
//   score_g(y) = score(y) + sum over its runs of ( g[min(n_r, M)] + tau * max(n_r - M, 0) ),
// and a term of -infinity makes the path infeasible.  g = 0, tau = 0 is the plain lattice; g = (-inf, .., -inf, 0), tau = 0 is
// crf_minrun.hip's minimum M; tau = -inf is a maximum run length M.  gl_state (crf_general.hip) leaves the raw state scores in
// GenArgs::state; nothing else of the marginals' workspace is read.  Compiled without floating-point contraction.
//
// States: crf_minrun.hip's.  A label outside S has one state; a label j in S has (j, d), d = 1 .. M, d = min(run length so far, M);
// at gene 0 (j, 1) and the outside states start at state_0[j], the others at -infinity.  What is new is the exit aggregate of a
// source label, A_t(i) = (+)_d (alpha_t(i, d) + g[d]) for i in S and alpha_t(i) for i outside: a run is scored where it ends.
// The sources of a destination at gene t:
//   j outside S             every label i: A_{t-1}(i) + trans[i][j]
//   (j, 1)                  alpha_{t-1}(i) + trans[i][j], i outside S; at M = 1 also (alpha_{t-1}(i, 1) + tau) + trans[i][j], i in S
//   (j, d), 1 < d < M       alpha_{t-1}(i, d - 1) + trans[i][j], i in S
//   (j, M), M > 1           (i, M - 1) as above, and (alpha_{t-1}(i, M) + tau) + trans[i][j], i in S
// then + state_t[j].  The total is (+)_i A_{T-1}(i): a run that reaches the last gene is scored like any other.
//   Max semiring: ((delta + g or tau) + trans) + state, every addition rounded on its own.  A destination's sources are scanned in
// ascending label order, a label's tau source directly behind its other one, with a strict `>`: the earlier source wins a tie.
// The aggregate is scanned with d ascending and a strict `>`.  At the end the smaller label wins among equal aggregates.  That
// is an operational tie rule on expanded states, as in crf_minrun.hip, not an order on paths.  Without a feasible path: score
// -infinity, label -1 at every gene, log Z_g -infinity; never NaN.
//   Sum semiring: the same sources, a max-shifted log-sum-exp in fp64; a destination (or an aggregate) all of whose terms are
// -infinity stays -infinity.
//
// gl_runlen_forward<LP, SUM, STORE>: the frame of crf_contig_walk.hpp, one lane per destination label.  A lane's column is
// [(M + 1) | 1] doubles: state (j, d) at slot d - 1, an outside label's one state at slot M - 1 (crf_minrun.hip's layout), and
// the aggregate at slot M, which the owning lane forms from its own column as it stores it -- M more semiring operations per gene
// and lane -- so an outside destination still reads one slot per source label.  The row length is odd: lanes that read different
// rows at one slot hit different banks (§4.9k's argument, unchanged).
//   Back-pointers (max only): crf_minrun.hip's byte per (gene, label, slot) -- the source label in the low five bits, kWalkSecond
// for the tau source -- and behind them one byte per (gene, label): the slot of the aggregate's arg max, written by the owning
// lane for a label in S.  The backtrack reads it when it leaves an outside state into a label of S, and at the contig's last gene.
//   <SUM, STORE> also writes every forward value to a workspace of 8 n_genes L M bytes and changes no arithmetic.
// gl_runlen_backtrack: one lane per contig, last gene to first.
// gl_runlen_backward<LP>: gl_minrun_backward's geometry (a lane owns a SOURCE label and its row of trans).  Per source i in S the
// lane forms the exit continuation E_t(i) = LSE over k outside S of (trans[i][k] + state_{t+1}[k]) + beta_{t+1}(k) (0 at the last
// gene), and the stay continuation C_t(i, d) = LSE over k in S of (trans[i][k] + state_{t+1}[k]) + beta_{t+1}(k, min(d + 1, M))
// (-infinity at the last gene); beta_t(i, d) = LSE(g[d] + E, C), the slot-M continuation carrying tau: LSE(g[M] + E, tau + C).
// An outside source: LSE over every k of its one entry state (slot 0 of a label in S).  marg and inside as in gl_minrun_backward.
//   Expected length counts, in the same lane and the same pass: counts[d] += exp(((alpha_t(i, d) + g[d]) + E_t(i)) - log Z_g), the
// posterior that a run ends at t with min(length, M) = d, and counts[M + 1] += exp((alpha_t(i, M) + (tau + C_t(i, M))) - log Z_g),
// the tail steps.  The sums are kept in a third block of the lane's LDS, added in walk order (last gene to first), and reduced
// across the group once, after the walk, by crf_lanes.hpp's butterfly.  No atomics: equal calls give equal bytes, and a contig's
// bytes do not depend on its neighbours.  A contig without a feasible path gets zeros.
// A contig is one sequential walk; it is not chunked.
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kLBack = kWalkBack;  // lanes per workgroup of the backtrack

// the lane's aggregate over its own column in either semiring: its value, and the slot of the arg max (max semiring)
template <bool SUM, class Terms>
__device__ __forceinline__ double runlen_aggregate(Terms &&terms, int &arg) {
    if constexpr (SUM) {
        arg = 0;
        return walk_sum(terms).value;
    } else {
        return walk_max(terms, arg);
    }
}

template <int LP, bool SUM, bool STORE = false>
__global__ void __launch_bounds__(kWalkLanes) gl_runlen_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                const int32_t *__restrict__ contig_ptr, const int L,
                                                                const int n_contigs, const uint32_t set_mask, const RunLengthScores sc,
                                                                uint8_t *__restrict__ back, uint8_t *__restrict__ back_agg,
                                                                int8_t *__restrict__ y, double *__restrict__ out,
                                                                double *__restrict__ fwd) {
    static_assert(SUM || !STORE, "the forward values are the sum semiring's");
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][(M + 1) | 1]
    const double ninf = kWalkNinf;
    const int m = sc.M, top = m - 1;
    const double tau = sc.tau;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    const bool inside = (set_mask >> j) & 1u;  // (no bit at or above L: a lane without a label is an outside lane at -infinity)
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, m + 1);
    const int KS = cols.KS;
    // the aggregate of the lane's column of gene t, into slot M (and its arg max into back_agg)
    const auto aggregate = [&](double *mine, const bool act, const int t) {
        const auto terms = [&](auto &&f) {
#pragma unroll 1
            for (int d = 0; d < m; ++d) {
                const double v = mine[d] + sc.g[d];
                f(d, inside ? v : ninf, false);
            }
        };
        int arg;
        const double a = runlen_aggregate<SUM>(terms, arg);
        if (act) {
            mine[m] = inside ? a : mine[top];
            if constexpr (!SUM) {
                if (g.on && inside) back_agg[static_cast<size_t>(g.g0 + t) * L + g.jj] = static_cast<uint8_t>(arg);
            }
        }
    };
    {
        const double s0 = g.state_at(st, L, 0 < T, 0);
        const int first = inside ? 0 : top;
        cols.fill(lane, first, s0);
        if constexpr (STORE) {
            if (g.on && T > 0) {
                const size_t b0 = (static_cast<size_t>(g.g0) * L + g.jj) * static_cast<size_t>(m);
                for (int k = first; k < m; ++k) fwd[b0 + k] = k == first ? s0 : ninf;
            }
        }
        aggregate(cols.gen(0) + lane * KS, T > 0, 0);
    }
    __syncthreads();  // (one wave)
    // one gene: the lane's states in slot order.  An outside lane has its one state at slot M - 1 and idles before it.
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double *mine = cols.gen(t) + lane * KS;
        const size_t bk = (static_cast<size_t>(g.g0 + (act ? t : 0)) * L + g.jj) * static_cast<size_t>(m);
#pragma unroll 1
        for (int d = 0; d < m; ++d) {
            const bool last = d == top;  // (wave-uniform)
            // where this destination's sources lie: the labels (`from`) and their slot; at d = M a tau source behind each, at slot M - 1
            const bool opens = !inside || d == 0;  // an outside state, or the first gene of a run: the aggregates (alpha itself outside S)
            const uint32_t from = !inside ? ~0u : (d == 0 ? ~set_mask : set_mask);
            const int slot = opens ? m : d - 1;
            const bool two = inside && last;
            const auto sources = [&](auto &&f) {
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    const bool src = (from >> i) & 1u;
                    const double v = prev[i * KS + slot] + tcol[i];
                    f(i, src ? v : ninf, false);
                    if (last) {  // (wave-uniform)
                        const double w = (prev[i * KS + top] + tau) + tcol[i];
                        f(i, (two && ((set_mask >> i) & 1u)) ? w : ninf, true);
                    }
                }
            };
            int arg;
            const double value = walk_value<SUM>(sources, s_t, arg);
            if (act && (inside || last)) {
                mine[d] = value;
                if constexpr (!SUM) {
                    if (g.on) back[bk + d] = static_cast<uint8_t>(arg);
                }
                if constexpr (STORE) {
                    if (g.on) fwd[bk + d] = value;
                }
            }
        }
        aggregate(mine, act, act ? t : 0);
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the end of the contig: every lane its label's aggregate
    double v = T > 0 ? cols.gen(T - 1)[lane * KS + m] : ninf;
    if constexpr (SUM) {
        const double lse = group_lse<LP>(v);
        if (g.valid && j == 0) out[g.c] = T > 0 ? lse : 0.0;
    } else {
        int bj = j;
        group_argmax<LP>(v, bj);
        if (g.valid && j == 0) {
            // (a contig without genes: the score of gl_viterbi_seq's convention)
            out[g.c] = T > 0 ? v : 0.0;
            if (T > 0) y[static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)] = v > ninf ? static_cast<int8_t>(bj) : int8_t(-1);
        }
    }
}

__global__ void __launch_bounds__(kLBack) gl_runlen_backtrack(const uint8_t *__restrict__ back, const uint8_t *__restrict__ back_agg,
                                                              const int32_t *__restrict__ contig_ptr, const int L, const int n_contigs,
                                                              const int m, const uint32_t set_mask, int8_t *__restrict__ y) {
    const size_t c = static_cast<size_t>(blockIdx.x) * kLBack + threadIdx.x;
    if (c >= static_cast<size_t>(n_contigs)) return;
    const int g0 = contig_ptr[c], T = contig_ptr[c + 1] - g0;
    if (T <= 0) return;
    int8_t *col = y + static_cast<size_t>(g0);
    int lab = col[T - 1];  // (the forward kernel's, earlier on the stream)
    if (lab < 0) {
        for (int t = 0; t < T; ++t) col[t] = -1;
        return;
    }
    const int top = m - 1;
    const size_t M = static_cast<size_t>(m);
    // the slot in which a run through label `l` of S at gene t ends: the aggregate's arg max
    const auto exit_slot = [&](const int t, const int l) { return static_cast<int>(back_agg[static_cast<size_t>(g0 + t) * L + l]); };
    int slot = ((set_mask >> lab) & 1u) ? exit_slot(T - 1, lab) : top;
    for (int t = T - 1; t >= 1; --t) {
        if (lab >= L || slot < 0 || slot > top) {  // (cannot happen: a finite state points at a finite state; no address leaves the workspace)
            lab = 0;
            slot = top;
        }
        const uint8_t b = back[(static_cast<size_t>(g0 + t) * L + lab) * M + static_cast<size_t>(slot)];
        const bool inside = (set_mask >> lab) & 1u;
        const int src = b & 0x1f;
        const bool src_inside = src < L && ((set_mask >> src) & 1u);
        if (!inside) slot = src_inside ? exit_slot(t - 1, src) : top;   // out of an outside state: where the run before it ended
        else if (b & kWalkSecond) slot = top;                          // the tau source: (src, M)
        else if (slot == 0) slot = top;                                // the first gene of a run: an outside state
        else slot = slot - 1;
        lab = src;
        col[t - 1] = static_cast<int8_t>(lab);
    }
}

// log(exp(a) + exp(b)), max-shifted; -infinity when both are
__device__ __forceinline__ double runlen_lse2(const double a, const double b) {
    const double mx = a > b ? a : b;
    if (!(mx > kWalkNinf)) return kWalkNinf;
    return mx + log(exp(a - mx) + exp(b - mx));
}

template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_runlen_backward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                 const int32_t *__restrict__ contig_ptr, const int L,
                                                                 const int n_contigs, const uint32_t set_mask, const RunLengthScores sc,
                                                                 const double *__restrict__ fwd, const double *__restrict__ lognorm_g,
                                                                 double *__restrict__ marg, double *__restrict__ inside_out,
                                                                 double *__restrict__ counts) {
    // [2][kWalkLanes][(M + 1) | 1] beta, then [2][kWalkLanes] state scores, then [kWalkLanes][(M + 1) | 1] the lane's count sums
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];
    const double ninf = kWalkNinf;
    const int m = sc.M, top = m - 1;
    const double tau = sc.tau;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, i = g.j, ii = g.jj, T = g.T;
    const bool on = g.on;
    const bool inside = (set_mask >> i) & 1u;
    const double lz = g.valid ? lognorm_g[g.c] : ninf;
    const bool feasible = lz > ninf;
    double trow[LP];
    g.template load_trans<true>(trans, L, trow);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, m + 1);
    const int KS = cols.KS;
    double *const sb0 = cols_lds + 2 * kWalkLanes * KS, *const sb1 = sb0 + kWalkLanes;
    double *const cnt = sb1 + kWalkLanes + lane * KS;
    // the state score of the gene u steps before the last one
    const auto fetch = [&](int u) { return g.state_at(st, L, u < T, T - 1 - u); };
    const auto prob = [&](const double x) { return (feasible && x > ninf) ? exp(x - lz) : 0.0; };
    // one gene's outputs; every lane of the wave comes here
    const auto emit = [&](const bool act, const int t, const double p) {
        const size_t gene = static_cast<size_t>(g.g0) + static_cast<size_t>(act ? t : 0);
        if (marg && act && on) marg[gene * L + ii] = p;
        if (inside_out) {  // (wave-uniform)
            const double s = group_sum<LP>(inside && on ? p : 0.0);
            if (act && i == 0) inside_out[gene] = s;
        }
    };
    {
        cols.fill(lane, (on && !inside) ? top : -1, 0.0);
        for (int d = 0; d <= m; ++d) cnt[d] = 0.0;
        sb0[lane] = fetch(0);
        sb1[lane] = ninf;
        double p = 0.0;
        if (T > 0 && on) {  // the last gene: a run that ends here pays g[d]; an outside state nothing
            const size_t a0 = ((static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)) * L + ii) * static_cast<size_t>(m);
            double *mine = cols.gen(0) + lane * KS;
            if (inside) {
#pragma unroll 1
                for (int d = 0; d < m; ++d) {
                    const double gd = sc.g[d];
                    mine[d] = gd;
                    const double q = prob((fwd[a0 + d] + gd) + 0.0);
                    cnt[d] += q;
                    p += q;
                }
            } else {
                p = prob(fwd[a0 + top]);
            }
        }
        emit(T > 0, T - 1, p);
    }
    __syncthreads();  // (one wave)
    const auto step = [&](const int u, const double s_t) {
        const int t = T - 2 - u;
        const bool act = t >= 0;
        const double *prev = cols.gen(u) + g.row0 * KS;
        const double *sprev = ((u & 1) ? sb1 : sb0) + g.row0;
        double *mine = cols.gen(u + 1) + lane * KS;
        double ts[LP];  // what every successor label costs on top of its beta
#pragma unroll
        for (int k = 0; k < LP; ++k) ts[k] = trow[k] + sprev[k];
        const size_t ak = ((static_cast<size_t>(g.g0) + static_cast<size_t>(act ? t : 0)) * L + ii) * static_cast<size_t>(m);
        // the exit continuation: the outside successors, each at its one state
        const auto leaving = [&](auto &&f) {
#pragma unroll
            for (int k = 0; k < LP; ++k) {
                const bool in_k = (set_mask >> k) & 1u;
                const double v = prev[k * KS + top] + ts[k];
                f(k, in_k ? ninf : v, false);
            }
        };
        const double E = walk_sum(leaving).value;
        double p = 0.0;
#pragma unroll 1
        for (int d = 0; d < m; ++d) {
            const bool last = d == top;  // (wave-uniform)
            const bool own = inside || last;
            const double a = (act && on && own) ? fwd[ak + d] : ninf;
            const int slot_in = last ? top : d + 1;
            // an outside source: every label, a label of S at the first slot of a run; a source in S: the labels of S one slot on
            const auto successors = [&](auto &&f) {
#pragma unroll
                for (int k = 0; k < LP; ++k) {
                    const bool in_k = (set_mask >> k) & 1u;
                    const int slot = inside ? slot_in : (in_k ? 0 : top);
                    const double v = prev[k * KS + slot] + ts[k];
                    f(k, (!inside || in_k) ? v : ninf, false);
                }
            };
            const double C = walk_sum(successors).value;
            const double gd = sc.g[d];
            const double stay = last ? tau + C : C;
            const double b = on ? (inside ? runlen_lse2(gd + E, stay) : C) : ninf;
            if (act && own) {
                mine[d] = b;
                p += prob(a + b);
                if (inside && on) {
                    cnt[d] += prob((a + gd) + E);
                    if (last) cnt[m] += prob(a + stay);
                }
            }
        }
        if (act) (((u & 1) ? sb0 : sb1))[lane] = s_t;
        emit(act, t, p);
        __syncthreads();
    };
    contig_walk(0, T - 1, [&](int u) { return fetch(u + 1); }, step);
    if (counts) {  // (wave-uniform) the group's sums, one order of additions in every lane
#pragma unroll 1
        for (int d = 0; d <= m; ++d) {
            const double s = group_sum<LP>(cnt[d]);
            if (g.valid && i == 0) counts[static_cast<size_t>(g.c) * static_cast<size_t>(m + 1) + d] = s;
        }
    }
}

inline size_t runlen_lds_bytes(const int32_t m) { return walk_lds_bytes(m + 1); }

template <int LP, bool SUM, bool STORE = false>
void launch_forward(const GenArgs &a, uint32_t set_mask, const RunLengthScores &sc, uint8_t *back, uint8_t *back_agg, int8_t *y,
                    double *out, hipStream_t stream, double *fwd = nullptr) {
    hipLaunchKernelGGL((gl_runlen_forward<LP, SUM, STORE>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), runlen_lds_bytes(sc.M),
                       stream, a.state, a.trans, a.contig_ptr, a.L, a.n_contigs, set_mask, sc, back, back_agg, y, out, fwd);
}

template <int LP>
void launch_backward(const GenArgs &a, uint32_t set_mask, const RunLengthScores &sc, const double *fwd, const double *lognorm_g,
                     double *marg, double *inside, double *counts, hipStream_t stream) {
    // (the columns, then the state scores, then the count sums)
    const size_t lds = runlen_lds_bytes(sc.M) + size_t(2) * kWalkLanes * sizeof(double) + runlen_lds_bytes(sc.M) / 2;
    hipLaunchKernelGGL((gl_runlen_backward<LP>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), lds, stream, a.state, a.trans,
                       a.contig_ptr, a.L, a.n_contigs, set_mask, sc, fwd, lognorm_g, marg, inside, counts);
}

// the table as the kernels take it: no NaN and no +infinity
bool scores_ok(const RunLengthScores &sc) {
    if (sc.M < 1 || sc.M > kMaxRunLength || !(sc.tau < INFINITY)) return false;
    for (int d = 0; d < sc.M; ++d)
        if (!(sc.g[d] < INFINITY)) return false;
    return true;
}

}  // namespace

size_t runlen_back_bytes(int64_t n_genes, int32_t L, int32_t max_length) {
    return static_cast<size_t>(n_genes) * static_cast<size_t>(L) * (static_cast<size_t>(max_length) + 1);
}

hipError_t launch_gen_run_length(const GenArgs &a, uint32_t set_mask, const RunLengthScores &sc, uint8_t *back, int8_t *y, double *score,
                                 double *lognorm_run_length, hipStream_t stream) {
    if (!scores_ok(sc) || !walk_counter_ok(a, set_mask, sc.M, kMaxRunLength)) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !back || !y || !score) return hipErrorNotSupported;
    uint8_t *back_agg = back + static_cast<size_t>(a.n_genes) * static_cast<size_t>(a.L) * static_cast<size_t>(sc.M);
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, false>(a, set_mask, sc, back, back_agg, y, score, stream); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(a.n_contigs) + kLBack - 1) / kLBack);
    hipLaunchKernelGGL(gl_runlen_backtrack, dim3(blocks), dim3(kLBack), 0, stream, back, back_agg, a.contig_ptr, a.L, a.n_contigs, sc.M,
                       set_mask, y);
    e = hipGetLastError();
    if (e != hipSuccess || !lognorm_run_length) return e;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true>(a, set_mask, sc, nullptr, nullptr, nullptr, lognorm_run_length, stream); });
    return hipGetLastError();
}

size_t runlen_forward_bytes(int64_t n_genes, int32_t L, int32_t max_length) {
    return sizeof(double) * static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(max_length);
}

hipError_t launch_gen_run_length_marginals(const GenArgs &a, uint32_t set_mask, const RunLengthScores &sc, double *fwd, double *marg,
                                           double *inside, double *counts, double *lognorm_run_length, hipStream_t stream) {
    if (!scores_ok(sc) || !walk_counter_ok(a, set_mask, sc.M, kMaxRunLength)) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !fwd || !lognorm_run_length || (!marg && !inside && !counts)) return hipErrorNotSupported;
    dispatch_lp(a.L, [&](auto lp) {
        launch_forward<lp, true, true>(a, set_mask, sc, nullptr, nullptr, nullptr, lognorm_run_length, stream, fwd);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    dispatch_lp(a.L, [&](auto lp) { launch_backward<lp>(a, set_mask, sc, fwd, lognorm_run_length, marg, inside, counts, stream); });
    return hipGetLastError();
}

}  // namespace gecco
