// Circular contigs: exact log Z, marginals and the best label path of a ring.  A ring of T >= 1 genes has T
// edges, t -> (t + 1) mod T, all scored by the model's one transition table: the last gene has a transition into the first.
//   score(y) = sum_t state_t[y_t] + sum_{t = 0 .. T-1} trans[y_t][y_{(t+1) mod T}]
// A ring of one gene has the self-edge trans[y_0][y_0], a ring of two both trans[y_0][y_1] and trans[y_1][y_0].
// gl_state (crf_general.hip) leaves the raw state scores in GenArgs::state, -infinity at a disallowed (gene, label) pair; nothing
// else of the marginals' workspace is read.  The file is compiled without floating-point contraction, like crf_minrun.hip.
//
// The recursion runs on the whole-contig lattice expanded by the START label a = y_0: a counter lattice whose slots never mix.
//   F_0[a][j] = state_0[a] if j = a, else -infinity          F_t[a][j] = R_i(F_{t-1}[a][i] + trans[i][j]) + state_t[j]
//   closed[a] = R_j(F_{T-1}[a][j] + trans[j][a])             log Z_ring = LSE_a closed[a],  best = max_a closed[a]
// with R the max-shifted log-sum-exp (sum semiring) or the max (max semiring).  The L conditioned chains meet at the closure only.
//   B_{T-1}[a][i] = trans[i][a]          B_t[a][i] = LSE_k((trans[i][k] + state_{t+1}[k]) + B_{t+1}[a][k])
//   P(y_t = i | x) = sum over a, ascending, of exp((F_t[a][i] + B_t[a][i]) - log Z_ring)
//
// gl_ring_forward<LP, SUM, STORE>: the frame of crf_contig_walk.hpp (group geometry, columns in LDS, gene loop, the two reducers
// over sources(f), the end-of-contig reductions), one lane per destination label j.  A lane's column, [L | 1] doubles: F_t[a][j]
// at slot a.  A destination (a, j) reads slot a of every source lane and nothing else.  The closure runs in lane a: it reads slot
// a of every lane j of its group with its own column of trans (trans[j][a]), then the group reduces over a -- a log-sum-exp by
// the butterflies (one order in every lane), or an arg max in which the smaller start label wins a tie.
//   The sum walk keeps its values small.  A gene takes two passes over its slots.  The first leaves every destination's largest
// source, mx[a], in the lane's own new column, and the group takes sigma_t = the maximum over its L * L destinations of mx +
// state_t[j] (0 when there is none; sigma_0 = 0).  The second forms (mx + (state_t[j] - sigma_t)) + log(sum of exp(source - mx)):
// the stored value is F_t - S_t, S_t = sigma_1 + .. + sigma_t, at most log L, and the destinations that carry the mass are near
// 0 whatever t and however large the weights, so their rounding error grows neither with the ring's length nor with the
// weights (unshifted, a marginal of a 300-gene ring was off by 1.2e-12, and with weights of 700 by more at 100 genes).
// log Z_ring = S_{T-1} + LSE_a of the shifted closed[a].  The backward walk subtracts sigma_{t+1} at gene t, with the state
// score of gene t + 1, so that F + B carries S_{T-1} at every gene and the marginal is exp((F + B) - LSE_a closed[a]) on
// shifted values alone: no accumulated sum enters a marginal.
//   SUM leaves log Z_ring; <SUM, STORE> also writes every (shifted) forward value to a workspace, [gene][start label][label] (the lanes of a group
// write and read neighbouring doubles),
// then sigma [gene] and the shifted log Z [ring] -- 8 (n_genes L L + n_genes + n_contigs) bytes -- and changes no arithmetic.
// The max instantiation is not shifted (its score is the plain left-to-right sum) and keeps no back-pointers: it leaves
// closed[a*] (the score's bits) and a*.
// gl_ring_viterbi: the walk conditioned on y_0 = a*, one slot, one byte of back-pointer per (gene, label); sources in ascending
// label order with a strict `>` (predict's rule: the earlier source wins); the last label is the first arg max of
// V_{T-1}[a*][j] + trans[j][a*].  Its values are slot a* of the max walk, operation for operation.
// gl_ring_backtrack: one lane per ring, last gene to first.
// gl_ring_backward: the geometry transposed, one lane per SOURCE label i with its row of trans; B_t[a][i] at slot a, and beside
// the columns one double per lane, the state score of the gene the column belongs to.  It writes the marginals as it goes.
// Values are (previous + trans) + state, every addition rounded on its own.  A ring is one sequential walk; it is not chunked.
// Without a feasible path: log Z_ring and the score -infinity, label -1 at every gene, marginals 0.0; never NaN.  No atomics.
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

template <int LP, bool SUM, bool STORE = false>
__global__ void __launch_bounds__(kWalkLanes) gl_ring_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                              const int32_t *__restrict__ contig_ptr, const int L, const int n_contigs,
                                                              double *__restrict__ out, int32_t *__restrict__ start,
                                                              double *__restrict__ fwd, double *__restrict__ sigma,
                                                              double *__restrict__ lz_shifted) {
    static_assert(SUM || !STORE, "the forward values are the sum semiring's");
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][L | 1]
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, L);
    const int KS = cols.KS;
    double shifts = 0.0;  // (sum semiring) S_t
    {
        const double s0 = g.state_at(st, L, 0 < T, 0);
        cols.fill(lane, g.on ? j : -1, s0);  // the chain that starts at the lane's own label, and no other
        if constexpr (STORE) {
            if (g.on && T > 0) {
                const size_t b0 = static_cast<size_t>(g.g0) * L * L + g.jj;
                for (int a = 0; a < L; ++a) fwd[b0 + static_cast<size_t>(a) * L] = a == j ? s0 : ninf;
                if (j == 0) sigma[g.g0] = 0.0;
            }
        }
    }
    __syncthreads();  // (one wave)
    // one gene: the lane's label under every start label, in slot order
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double *mine = cols.gen(t) + lane * KS;
        const size_t bk = static_cast<size_t>(g.g0 + (act ? t : 0)) * L * L + g.jj;
        if constexpr (SUM) {
            // the first pass: every destination's largest source, and from them the gene's shift
            double top = ninf;
#pragma unroll 1
            for (int a = 0; a < L; ++a) {
                double mx = ninf;
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    const double v = prev[i * KS + a] + tcol[i];  // (a lane without a label holds -infinity)
                    mx = v > mx ? v : mx;
                }
                if (act) mine[a] = mx;  // (a group that has ended keeps its last column: the buffers alternate)
                const double c = mx + s_t;
                top = c > top ? c : top;
            }
            const double m = group_max<LP>(g.on ? top : ninf);  // (every lane of the wave shuffles)
            const double sig = m > ninf ? m : 0.0;
            const double s_in = s_t - sig;
            // the second pass: the log-sum-exp around that source, then the shifted state score
#pragma unroll 1
            for (int a = 0; a < L; ++a) {
                const double mx = mine[a];  // (the lane's own store; unused where the group has ended)
                const double shift = mx > ninf ? mx : 0.0;
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    const double v = prev[i * KS + a] + tcol[i];
                    sum += v > ninf ? exp(v - shift) : 0.0;
                }
                const double value = mx > ninf ? (mx + s_in) + log(sum) : ninf;
                if (act) {
                    mine[a] = value;
                    if constexpr (STORE) {
                        if (g.on) fwd[bk + static_cast<size_t>(a) * L] = value;
                    }
                }
            }
            if (act) {
                shifts += sig;
                if constexpr (STORE) {
                    if (j == 0) sigma[g.g0 + t] = sig;
                }
            }
        } else {
#pragma unroll 1
            for (int a = 0; a < L; ++a) {
                const auto sources = [&](auto &&f) {
#pragma unroll
                    for (int i = 0; i < LP; ++i) f(i, prev[i * KS + a] + tcol[i], false);  // (a lane without a label holds -infinity)
                };
                int arg;
                const double value = walk_max(sources, arg) + s_t;
                if (act) mine[a] = value;
            }
        }
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the closing edge, in the lane of the start label: every end label j into a, with the lane's column trans[j][a]
    const double *fin = cols.gen(T > 0 ? T - 1 : 0) + g.row0 * KS;
    const auto closing = [&](auto &&f) {
#pragma unroll
        for (int i = 0; i < LP; ++i) f(i, fin[i * KS + g.jj] + tcol[i], false);
    };
    const bool mine_counts = g.on && T > 0;
    if constexpr (SUM) {
        const WalkSum r = walk_sum(closing);
        const double lse = group_lse<LP>(mine_counts ? r.value : ninf);  // (of the shifted values)
        if (g.valid && j == 0) {
            out[g.c] = T > 0 ? shifts + lse : 0.0;
            if constexpr (STORE) lz_shifted[g.c] = T > 0 ? lse : 0.0;
        }
    } else {
        int arg;
        const double closed = walk_max(closing, arg);
        double v = mine_counts ? closed : ninf;
        int a = j;
        group_argmax<LP>(v, a);  // the smaller start label wins a tie
        if (g.valid && j == 0) {
            out[g.c] = T > 0 ? v : 0.0;  // (a ring without genes: the score of gl_viterbi_seq's convention)
            start[g.c] = v > ninf ? a : -1;
        }
    }
}

// The Viterbi walk of the chain that starts at a* (start[c], the max walk's, earlier on the stream), with back-pointers.
template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_ring_viterbi(const double *__restrict__ state, const double *__restrict__ trans,
                                                              const int32_t *__restrict__ contig_ptr, const int L, const int n_contigs,
                                                              const int32_t *__restrict__ start, uint8_t *__restrict__ back,
                                                              int8_t *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][1]
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, 1);
    int a = g.valid && T > 0 ? start[g.c] : -1;
    a = a >= 0 && a < L ? a : -1;  // (no address below leaves trans)
    cols.fill(lane, g.on && j == a ? 0 : -1, g.state_at(st, L, 0 < T, 0));
    __syncthreads();  // (one wave)
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0;
        const auto sources = [&](auto &&f) {
#pragma unroll
            for (int i = 0; i < LP; ++i) f(i, prev[i] + tcol[i], false);
        };
        int arg;
        const double value = walk_max(sources, arg) + s_t;
        if (act) {
            cols.gen(t)[lane] = value;
            if (g.on) back[static_cast<size_t>(g.g0 + t) * L + g.jj] = static_cast<uint8_t>(arg);
        }
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the closing edge into a*: the first arg max over the end labels
    double v = (g.on && a >= 0) ? cols.gen(T - 1)[lane] + trans[g.jj * L + a] : ninf;
    int bj = j;
    group_argmax<LP>(v, bj);
    if (g.valid && j == 0 && T > 0) y[static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)] = v > ninf ? static_cast<int8_t>(bj) : int8_t(-1);
}

__global__ void __launch_bounds__(kWalkBack) gl_ring_backtrack(const uint8_t *__restrict__ back, const int32_t *__restrict__ contig_ptr,
                                                              const int L, const int n_contigs, int8_t *__restrict__ y) {
    const size_t c = static_cast<size_t>(blockIdx.x) * kWalkBack + threadIdx.x;
    if (c >= static_cast<size_t>(n_contigs)) return;
    const int g0 = contig_ptr[c], T = contig_ptr[c + 1] - g0;
    if (T <= 0) return;
    int8_t *col = y + static_cast<size_t>(g0);
    int lab = col[T - 1];  // (gl_ring_viterbi's, earlier on the stream)
    if (lab < 0) {
        for (int t = 0; t < T; ++t) col[t] = -1;
        return;
    }
    for (int t = T - 1; t >= 1; --t) {
        if (lab >= L) lab = 0;  // (cannot happen: a finite state points at a finite state; no address leaves the workspace)
        lab = back[static_cast<size_t>(g0 + t) * L + lab] & 0x1f;
        col[t - 1] = static_cast<int8_t>(lab);
    }
}

// The backward walk and the marginals.  The groups of a wave start at their rings' last genes, so step u is gene T - 2 - u of
// each; a group that has reached gene 0 stores nothing more.  State scores come eight steps ahead.  One barrier per step, outside
// every divergent branch.  The values are shifted like the forward walk's: gene t subtracts sigma_{t+1}, which comes with the
// state score of gene t + 1, eight steps ahead.  marg[g][i] = the sum over the start labels, ascending, of exp((F + B) - log Z), all
// three shifted, at most 1; a state that no path visits adds exactly 0.0, and so does every state of a ring without a feasible
// path.
template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_ring_backward(const double *__restrict__ state, const double *__restrict__ trans,
                                                               const int32_t *__restrict__ contig_ptr, const int L, const int n_contigs,
                                                               const double *__restrict__ fwd, const double *__restrict__ sigma,
                                                               const double *__restrict__ lz_shifted, double *__restrict__ marg) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][L | 1] B, then [2][kWalkLanes] state scores
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, ii = g.jj, T = g.T;
    const bool on = g.on;
    const double lz = g.valid ? lz_shifted[g.c] : ninf;
    const bool feasible = lz > ninf;
    double trow[LP];
    g.template load_trans<true>(trans, L, trow);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, L);
    const int KS = cols.KS;
    double *const sb0 = cols_lds + 2 * kWalkLanes * KS, *const sb1 = sb0 + kWalkLanes;
    // the state score of the gene u steps before the last one, less that gene's shift
    const auto fetch = [&](int u) {
        const double s = g.state_at(st, L, u < T, T - 1 - u);
        return u < T ? s - sigma[g.g0 + (T - 1 - u)] : s;
    };
    const auto emit = [&](const bool act, const int t, const double p) {
        if (act && on) marg[(static_cast<size_t>(g.g0) + static_cast<size_t>(t)) * L + ii] = gl_prob(p);
    };
    {
        // the last gene: B is the closing edge into every start label, the lane's row of trans
        double *mine = cols.buf0 + lane * KS;
        for (int a = 0; a < KS; ++a) {
            mine[a] = (on && a < L) ? trans[ii * L + a] : ninf;
            cols.buf1[lane * KS + a] = ninf;
        }
        sb0[lane] = fetch(0);
        sb1[lane] = ninf;
        double p = 0.0;
        if (T > 0 && on) {
            const size_t ak = (static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)) * L * L + ii;
            for (int a = 0; a < L; ++a) {
                const double ab = fwd[ak + static_cast<size_t>(a) * L] + mine[a];
                p += (feasible && ab > ninf) ? exp(ab - lz) : 0.0;
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
        double ts[LP];  // what every successor label costs on top of its B
#pragma unroll
        for (int k = 0; k < LP; ++k) ts[k] = trow[k] + sprev[k];
        const size_t ak = (static_cast<size_t>(g.g0) + static_cast<size_t>(act ? t : 0)) * L * L + ii;
        double p = 0.0;
#pragma unroll 1
        for (int a = 0; a < L; ++a) {
            const double f = (act && on) ? fwd[ak + static_cast<size_t>(a) * L] : ninf;
            const auto successors = [&](auto &&fn) {
#pragma unroll
                for (int k = 0; k < LP; ++k) fn(k, prev[k * KS + a] + ts[k], false);  // (a lane without a label: state -infinity)
            };
            const WalkSum r = walk_sum(successors);
            const double b = (on && r.finite) ? r.value : ninf;
            if (act) {
                mine[a] = b;
                const double ab = f + b;
                p += (feasible && ab > ninf) ? exp(ab - lz) : 0.0;
            }
        }
        if (act) (((u & 1) ? sb0 : sb1))[lane] = s_t;
        emit(act, t, p);
        __syncthreads();
    };
    contig_walk(0, T - 1, [&](int u) { return fetch(u + 1); }, step);
}

template <int LP, bool SUM, bool STORE = false>
void launch_forward(const GenArgs &a, double *out, int32_t *start, double *fwd, double *sigma, double *lz_shifted, hipStream_t stream) {
    hipLaunchKernelGGL((gl_ring_forward<LP, SUM, STORE>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(a.L), stream,
                       a.state, a.trans, a.contig_ptr, a.L, a.n_contigs, out, start, fwd, sigma, lz_shifted);
}

}  // namespace

size_t ring_forward_bytes(int64_t n_genes, int32_t L, int32_t n_contigs) {
    return sizeof(double) * (static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(L) + static_cast<size_t>(n_genes) +
                             static_cast<size_t>(n_contigs));
}

size_t ring_back_bytes(int64_t n_genes, int32_t L) { return static_cast<size_t>(n_genes) * static_cast<size_t>(L); }

hipError_t launch_gen_ring(const GenArgs &a, const RingArgs &q, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !q.lognorm_ring || (q.marg && !q.fwd) || (!q.y != !q.score) || (q.y && (!q.back || !q.start)))
        return hipErrorNotSupported;
    hipError_t e;
    if (q.marg) {
        // the workspace: the forward values, then sigma per gene, then the shifted log Z per ring
        double *sigma = q.fwd + static_cast<size_t>(a.n_genes) * a.L * a.L, *lz_shifted = sigma + a.n_genes;
        dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true, true>(a, q.lognorm_ring, nullptr, q.fwd, sigma, lz_shifted, stream); });
        if ((e = hipGetLastError()) != hipSuccess) return e;
        dispatch_lp(a.L, [&](auto lp) {
            const size_t lds = walk_lds_bytes(a.L) + size_t(2) * kWalkLanes * sizeof(double);  // (the columns, then the state scores)
            hipLaunchKernelGGL((gl_ring_backward<lp>), dim3(walk_blocks<lp>(a.n_contigs)), dim3(kWalkLanes), lds, stream, a.state, a.trans,
                               a.contig_ptr, a.L, a.n_contigs, q.fwd, sigma, lz_shifted, q.marg);
        });
    } else {
        dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true>(a, q.lognorm_ring, nullptr, nullptr, nullptr, nullptr, stream); });
    }
    if ((e = hipGetLastError()) != hipSuccess || !q.y) return e;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, false>(a, q.score, q.start, nullptr, nullptr, nullptr, stream); });
    if ((e = hipGetLastError()) != hipSuccess) return e;
    dispatch_lp(a.L, [&](auto lp) {
        hipLaunchKernelGGL((gl_ring_viterbi<lp>), dim3(walk_blocks<lp>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(1), stream, a.state,
                           a.trans, a.contig_ptr, a.L, a.n_contigs, q.start, q.back, q.y);
    });
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(a.n_contigs) + kWalkBack - 1) / kWalkBack);
    hipLaunchKernelGGL(gl_ring_backtrack, dim3(blocks), dim3(kWalkBack), 0, stream, q.back, a.contig_ptr, a.L, a.n_contigs, q.y);
    return hipGetLastError();
}

}  // namespace gecco
