// The best label path of every contig among those without a short run, and the log-mass of all such paths.
// A label set S and a minimum m, 1 <= m <= 32: a path is feasible when every maximal run of consecutive genes with labels in S
// has at least m genes (runs at a contig's first or last gene count like any other; the labels inside a run may differ).
// gl_state (crf_general.hip) leaves the raw state scores in GenArgs::state, -infinity at a disallowed (gene, label) pair; nothing
// else of the marginals' workspace is read.  The file is compiled without floating-point contraction, like crf_kbest.hip.
//
// The recursion runs on the lattice expanded by a run counter.  A label outside S has one state; a label j in S has the states
// (j, d), d = 1 .. m, d = min(run length so far, m); states are ordered by label, then by d.  At gene 0 the states with d <= 1
// (the outside states among them) start at state_0[j], the others at -infinity.  The sources of a destination at gene t:
//   j outside S             every label i: its one state if i is outside S, (i, m) if inside (a run ends only when long enough)
//   (j, 1), m > 1           the labels i outside S
//   (j, d), 1 < d < m       (i, d - 1), i in S
//   (j, m), m > 1           (i, m - 1) and (i, m), i in S
//   (j, 1), m = 1           every label i (the expanded lattice is the plain one)
// At a contig's end the outside states and the states (j, m) are admissible.
//   Max semiring: value = (delta[source] + trans[i][j]) + state_t[j], the operation order of the other Viterbi recursions, so a
// path's score is its left-to-right sum.  Sources are scanned in ascending (label, d) order with a strict `>` update, and the
// first arg max over the admissible states in state order wins at the end.  That is an operational tie rule on expanded states,
// not "reversed path ascending" (two expanded states may stand for one label, and no local rule can order the paths behind
// them).  Without a feasible path (S every label and T < m, or masks): score -infinity, label -1 at every gene, log Z_C
// -infinity; never NaN.
//   Sum semiring: the same sources, a max-shifted log-sum-exp in place of the max; a destination all of whose sources are
// -infinity stays -infinity.
//
// gl_minrun_forward<LP, SUM>: the frame of crf_contig_walk.hpp (group geometry, columns in LDS, gene loop, the two reducers over
// sources(f), the end-of-contig reductions), one lane per destination label.  A lane's d-column, [m | 1] doubles: state (j, d) at
// slot d - 1, an outside label's one state at slot m - 1 -- so every state a run may end in, and every admissible one, is at slot
// m - 1.
//   Back-pointers (max only): one byte per (gene, label, slot), the source label in the low five bits and one bit "from d = m"
// (as against m - 1), which means something at d = m only.  The final arg max runs across the group's lanes by xor-shuffles, the
// smaller label winning a tie (one admissible state per label), and leaves the last gene's label in y, or -1.
//   SUM is the second instantiation of the same body: no back-pointers, log Z_C instead of the score.  <SUM, STORE> is the third:
// it also writes every (gene, label, slot) forward value it stores in LDS to a workspace of 8 n_genes L m bytes, the slots of a
// label that exist only (an outside label's one state at slot m - 1), and changes no arithmetic: its log Z_C has SUM's bits.
// gl_minrun_backward reads them (below, at the kernel).
// gl_minrun_backtrack: one lane per contig, last gene to first; the previous slot follows from the rule above.
// A contig is one sequential walk; it is not chunked.
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kRBack = kWalkBack;  // lanes per workgroup of the backtrack

template <int LP, bool SUM, bool STORE = false>
__global__ void __launch_bounds__(kWalkLanes) gl_minrun_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                const int32_t *__restrict__ contig_ptr, const int L,
                                                                const int n_contigs, const int m, const uint32_t set_mask,
                                                                uint8_t *__restrict__ back, int8_t *__restrict__ y,
                                                                double *__restrict__ out, double *__restrict__ fwd) {
    static_assert(SUM || !STORE, "the forward values are the sum semiring's");
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][m | 1]
    const double ninf = kWalkNinf;
    const int top = m - 1;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    const bool inside = (set_mask >> j) & 1u;  // (no bit at or above L: a lane without a label is an outside lane at -infinity)
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, m);
    const int KS = cols.KS;
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
    }
    __syncthreads();  // (one wave)
    // one gene: the lane's states in slot order.  An outside lane has its one state at the last slot and idles before it.
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double *mine = cols.gen(t) + lane * KS;
        const size_t bk = (static_cast<size_t>(g.g0 + (act ? t : 0)) * L + g.jj) * static_cast<size_t>(m);
#pragma unroll 1
        for (int d = 0; d < m; ++d) {
            const bool last = d == top;  // (wave-uniform)
            // where this destination's sources lie: the labels (`from`), their slot, and at d = m a second slot behind it
            const bool plain = !inside || m == 1;
            const uint32_t from = plain ? ~0u : (d == 0 ? ~set_mask : set_mask);
            const bool two = !plain && last;
            const int slot = plain || d == 0 ? top : (two ? top - 1 : d - 1);
            const auto sources = [&](auto &&f) {
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    const bool src = (from >> i) & 1u;
                    const double v = prev[i * KS + slot] + tcol[i];
                    f(i, src ? v : ninf, false);
                    if (last && m > 1) {  // (wave-uniform; at m = 1 no destination has a second slot to read)
                        const double w = prev[i * KS + top] + tcol[i];
                        f(i, (src && two) ? w : ninf, true);
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
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the end of the contig: every lane its label's admissible state, which is the last slot of its column
    double v = T > 0 ? cols.gen(T - 1)[lane * KS + top] : ninf;
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

__global__ void __launch_bounds__(kRBack) gl_minrun_backtrack(const uint8_t *__restrict__ back, const int32_t *__restrict__ contig_ptr,
                                                              const int L, const int n_contigs, const int m, const uint32_t set_mask,
                                                              int8_t *__restrict__ y) {
    const size_t c = static_cast<size_t>(blockIdx.x) * kRBack + threadIdx.x;
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
    int slot = top;
    for (int t = T - 1; t >= 1; --t) {
        if (lab >= L || slot < 0 || slot > top) {  // (cannot happen: a finite state points at a finite state; no address leaves the workspace)
            lab = 0;
            slot = top;
        }
        const uint8_t b = back[(static_cast<size_t>(g0 + t) * L + lab) * M + static_cast<size_t>(slot)];
        const bool inside = (set_mask >> lab) & 1u;
        if (!inside || m == 1 || slot == 0) slot = top;          // from an outside state, or from a run that was long enough
        else if (slot == top) slot = (b & kWalkSecond) ? top : top - 1;
        else slot = slot - 1;
        lab = b & 0x1f;
        col[t - 1] = static_cast<int8_t>(lab);
    }
}

// The backward walk of the sum semiring and the marginals under the constraint.  The geometry of the forward
// kernel, transposed: a lane owns a SOURCE label i and keeps its row of trans; its column beta_t(i, d) lies in LDS as the forward
// column does, and beside it one double per lane, the state score of the gene the column belongs to, so that a source reads
// state_{t+1}[k] of every successor label from LDS.  The successors of a source at gene t, from the table at the head of the file:
//   i outside S             every k outside S, and (k, 1) for k in S (slot 0; at m = 1 that is the one state of k)
//   (i, d), d < m           (k, d + 1), k in S
//   (i, m)                  (k, m), k in S, and every k outside S -- all of them at slot m - 1
// beta_{T-1} = 0 at the admissible states (slot m - 1 of every label), -infinity elsewhere;
// beta_t(s) = LSE over successors s' of (trans[i][k] + state_{t+1}[k]) + beta_{t+1}(s'), max-shifted, -infinity when every
// term is.  The groups of a wave start at their contigs' last genes, so step u is gene T - 2 - u of each; a group that has reached
// gene 0 stores nothing more.  State scores come eight steps ahead.  One barrier per step, outside every divergent branch.
//   As it goes: marg[g][i] = sum over the lane's slots, ascending, of exp((alpha + beta) - log Z_C) with alpha from the forward
// launch's workspace and log Z_C its output; inside[g] = the group's sum of marg over the labels of S (crf_lanes.hpp's butterfly:
// one order of additions).  A state that no feasible path visits adds exactly 0.0, and so does every state of a contig without a
// feasible path.  No atomics.
template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_minrun_backward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                 const int32_t *__restrict__ contig_ptr, const int L,
                                                                 const int n_contigs, const int m, const uint32_t set_mask,
                                                                 const double *__restrict__ fwd, const double *__restrict__ lognorm_c,
                                                                 double *__restrict__ marg, double *__restrict__ inside_out) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][m | 1] beta, then [2][kWalkLanes] state scores
    const double ninf = kWalkNinf;
    const int top = m - 1;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, i = g.j, ii = g.jj, T = g.T;
    const bool on = g.on;
    const bool inside = (set_mask >> i) & 1u;
    const double lz = g.valid ? lognorm_c[g.c] : ninf;
    const bool feasible = lz > ninf;
    double trow[LP];
    g.template load_trans<true>(trans, L, trow);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, m);
    const int KS = cols.KS;
    double *const sb0 = cols_lds + 2 * kWalkLanes * KS, *const sb1 = sb0 + kWalkLanes;
    // the state score of the gene u steps before the last one
    const auto fetch = [&](int u) { return g.state_at(st, L, u < T, T - 1 - u); };
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
        cols.fill(lane, on ? top : -1, 0.0);
        sb0[lane] = fetch(0);
        sb1[lane] = ninf;
        double p = 0.0;
        if (T > 0 && on) {  // the last gene: beta is 0 at the one admissible state of the label
            const double a = fwd[((static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)) * L + ii) * static_cast<size_t>(m) + top];
            p = (feasible && a > ninf) ? exp(a - lz) : 0.0;
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
        double p = 0.0;
#pragma unroll 1
        for (int d = 0; d < m; ++d) {
            const bool last = d == top;  // (wave-uniform)
            const bool own = inside || last;
            const double a = (act && on && own) ? fwd[ak + d] : ninf;
            const int slot_in = last ? top : d + 1;
            const bool every = !inside || last;  // every label has a successor state; otherwise the labels of S only
            const auto successors = [&](auto &&f) {
#pragma unroll
                for (int k = 0; k < LP; ++k) {
                    const bool in_k = (set_mask >> k) & 1u;
                    const int slot = inside ? slot_in : (in_k ? 0 : top);
                    const double v = prev[k * KS + slot] + ts[k];
                    f(k, (every || in_k) ? v : ninf, false);
                }
            };
            const WalkSum r = walk_sum(successors);
            const double b = (on && r.finite) ? r.value : ninf;
            if (act && own) {
                mine[d] = b;
                const double ab = a + b;
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
void launch_forward(const GenArgs &a, uint32_t set_mask, int32_t m, uint8_t *back, int8_t *y, double *out, hipStream_t stream,
                    double *fwd = nullptr) {
    hipLaunchKernelGGL((gl_minrun_forward<LP, SUM, STORE>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(m), stream,
                       a.state, a.trans, a.contig_ptr, a.L, a.n_contigs, m, set_mask, back, y, out, fwd);
}

template <int LP>
void launch_backward(const GenArgs &a, uint32_t set_mask, int32_t m, const double *fwd, const double *lognorm_c, double *marg,
                     double *inside, hipStream_t stream) {
    const size_t lds = walk_lds_bytes(m) + size_t(2) * kWalkLanes * sizeof(double);  // (the columns, then the state scores)
    hipLaunchKernelGGL((gl_minrun_backward<LP>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), lds, stream, a.state, a.trans,
                       a.contig_ptr, a.L, a.n_contigs, m, set_mask, fwd, lognorm_c, marg, inside);
}

}  // namespace

size_t minrun_back_bytes(int64_t n_genes, int32_t L, int32_t min_run) {
    return static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(min_run);
}

hipError_t launch_gen_min_run(const GenArgs &a, uint32_t set_mask, int32_t min_run, uint8_t *back, int8_t *y, double *score,
                              double *lognorm_min_run, hipStream_t stream) {
    if (!walk_counter_ok(a, set_mask, min_run, kMaxMinRun)) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !back || !y || !score) return hipErrorNotSupported;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, false>(a, set_mask, min_run, back, y, score, stream); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(a.n_contigs) + kRBack - 1) / kRBack);
    hipLaunchKernelGGL(gl_minrun_backtrack, dim3(blocks), dim3(kRBack), 0, stream, back, a.contig_ptr, a.L, a.n_contigs, min_run, set_mask, y);
    e = hipGetLastError();
    if (e != hipSuccess || !lognorm_min_run) return e;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true>(a, set_mask, min_run, nullptr, nullptr, lognorm_min_run, stream); });
    return hipGetLastError();
}

size_t minrun_forward_bytes(int64_t n_genes, int32_t L, int32_t min_run) {
    return sizeof(double) * static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(min_run);
}

hipError_t launch_gen_min_run_marginals(const GenArgs &a, uint32_t set_mask, int32_t min_run, double *fwd, double *marg,
                                        double *inside, double *lognorm_min_run, hipStream_t stream) {
    if (!walk_counter_ok(a, set_mask, min_run, kMaxMinRun)) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !fwd || !lognorm_min_run || (!marg && !inside)) return hipErrorNotSupported;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true, true>(a, set_mask, min_run, nullptr, nullptr, lognorm_min_run, stream, fwd); });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    dispatch_lp(a.L, [&](auto lp) { launch_backward<lp>(a, set_mask, min_run, fwd, lognorm_min_run, marg, inside, stream); });
    return hipGetLastError();
}

}  // namespace gecco
