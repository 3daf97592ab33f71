// How many runs a contig holds: for a label set S and K = max_runs, 1 <= K <= 32, the log-mass of the paths with exactly k runs
// of labels of S, k = 0 .. K - 1, and of those with at least K (the saturating tail slot k = K), and the best path of each of
// the K + 1 classes with its score.  A run is a maximal stretch of consecutive genes with labels in S; runs at a
// contig's first or last gene count like any other, and the labels inside a run may differ (crf_minrun.hip's notion).
// gl_state (crf_general.hip) leaves the raw state scores in GenArgs::state, -infinity at a disallowed (gene, label) pair; nothing
// else of the marginals' workspace is read.  The file is compiled without floating-point contraction, like crf_minrun.hip.
//
// The recursion runs on the lattice expanded by a run counter c = min(runs begun up to and including this gene, K).  A label
// outside S has the states (j, c), c = 0 .. K; a label inside S has (j, c), c = 1 .. K; states are ordered by label, then by c.
// At gene 0 (j outside, 0) and (j inside, 1) start at state_0[j], the others at -infinity.  The sources of a destination at gene t:
//   (j, c), j outside S     (i, c) for every label i (no run begins)
//   (j, c), j inside S      (i, c) for i inside S (the run goes on); (i, c - 1) for i outside S (a run begins);
//                           at c = K also (i, K) for i outside S (a run begins beyond the K-th: the counter saturates)
// At a contig's end every state is admissible, and slot k collects the states (., k) of every label.
//   Max semiring: value = (delta[source] + trans[i][j]) + state_t[j], the operation order of the other Viterbi recursions, so a
// path's score is its left-to-right sum.  Sources are scanned in ascending (label, c) order with a strict `>` update, and at the
// end the smaller label wins a tie.  That is an operational tie rule on expanded states, not an order on paths (at the tail
// slot two expanded states may stand for one label).  A class without a path (k > ceil(T / 2), k = 0 with S every label,
// masks): score -infinity, label -1 at every gene of its plane, log-mass -infinity; never NaN.
//   Sum semiring: the same sources, a max-shifted log-sum-exp in place of the max; a destination all of whose sources are
// -infinity stays -infinity.
//
// gl_counts_forward<LP, SUM>: the frame of crf_contig_walk.hpp (group geometry, columns in LDS, gene loop, the two reducers over
// sources(f), the end-of-contig reductions), one lane per destination label.  A lane's counter column, [(K + 1) | 1] doubles:
// state (j, c) at slot c (slot 0 of an inside label stays -infinity).
//   Back-pointers (max only): one byte per (gene, label, slot), the source label in the low five bits and one bit "the source
// slot was K" (as against K - 1), which means something only at slot K of an inside label reached from an outside label;
// everywhere else the source slot follows from the two labels.  The final arg max of every slot runs across the group's lanes by
// xor-shuffles and leaves the last gene's label in plane k of y, or -1.
// gl_counts_backtrack: one lane per (contig, k), last gene to first, plane k of y [K + 1][n_genes].
// A contig is one sequential walk; it is not chunked.  No atomics: equal calls give equal bytes.
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kCBack = kWalkBack;  // lanes per workgroup of the backtrack

template <int LP, bool SUM>
__global__ void __launch_bounds__(kWalkLanes) gl_counts_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                const int32_t *__restrict__ contig_ptr, const int L,
                                                                const int n_contigs, const long long n_genes, const int K,
                                                                const uint32_t set_mask, uint8_t *__restrict__ back,
                                                                int8_t *__restrict__ y, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][(K + 1) | 1]
    const double ninf = kWalkNinf;
    const int K1 = K + 1;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    const bool inside = (set_mask >> j) & 1u;  // (no bit at or above L: a lane without a label is an outside lane at -infinity)
    // the labels whose state one slot below is this lane's source: the outside labels, for an inside lane
    const uint32_t below = inside ? ~set_mask : 0u;
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, K1);
    const int KS = cols.KS;
    cols.fill(lane, inside ? 1 : 0, g.state_at(st, L, 0 < T, 0));
    __syncthreads();  // (one wave)
    // one gene: the lane's states in slot order.  An inside lane has no state at slot 0 and idles there.
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double *mine = cols.gen(t) + lane * KS;
        const size_t bk = (static_cast<size_t>(g.g0 + (act ? t : 0)) * L + g.jj) * static_cast<size_t>(K1);
#pragma unroll 1
        for (int k = 0; k < K1; ++k) {
            const bool tail = k == K;          // (wave-uniform)
            const bool own = !inside || k > 0;  // the lane has a state at this slot
            const uint32_t dec = k > 0 ? below : 0u;
            const auto sources = [&](auto &&f) {
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    const int lower = (dec >> i) & 1u;
                    const double v = prev[i * KS + k - lower] + tcol[i];
                    f(i, own ? v : ninf, false);
                    if (tail) {  // (wave-uniform: an outside label's state at the tail slot too, for an inside lane)
                        const double w = prev[i * KS + K] + tcol[i];
                        f(i, lower ? w : ninf, true);
                    }
                }
            };
            int arg;
            const double value = walk_value<SUM>(sources, s_t, arg);
            if (act && own) {
                mine[k] = value;
                if constexpr (!SUM) {
                    if (g.on) back[bk + k] = static_cast<uint8_t>(arg);
                }
            }
        }
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the end of the contig: slot k collects the states (., k) of the group's lanes
    const double *fl = cols.gen(T - 1) + lane * KS;
    const size_t ob = static_cast<size_t>(g.valid ? g.c : 0) * static_cast<size_t>(K1);
#pragma unroll 1
    for (int k = 0; k < K1; ++k) {
        double v = T > 0 ? fl[k] : ninf;
        const double none = k == 0 ? 0.0 : ninf;  // (a contig without genes: the empty path, which has no run)
        if constexpr (SUM) {
            const double lse = group_lse<LP>(v);
            if (g.valid && j == 0) out[ob + k] = T > 0 ? lse : none;
        } else {
            int bj = j;
            group_argmax<LP>(v, bj);
            if (g.valid && j == 0) {
                out[ob + k] = T > 0 ? v : none;  // (without genes: the score of gl_viterbi_seq's convention, in the slot of no run)
                if (T > 0)
                    y[static_cast<size_t>(k) * static_cast<size_t>(n_genes) + static_cast<size_t>(g.g0) + static_cast<size_t>(T - 1)] =
                        v > ninf ? static_cast<int8_t>(bj) : int8_t(-1);
            }
        }
    }
}

__global__ void __launch_bounds__(kCBack) gl_counts_backtrack(const uint8_t *__restrict__ back, const int32_t *__restrict__ contig_ptr,
                                                              const int L, const int n_contigs, const long long n_genes, const int K,
                                                              const uint32_t set_mask, int8_t *__restrict__ y) {
    const size_t K1 = static_cast<size_t>(K) + 1;
    const size_t idx = static_cast<size_t>(blockIdx.x) * kCBack + threadIdx.x;
    if (idx >= static_cast<size_t>(n_contigs) * K1) return;
    const size_t c = idx / K1;
    const int k = static_cast<int>(idx % K1);
    const int g0 = contig_ptr[c], T = contig_ptr[c + 1] - g0;
    if (T <= 0) return;
    int8_t *col = y + static_cast<size_t>(k) * static_cast<size_t>(n_genes) + static_cast<size_t>(g0);
    int lab = col[T - 1];  // (the forward kernel's, earlier on the stream)
    if (lab < 0) {
        for (int t = 0; t < T; ++t) col[t] = -1;
        return;
    }
    int slot = k;
    for (int t = T - 1; t >= 1; --t) {
        if (lab >= L || slot < 0 || slot > K) {  // (cannot happen: a finite state points at a finite state; no address leaves the workspace)
            lab = 0;
            slot = K;
        }
        const uint8_t b = back[(static_cast<size_t>(g0 + t) * L + lab) * K1 + static_cast<size_t>(slot)];
        const int src = b & 0x1f;
        const bool inside = (set_mask >> lab) & 1u, src_inside = (set_mask >> src) & 1u;
        // a run began at this gene: the source is one slot below, or at the tail slot itself when the bit says so
        if (inside && !src_inside && !(slot == K && (b & kWalkSecond))) slot -= 1;
        lab = src;
        col[t - 1] = static_cast<int8_t>(lab);
    }
}

template <int LP, bool SUM>
void launch_forward(const GenArgs &a, uint32_t set_mask, int32_t K, uint8_t *back, int8_t *y, double *out, hipStream_t stream) {
    hipLaunchKernelGGL((gl_counts_forward<LP, SUM>), dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(K + 1), stream,
                       a.state, a.trans, a.contig_ptr, a.L, a.n_contigs, static_cast<long long>(a.n_genes), K, set_mask, back, y, out);
}

}  // namespace

size_t counts_back_bytes(int64_t n_genes, int32_t L, int32_t max_runs) {
    return static_cast<size_t>(n_genes) * static_cast<size_t>(L) * (static_cast<size_t>(max_runs) + 1);
}

hipError_t launch_gen_run_counts(const GenArgs &a, uint32_t set_mask, int32_t max_runs, uint8_t *back, double *log_mass,
                                 double *score, int8_t *y, hipStream_t stream) {
    if (!walk_counter_ok(a, set_mask, max_runs, kMaxRunCounts)) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || (!log_mass && !score) || (score && (!back || !y))) return hipErrorNotSupported;
    if (log_mass) {
        dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, true>(a, set_mask, max_runs, nullptr, nullptr, log_mass, stream); });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!score) return hipSuccess;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp, false>(a, set_mask, max_runs, back, y, score, stream); });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lanes = static_cast<size_t>(a.n_contigs) * (static_cast<size_t>(max_runs) + 1);
    const unsigned blocks = static_cast<unsigned>((lanes + kCBack - 1) / kCBack);
    hipLaunchKernelGGL(gl_counts_backtrack, dim3(blocks), dim3(kCBack), 0, stream, back, a.contig_ptr, a.L, a.n_contigs,
                       static_cast<long long>(a.n_genes), max_runs, set_mask, y);
    return hipGetLastError();
}

}  // namespace gecco
