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
// gl_minrun_forward<LP, SUM>: a group of LP = next-pow2(L) lanes per contig, one lane per destination label, 64 / LP contigs per
// wave (a workgroup is one wave); lanes of labels that do not exist carry -infinity.  A lane's d-column lies in LDS, two
// generations, [2][64 rows][m | 1] doubles: state (j, d) at slot d - 1, an outside label's one state at slot m - 1 -- so every
// state a run may end in, and every admissible one, is at slot m - 1.  The row length is odd, so that lanes reading different
// rows at one slot hit different banks.  The lane's column of trans is in registers, indexed by unrolled loops only.  State
// scores come eight genes ahead, as in gl_viterbi_wave.  The groups of a wave end at different genes; a group that has ended
// keeps its values and stores nothing.  One barrier per gene, outside every divergent branch.
//   Back-pointers (max only): one byte per (gene, label, slot), the source label in the low five bits and one bit "from d = m"
// (as against m - 1), which means something at d = m only.  The final arg max runs across the group's lanes by xor-shuffles, the
// smaller label winning a tie (one admissible state per label), and leaves the last gene's label in y, or -1.
//   SUM is the second instantiation of the same body: no back-pointers, log Z_C instead of the score.
// gl_minrun_backtrack: one lane per contig, last gene to first; the previous slot follows from the rule above.
// A contig is one sequential walk; it is not chunked.
#include "crf_device.hpp"
#include "crf_lanes.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kRW = 64;      // lanes per workgroup of the forward kernel: one wave
constexpr int kRTile = 8;    // genes of state scores fetched ahead
constexpr int kRBack = 256;  // lanes per workgroup of the backtrack
constexpr uint8_t kFromFull = 0x20;  // back-pointer bit: the source was (i, m), not (i, m - 1)

template <int LP, bool SUM>
__global__ void __launch_bounds__(kRW) gl_minrun_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                         const int32_t *__restrict__ contig_ptr, const int L, const int n_contigs,
                                                         const int m, const uint32_t set_mask, uint8_t *__restrict__ back,
                                                         int8_t *__restrict__ y, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double cols[];  // [2][kRW][KS]
    constexpr int G = kRW / LP;
    const double ninf = -INFINITY;
    const int KS = m | 1, top = m - 1;
    const int lane = threadIdx.x, j = lane & (LP - 1), row0 = lane - j;
    const long long c = static_cast<long long>(blockIdx.x) * G + lane / LP;
    const bool valid = c < n_contigs;
    int g0 = 0, T = 0;
    if (valid) {
        g0 = contig_ptr[c];
        T = contig_ptr[c + 1] - g0;
        T = T < 0 ? 0 : T;
    }
    const bool on = j < L;
    const int jj = on ? j : 0;
    const bool inside = (set_mask >> j) & 1u;  // (no bit at or above L: a lane without a label is an outside lane at -infinity)
    double tcol[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) tcol[i] = i < L ? trans[i * L + jj] : 0.0;
    double *const buf0 = cols, *const buf1 = cols + kRW * KS;
    const double *st = state + static_cast<size_t>(g0) * L + jj;
    const auto fetch = [&](int t) { return t < T ? (on ? st[static_cast<size_t>(t) * L] : ninf) : 0.0; };
    {
        const double s0 = fetch(0);
        const int first = inside ? 0 : top;
        for (int k = 0; k < KS; ++k) {
            buf0[lane * KS + k] = k == first ? s0 : ninf;
            buf1[lane * KS + k] = ninf;
        }
    }
    __syncthreads();  // (one wave)
    // one gene: the lane's states in slot order.  An outside lane has its one state at the last slot and idles before it.
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = ((t & 1) ? buf0 : buf1) + row0 * KS;
        double *mine = ((t & 1) ? buf1 : buf0) + lane * KS;
        const size_t bk = (static_cast<size_t>(g0 + (act ? t : 0)) * L + jj) * static_cast<size_t>(m);
#pragma unroll 1
        for (int d = 0; d < m; ++d) {
            const bool last = d == top;  // (wave-uniform)
            // where this destination's sources lie: the labels (`from`), their slot, and at d = m a second slot behind it
            const bool plain = !inside || m == 1;
            const uint32_t from = plain ? ~0u : (d == 0 ? ~set_mask : set_mask);
            const bool two = !plain && last;
            const int slot = plain || d == 0 ? top : (two ? top - 1 : d - 1);
            // f(i, value, from_full) for every source in ascending (label, d) order; a label that is no source gives -infinity
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
            double value;
            int arg = 0;
            if constexpr (SUM) {
                double mx = ninf;
                sources([&](int, double v, bool) { mx = v > mx ? v : mx; });
                const double shift = mx > ninf ? mx : 0.0;
                double sum = 0.0;
                sources([&](int, double v, bool) { sum += v > ninf ? exp(v - shift) : 0.0; });
                value = mx > ninf ? (mx + log(sum)) + s_t : ninf;
            } else {
                double best = ninf;
                sources([&](int i, double v, bool full) {
                    const bool take = v > best;  // strict: the earlier source wins a tie
                    best = take ? v : best;
                    arg = take ? (i | (full ? kFromFull : 0)) : arg;
                });
                value = best + s_t;
            }
            if (act && (inside || last)) {
                mine[d] = value;
                if constexpr (!SUM) {
                    if (on) back[bk + d] = static_cast<uint8_t>(arg);
                }
            }
        }
        __syncthreads();
    };
    double nxt[kRTile];
#pragma unroll
    for (int k = 0; k < kRTile; ++k) nxt[k] = fetch(1 + k);
    for (int tb = 1; __any(tb < T); tb += kRTile) {
        double cur[kRTile];
#pragma unroll
        for (int k = 0; k < kRTile; ++k) cur[k] = nxt[k];
#pragma unroll
        for (int k = 0; k < kRTile; ++k) nxt[k] = fetch(tb + kRTile + k);
#pragma unroll
        for (int k = 0; k < kRTile; ++k) {
            if (!__any(tb + k < T)) break;  // (wave-uniform)
            step(tb + k, cur[k]);
        }
    }
    // the end of the contig: every lane its label's admissible state, which is the last slot of its column
    const double *fl = (((T - 1) & 1) ? buf1 : buf0) + lane * KS;
    double v = T > 0 ? fl[top] : ninf;
    if constexpr (SUM) {
        const double mx = group_max<LP>(v);
        const double shift = mx > ninf ? mx : 0.0;
        const double sum = group_sum<LP>(v > ninf ? exp(v - shift) : 0.0);
        if (valid && j == 0) out[c] = T > 0 ? (mx > ninf ? mx + log(sum) : ninf) : 0.0;
    } else {
        int bj = j;
#pragma unroll
        for (int off = LP / 2; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(v, off);
            const int oj = __shfl_xor(bj, off);
            const bool take = ov > v || (ov == v && oj < bj);
            v = take ? ov : v;
            bj = take ? oj : bj;
        }
        if (valid && j == 0) {
            // (a contig without genes: the score of gl_viterbi_seq's convention)
            out[c] = T > 0 ? v : 0.0;
            if (T > 0) y[static_cast<size_t>(g0) + static_cast<size_t>(T - 1)] = v > ninf ? static_cast<int8_t>(bj) : int8_t(-1);
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
        else if (slot == top) slot = (b & kFromFull) ? top : top - 1;
        else slot = slot - 1;
        lab = b & 0x1f;
        col[t - 1] = static_cast<int8_t>(lab);
    }
}

template <int LP, bool SUM>
void launch_forward(const GenArgs &a, uint32_t set_mask, int32_t m, uint8_t *back, int8_t *y, double *out, hipStream_t stream) {
    constexpr int G = kRW / LP;
    const unsigned blocks = static_cast<unsigned>((static_cast<long long>(a.n_contigs) + G - 1) / G);
    const size_t lds = size_t(2) * kRW * size_t(m | 1) * sizeof(double);
    hipLaunchKernelGGL((gl_minrun_forward<LP, SUM>), dim3(blocks), dim3(kRW), lds, stream, a.state, a.trans, a.contig_ptr, a.L,
                       a.n_contigs, m, set_mask, back, y, out);
}

}  // namespace

size_t minrun_back_bytes(int64_t n_genes, int32_t L, int32_t min_run) {
    return static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(min_run);
}

hipError_t launch_gen_min_run(const GenArgs &a, uint32_t set_mask, int32_t min_run, uint8_t *back, int8_t *y, double *score,
                              double *lognorm_min_run, hipStream_t stream) {
    const uint32_t beyond = a.L >= 32 ? 0u : ~0u << a.L;
    if (a.L <= 0 || a.L > kGenMaxL || min_run < 1 || min_run > kMaxMinRun || set_mask == 0 || (set_mask & beyond))
        return hipErrorNotSupported;
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

}  // namespace gecco
