// Max-marginals of the whole-contig lattice: through[g][l] = the score of the best label path of gene g's contig
// that gives gene g the label l, the max-plus forward vector plus the max-plus backward vector, and what follows from the two
// stored vectors: the best path per gene inside / outside a label set, and per span query the best path that keeps a whole
// span inside a set and the best one that leaves it somewhere.  gl_state (crf_general.hip) leaves the raw state scores in
// GenArgs::state, -infinity at a disallowed (gene, label) pair; nothing else of the marginals' workspace is read.  Additions and
// comparisons only; the file is compiled without floating-point contraction, like crf_kbest.hip.
//
// With s_t the state scores of a contig of T genes and A the raw transition weights:
//   a_0(j) = s_0(j),   a_t(j) = max_i (a_{t-1}(i) + A(i, j)) + s_t(j)       -- gecco_crf_viterbi's operation order
//   b_{T-1}(i) = 0,    b_t(i) = max_j ((b_{t+1}(j) + s_{t+1}(j)) + A(i, j))
//   best = max_j a_{T-1}(j)  (the score bits of gl_kbest_forward's rank 0),   through_t(l) = a_t(l) + b_t(l), not clamped.
// A maximum is exact, so no scan order enters the bits; -infinity + finite = -infinity and +infinity never arises, so a value is
// -infinity exactly where no path exists and never NaN.
//
// gl_maxmarg_forward<LP>: the frame of crf_contig_walk.hpp (group geometry, columns in LDS, gene loop, group arg max), one lane
// per destination label with its column of trans in registers and ONE slot per lane in the two generations of columns; a strict
// `>` max and no back-pointers.  Stores a_t(.) to fwd [n_genes][L] and best[c] at the end, group_argmax's tie order.
// gl_maxmarg_backward<LP>: the same frame transposed, a lane owns a source label and keeps its row of trans (load_trans<true>).
// What a lane leaves in its slot is w_t(j) = b_t(j) + s_t(j), its own label's term of every source's maximum one gene earlier.
// The groups of a wave start at their contigs' last genes, so step u is gene T - 2 - u of each.  Stores b_t(.) to bwd.
// gl_maxmarg_epilogue<LP>: one group of lanes per gene, on the frame of crf_lane_group.hpp: through, and per label set the maxima
// over the lanes inside and outside it; only what was asked for is formed.
// gl_maxmarg_spans<LP>: one group per query, as gl_span_logp: v_begin = a_begin on the labels of the set, -infinity elsewhere,
// v_t(j) = max_i (v_{t-1}(i) + A(i, j)) + s_t(j) likewise (max_plus), span_best = max_j (v_{end-1}(j) + b_{end-1}(j)); in the same
// walk span_broken = the maximum of through over the span's genes and the labels outside the set.
// No atomics, no scratch; a contig is one sequential walk, and it is not chunked.
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kMT = 256;  // lanes per workgroup of the epilogue and of the span walks

template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_maxmarg_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                 const int32_t *__restrict__ contig_ptr, const int L,
                                                                 const int n_contigs, double *__restrict__ fwd,
                                                                 double *__restrict__ best) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][1]
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, 1);
    const int KS = cols.KS;
    double *const out = fwd + static_cast<size_t>(g.g0) * L + g.jj;
    {
        const double s0 = g.state_at(st, L, 0 < T, 0);
        cols.fill(lane, 0, s0);
        if (g.on && T > 0) out[0] = s0;
    }
    __syncthreads();  // (one wave)
    // one gene: the lane's maximum over the previous generation's column (a lane without a label holds -infinity there)
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double m = ninf;
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            const double v = prev[i * KS] + tcol[i];
            m = v > m ? v : m;
        }
        const double value = m + s_t;
        if (act) {
            cols.gen(t)[lane * KS] = value;
            if (g.on) out[static_cast<size_t>(t) * L] = value;
        }
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    double v = T > 0 ? cols.gen(T - 1)[lane * KS] : ninf;
    int bj = j;
    group_argmax<LP>(v, bj);
    // (a contig without genes: the score of gl_viterbi_seq's convention)
    if (g.valid && j == 0) best[g.c] = T > 0 ? v : 0.0;
}

template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_maxmarg_backward(const double *__restrict__ state, const double *__restrict__ trans,
                                                                  const int32_t *__restrict__ contig_ptr, const int L,
                                                                  const int n_contigs, double *__restrict__ bwd) {
    extern __shared__ __attribute__((aligned(16))) double cols_lds[];  // [2][kWalkLanes][1]: w = b + s of the generation's gene
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, T = g.T;
    double trow[LP];
    g.template load_trans<true>(trans, L, trow);
    const double *st = g.column(state, L);
    const WalkColumns cols(cols_lds, 1);
    const int KS = cols.KS;
    double *const out = bwd + static_cast<size_t>(g.g0) * L + g.jj;
    // the state score of the gene u steps before the last one
    const auto fetch = [&](int u) { return g.state_at(st, L, u < T, T - 1 - u); };
    {
        // the last gene: b = 0, so w is its state score (-infinity in a lane without a label, and without a gene)
        const double s_last = fetch(0);
        cols.fill(lane, 0, T > 0 ? 0.0 + s_last : ninf);
        if (g.on && T > 0) out[static_cast<size_t>(T - 1) * L] = 0.0;
    }
    __syncthreads();  // (one wave)
    const auto step = [&](const int u, const double s_t) {
        const int t = T - 2 - u;
        const bool act = t >= 0;
        const double *prev = cols.gen(u) + g.row0 * KS;
        double b = ninf;
#pragma unroll
        for (int k = 0; k < LP; ++k) {
            const double v = prev[k * KS] + trow[k];
            b = v > b ? v : b;
        }
        if (act) {
            cols.gen(u + 1)[lane * KS] = b + s_t;
            if (g.on) out[static_cast<size_t>(t) * L] = b;
        }
        __syncthreads();
    };
    contig_walk(0, T - 1, [&](int u) { return fetch(u + 1); }, step);
}

struct MaxMargSets {
    uint32_t mask[kMaxMargSets];
};

template <int LP>
__global__ void __launch_bounds__(kMT) gl_maxmarg_epilogue(const double *__restrict__ fwd, const double *__restrict__ bwd, const int L,
                                                           const int n_genes, const MaxMargSets sets, const int n_sets,
                                                           double *__restrict__ through, double *__restrict__ inside,
                                                           double *__restrict__ outside) {
    const LaneGroup<LP, kMT> g{};
    const int j = g.j;
    const long long gene = g.item;
    if (gene >= n_genes) return;  // (a whole group: the reductions below stay inside one)
    const double ninf = kWalkNinf;
    const bool on = j < L;
    const size_t at = static_cast<size_t>(gene) * L + (on ? j : 0);
    const double th = on ? fwd[at] + bwd[at] : ninf;
    if (through && on) through[at] = th;
    if (!inside && !outside) return;  // (wave-uniform)
    for (int s = 0; s < n_sets; ++s) {
        const bool in = (sets.mask[s] >> j) & 1u;  // (no bit at or above L)
        const double vi = group_max<LP>(in ? th : ninf), vo = group_max<LP>(in ? ninf : th);
        if (j == 0) {
            const size_t o = static_cast<size_t>(gene) * n_sets + s;
            if (inside) inside[o] = vi;
            if (outside) outside[o] = vo;
        }
    }
}

template <int LP>
__global__ void __launch_bounds__(kMT) gl_maxmarg_spans(const double *__restrict__ state, const double *__restrict__ trans,
                                                        const int32_t *__restrict__ contig_ptr, const int L,
                                                        const double *__restrict__ fwd, const double *__restrict__ bwd,
                                                        const SpanQuery *__restrict__ spans, const int n_spans,
                                                        double *__restrict__ span_best, double *__restrict__ span_broken) {
    __shared__ double vecs[kMT];
    const LaneGroup<LP, kMT> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const long long q = g.item;
    if (q >= n_spans) return;
    const SpanQuery s = spans[q];
    const int g0 = contig_ptr[s.contig];
    const int gb = g0 + s.begin, ge = g0 + s.end;
    const bool on = j < L, in = on && ((s.mask >> j) & 1u), out = on && !in;
    const int jj = on ? j : 0;
    const double ninf = kWalkNinf;
    double tcol[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) tcol[i] = (i < L && on) ? trans[i * L + j] : 0.0;
    const bool want_best = span_best != nullptr, want_broken = span_broken != nullptr;  // (wave-uniform)
    const size_t col = static_cast<size_t>(gb) * L + jj;
    const double *a = fwd + col, *b = bwd + col, *st = state + col;
    double v = in ? a[0] : ninf;
    double broken = (want_broken && out) ? a[0] + b[0] : ninf;
    for (int t = gb + 1; t < ge; ++t) {
        const size_t o = static_cast<size_t>(t - gb) * L;
        if (want_best) {
            const double m = max_plus(vec, j, v, tcol, L);
            v = in ? m + st[o] : ninf;
        }
        if (want_broken && out) {
            const double th = a[o] + b[o];
            broken = th > broken ? th : broken;
        }
    }
    if (want_best) {
        const double r = group_max<LP>(in ? v + b[static_cast<size_t>(ge - 1 - gb) * L] : ninf);
        if (j == 0) span_best[q] = r;
    }
    if (want_broken) {
        const double r = group_max<LP>(broken);
        if (j == 0) span_broken[q] = r;
    }
}

template <int LP>
void launch_walks(const GenArgs &a, double *fwd, double *bwd, double *best, hipStream_t stream) {
    hipLaunchKernelGGL(gl_maxmarg_forward<LP>, dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(1), stream, a.state,
                       a.trans, a.contig_ptr, a.L, a.n_contigs, fwd, best);
    hipLaunchKernelGGL(gl_maxmarg_backward<LP>, dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(1), stream, a.state,
                       a.trans, a.contig_ptr, a.L, a.n_contigs, bwd);
}

}  // namespace

size_t maxmarg_workspace_bytes(int64_t n_genes, int32_t L) {
    return size_t(2) * sizeof(double) * static_cast<size_t>(n_genes) * static_cast<size_t>(L);
}

hipError_t launch_gen_max_marginals(const GenArgs &a, const MaxMargArgs &p, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || p.n_sets < 0 || p.n_sets > kMaxMargSets || p.n_spans < 0) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !a.contig_ptr || !p.fwd || !p.bwd || !p.best) return hipErrorNotSupported;
    if ((p.inside || p.outside) && p.n_sets == 0) return hipErrorNotSupported;
    if (p.n_spans > 0 && !p.spans) return hipErrorNotSupported;
    dispatch_lp(a.L, [&](auto lp) { launch_walks<lp>(a, p.fwd, p.bwd, p.best, stream); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.n_genes > 0 && (p.through || p.inside || p.outside)) {
        MaxMargSets sets{};
        for (int32_t s = 0; s < p.n_sets; ++s) sets.mask[s] = p.set_mask[s];
        dispatch_lp(a.L, [&](auto lp) {
            hipLaunchKernelGGL(gl_maxmarg_epilogue<lp>, dim3(group_blocks(a.n_genes, LaneGroup<lp, kMT>::G)), dim3(kMT), 0, stream, p.fwd,
                               p.bwd, a.L, a.n_genes, sets, p.n_sets, p.through, p.inside, p.outside);
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (p.n_spans > 0 && (p.span_best || p.span_broken)) {
        dispatch_lp(a.L, [&](auto lp) {
            hipLaunchKernelGGL(gl_maxmarg_spans<lp>, dim3(group_blocks(p.n_spans, LaneGroup<lp, kMT>::G)), dim3(kMT), 0, stream, a.state,
                               a.trans, a.contig_ptr, a.L, p.fwd, p.bwd, p.spans, p.n_spans, p.span_best, p.span_broken);
        });
        e = hipGetLastError();
    }
    return e;
}

}  // namespace gecco
