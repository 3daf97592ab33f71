// Marginals given a region, and the exact knock-out attributions of a call.  Query q is a span [begin, end)
// of a contig with a label set S; E is the event "every gene of the span carries a label of S".  Its rows are the genes
// lo = max(begin - reach, 0) .. hi = min(end + reach, T) of the contig, and row t holds c_t(l) = P(y_t = l | E, x).  Any number
// of queries behind ONE forward-backward pass of the batch (gl_state + any arrangement of the marginals recursion,
// crf_general.hip), which leaves the raw state scores, E, alpha and the marginals in the plan's workspace.
//
// Layout: one group of lanes per walk, on the frame of crf_lane_group.hpp.  A RIGHT walk multiplies by the columns of
// exp(trans), a LEFT walk by its rows: the kernel is templated on the direction and a lane holds the one it needs.  A query is
// two walks in two launches.  Each keeps, for every gene it visits, the vector that reaches the gene from its side BEFORE the
// gene's own emission:
//   right: p = alpha[begin - 1] . M (ones at the contig's first gene); over [begin, end) the recursion restricted to S, its
//     entering vectors kept in the query's workspace, (end - begin) L doubles; then free over [end, hi), kept in the rows;
//   left: b = M . (E marg / alpha)[end] (ones at the contig's end; E marg / alpha is the direction of psi beta, 0 where alpha is
//     0: crf_spans.hip's leaving vector); over [begin, end) backwards the recursion restricted to S, then free down to lo, b
//     kept in the rows.
// Inside the span both walks take the RAW state scores shifted by their maximum over the labels of S, so that a label outside S
// that leads by hundreds does not flush the set's emissions to zero (§4.9f/g); outside it they take gl_state's E.  Every vector
// is scaled at every step by the power of two that brings its sum into [1/2, 1): exact, and no logarithm is accumulated.  This
// file is compiled without floating-point contraction; fma() is explicit.
//
// The epilogue, gl_cond_rows, one group of lanes per (query, row), puts a row together.  With p and b the two vectors that
// reach gene t on the restricted lattice (one from a walk, the other from a walk or -- on the far side of the span -- the free
// one, alpha[t - 1] . M or M . (E marg / alpha)[t + 1]), u(l) = p(l) b(l) is the mass of the restricted paths through (t, l)
// short of the gene's own emission, and
//   c_t(l) = u(l) e^{s_t(l) - A} / sum_k u(k) e^{s_t(k) - A},   A the largest score among the labels that take part.
// The sum is Z_E in the units of the two vectors, at every gene: dividing by it is exact as a normalisation and every scale
// cancels -- the factor of the stored alpha (a direction only), the shifts, the powers of two.  The same with the two free
// vectors gives the gene's unconditional row.  Changing the state scores of ONE gene by delta_l multiplies Z by
// sum_l marg_t(l) e^{delta_l} and Z_E by sum_l c_t(l) e^{delta_l}; with the rows written as above that is
//   log P(E | x) - log P(E | x with the change) = [lse_l(log u(l) + s(l) + delta(l)) - lse_l(log u(l) + s(l))]  (free)
//                                                 - [the same]                                               (restricted),
// every log-sum-exp shifted by its own maximum -- so a label that leads by 800 at the gene, under which every other label's
// marginal is below the smallest double, still gives the exact amount when the lead is taken away.  delta_l = -v w[a][l] for
// every attribute occurrence of the gene in CSR order, delta_l = -s_t(l) for the gene as a whole.  A disallowed label
// (state -infinity), a label outside S inside the span, and a label no path reaches take no part.
// A row is one fixed operation sequence: the walks go away from the span, so what they keep at gene t depends on the genes
// between it and the span only -- not on reach, nor on the other queries, nor on the query's place in the batch.  A query whose
// span is impossible (crf_spans.hip wrote -infinity, which every kernel here reads first), and a row without mass, keep the
// zeros the launcher has filled the outputs with; never NaN.  No atomics, no scratch.
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kCT = 256;  // lanes per workgroup

// x scaled by the power of two that brings the positive sum s into [1/2, 1)
__device__ __forceinline__ double to_unit_sum(double x, double s) {
    int e;
    (void)__builtin_frexp(s, &e);
    return ldexp(x, -e);
}
// a vector's component scaled likewise; false when the vector carries no mass (or more than a double holds)
template <int LP>
__device__ __forceinline__ bool unit_sum(double &x) {
    const double sum = group_sum<LP>(x);
    if (!(sum > 0.0) || !(sum <= DBL_MAX)) return false;
    x = to_unit_sum(x, sum);
    return true;
}
// The lane's row or column m of exp(trans), times one power of two for the whole group: 2^-k, k the binary exponent of the
// table's largest entry rounded towards zero to a multiple of 256.  A model whose largest transition weight is +-600 has its
// table around 2^+-866, a walk keeps the vector that LEFT the product with it, and gl_cond_rows multiplies two of those: the
// product left the doubles' range and every row of such a model came out 0.  A factor common to the whole table multiplies
// every vector of both walks alike and cancels in a row, which is a ratio, and a power of two is exact.
// k = 0, and not one bit changes, while the largest weight stays inside +-177 = +-256 ln 2.
template <int LP>
__device__ __forceinline__ void table_to_range(double (&m)[LP]) {
    double top = 0.0;
#pragma unroll
    for (int i = 0; i < LP; ++i) top = fmax(top, m[i]);
    top = group_max<LP>(top);
    int e;
    (void)__builtin_frexp(top, &e);
    const int k = e / 256 * 256;  // (towards zero)
    if (k == 0) return;
#pragma unroll
    for (int i = 0; i < LP; ++i) m[i] = ldexp(m[i], -k);
}
// the direction of psi beta at a gene: E marg / alpha, 0 where alpha is 0
__device__ __forceinline__ double psi_beta(const GenArgs &a, size_t at) {
    const double al = a.alpha[at];
    return al != 0.0 ? a.E[at] * a.marg[at] / al : 0.0;
}

template <int LP, bool RIGHT>
__global__ void __launch_bounds__(kCT) gl_cond_walk(GenArgs a, ConditionalArgs p) {
    __shared__ double vecs[kCT];
    const LaneGroup<LP, kCT> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const long long q = g.item;
    if (q >= p.n_spans) return;
    const double ninf = -__builtin_huge_val();
    if (!(p.logp[q] > ninf)) return;  // an impossible span: its rows stay 0
    const SpanQuery s = p.spans[q];
    const int L = a.L;
    const int g0 = a.contig_ptr[s.contig], g1 = a.contig_ptr[s.contig + 1];
    const int gb = g0 + s.begin, ge = g0 + s.end;
    const int lo = g0 + max(s.begin - p.reach, 0);
    const int hi = static_cast<int>(min(static_cast<long long>(ge) + p.reach, static_cast<long long>(g1)));
    const bool on = j < L, in = on && ((s.mask >> j) & 1u);
    const int jj = on ? j : 0;
    // the lane's column (right) or row (left) of exp(trans)
    double mvec[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) mvec[i] = (i < L && on) ? (RIGHT ? a.exp_trans[i * L + j] : a.exp_trans[j * L + i]) : 0.0;
    table_to_range(mvec);  // (every vector of both walks carries the factor: it cancels in a row)
    double *fwd = p.fwd + static_cast<size_t>(p.fwd_ptr[q]) * L;    // the restricted forward vector entering gene t at fwd[(t - gb) L + j]
    double *rows = p.walk + static_cast<size_t>(p.row_ptr[q]) * L;  // the walk's vector at gene t at rows[(t - lo) L + j]

    if (RIGHT) {
        double pv = on ? 1.0 : 0.0;
        if (gb > g0) {
            pv = sum_product(vec, j, on ? a.alpha[static_cast<size_t>(gb - 1) * L + jj] : 0.0, mvec);
            if (!unit_sum<LP>(pv)) return;
        }
        for (int t = gb; t < hi; ++t) {
            const size_t at = static_cast<size_t>(t) * L + jj;
            const bool inside = t < ge;
            if (on) (inside ? fwd[static_cast<size_t>(t - gb) * L + j] : rows[static_cast<size_t>(t - lo) * L + j]) = pv;
            if (t + 1 == hi) return;
            double e;  // the emission of gene t: restricted to S and shifted by the set's maximum inside the span
            if (inside) {
                const double st = in ? a.state[at] : ninf;
                const double mm = group_max<LP>(st);
                e = in ? exp(st - mm) : 0.0;  // (no label of the set allowed here: NaN, which ends the walk below)
            } else {
                e = on ? a.E[at] : 0.0;
            }
            double x = pv * e;
            if (!unit_sum<LP>(x)) return;
            pv = sum_product(vec, j, x, mvec);
        }
    } else {
        double b = on ? 1.0 : 0.0;
        if (ge < g1) {
            b = sum_product<true>(vec, j, on ? psi_beta(a, static_cast<size_t>(ge) * L + jj) : 0.0, mvec);
            if (!unit_sum<LP>(b)) return;
        }
        for (int t = ge - 1; t >= lo; --t) {
            const size_t at = static_cast<size_t>(t) * L + jj;
            if (on) rows[static_cast<size_t>(t - lo) * L + j] = b;
            if (t == lo) return;
            double e;
            if (t >= gb) {
                const double st = in ? a.state[at] : ninf;
                const double mm = group_max<LP>(st);
                e = in ? exp(st - mm) : 0.0;
            } else {
                e = on ? a.E[at] : 0.0;
            }
            double x = e * b;
            if (!unit_sum<LP>(x)) return;
            b = sum_product<true>(vec, j, x, mvec);
        }
    }
}

// One side of the identity at one gene: u(l) the mass through (gene, l) short of the gene's emission, s(l) its state score;
// the labels with u > 0 and a finite score take part.
template <int LP>
struct Side {
    double u, s, top, sum;  // top = the largest s among the labels that take part, sum = sum_l u(l) e^{s(l) - top}
    bool part, any;
    __device__ __forceinline__ Side(double u_, double s_) : u(u_), s(s_) {
        const double ninf = -__builtin_huge_val();
        part = u > 0.0 && s > ninf;
        top = group_max<LP>(part ? s : ninf);
        any = top > ninf;
        sum = group_sum<LP>(part ? u * exp(s - top) : 0.0);
        any = any && sum > 0.0 && sum <= DBL_MAX;
    }
    // the label's probability at the gene
    __device__ __forceinline__ double row() const { return part ? u * exp(s - top) / sum : 0.0; }
    // lse_l(log u + s + d) - lse_l(log u + s); `flat`: s + d is 0 at every label (the gene's scores taken out)
    __device__ __forceinline__ double change(double d, bool flat) const {
        const double ninf = -__builtin_huge_val();
        const double sd = flat ? 0.0 : s + d;
        const double t1 = group_max<LP>(part ? sd : ninf);
        const double s1 = group_sum<LP>(part ? u * exp(sd - t1) : 0.0);
        return (t1 - top) + (log(s1) - log(sum));
    }
};

// one group per (query, row): the conditional marginals of the row's gene, its contribution as a whole and that of each of its
// attribute occurrences
template <int LP>
__global__ void __launch_bounds__(kCT) gl_cond_rows(GenArgs a, ConditionalArgs p) {
    __shared__ double vecs[kCT];
    const LaneGroup<LP, kCT> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const long long row = g.item;
    if (row >= p.n_rows) return;
    // the row's query: the last q with row_ptr[q] <= row
    int q = 0, top = p.n_spans;
    while (top - q > 1) {
        const int mid = q + (top - q) / 2;
        if (p.row_ptr[mid] <= row) q = mid;
        else top = mid;
    }
    const double ninf = -__builtin_huge_val();
    if (!(p.logp[q] > ninf)) return;  // an impossible span: zeros throughout
    const SpanQuery s = p.spans[q];
    const int L = a.L;
    const bool on = j < L, in = on && ((s.mask >> j) & 1u);
    const int jj = on ? j : 0;
    const int g0 = a.contig_ptr[s.contig], g1 = a.contig_ptr[s.contig + 1];
    const int gb = g0 + s.begin, ge = g0 + s.end;
    const int t = g0 + max(s.begin - p.reach, 0) + static_cast<int>(row - p.row_ptr[q]);
    const size_t at = static_cast<size_t>(t) * L + jj;
    // the two free vectors that reach the gene: alpha[t - 1] . M and M . (E marg / alpha)[t + 1], each brought to a unit sum
    // (the table is read from memory: two products a row, not a walk)
    double pf = on ? 1.0 : 0.0, bf = pf;
    if (t > g0) {
        const double *al = a.alpha + static_cast<size_t>(t - 1) * L;
        double acc = 0.0;
        for (int i = 0; i < L; ++i) acc = fma(al[i], a.exp_trans[i * L + jj], acc);
        pf = on ? acc : 0.0;
        if (!unit_sum<LP>(pf)) return;
    }
    if (t + 1 < g1) {
        vec[j] = on ? psi_beta(a, static_cast<size_t>(t + 1) * L + jj) : 0.0;
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        for (int k = 0; k < L; ++k) acc = fma(a.exp_trans[jj * L + k], vec[k], acc);
        __builtin_amdgcn_wave_barrier();
        bf = on ? acc : 0.0;
        if (!unit_sum<LP>(bf)) return;
    }
    const double st = on ? a.state[at] : ninf;
    const double wv = on ? p.walk[static_cast<size_t>(row) * L + jj] : 0.0;
    double uc;  // the restricted lattice: the walk's vector, and the other side's -- a walk's inside the span, else the free one
    if (t < gb) uc = pf * wv;
    else if (t < ge) uc = in ? p.fwd[(static_cast<size_t>(p.fwd_ptr[q]) + (t - gb)) * L + jj] * wv : 0.0;
    else uc = wv * bf;
    const Side<LP> free(pf * bf, st), cond(uc, st);
    if (!free.any || !cond.any) return;
    if (on) p.cond[static_cast<size_t>(row) * L + j] = cond.row();
    const double whole = free.change(0.0, true) - cond.change(0.0, true);
    if (j == 0) p.item[row] = whole;
    if (!p.occ_ptr) return;
    double *out = p.attr + p.occ_ptr[row];
    const int k0 = a.gene_ptr[t], k1 = a.gene_ptr[t + 1];
    for (int k = k0; k < k1; ++k) {
        const int id = a.attr_id[k];
        double r = 0.0;  // (an id outside the model's dictionary has no weight: gl_state)
        if (unsigned(id) < unsigned(a.A)) {
            const double w = a.wtab[static_cast<size_t>(id) * L + jj];
            const double d = -(p.attr_value ? p.attr_value[k] * w : w);
            r = free.change(d, false) - cond.change(d, false);
        }
        if (j == 0) out[k - k0] = r;
    }
}

template <int LP, bool RIGHT>
void launch_walks(const GenArgs &a, const ConditionalArgs &p, hipStream_t stream) {
    hipLaunchKernelGGL((gl_cond_walk<LP, RIGHT>), dim3(group_blocks(p.n_spans, LaneGroup<LP, kCT>::G)), dim3(kCT), 0, stream, a, p);
}

}  // namespace

hipError_t launch_gen_conditionals(const GenArgs &a, const ConditionalArgs &p, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || !a.state || !a.E || !a.alpha || !a.marg) return hipErrorNotSupported;
    if (p.n_spans < 0 || p.reach < 0 || p.n_rows < 0) return hipErrorInvalidValue;
    if (p.n_spans == 0 || p.n_rows == 0) return hipSuccess;
    // (rows, stored vectors and contributions that a kernel does not reach -- an impossible span, a vector without mass -- are zeros)
    const size_t b_rows = static_cast<size_t>(p.n_rows) * a.L * sizeof(double);
    hipError_t rc = hipMemsetAsync(p.cond, 0, b_rows, stream);
    if (rc == hipSuccess) rc = hipMemsetAsync(p.walk, 0, b_rows, stream);
    if (rc == hipSuccess) rc = hipMemsetAsync(p.item, 0, static_cast<size_t>(p.n_rows) * sizeof(double), stream);
    if (rc == hipSuccess && p.n_fwd > 0) rc = hipMemsetAsync(p.fwd, 0, static_cast<size_t>(p.n_fwd) * a.L * sizeof(double), stream);
    if (rc == hipSuccess && p.occ_ptr && p.n_occ > 0) rc = hipMemsetAsync(p.attr, 0, static_cast<size_t>(p.n_occ) * sizeof(double), stream);
    if (rc != hipSuccess) return rc;
    dispatch_lp(a.L, [&](auto lp) {
        launch_walks<lp, true>(a, p, stream);
        launch_walks<lp, false>(a, p, stream);
        hipLaunchKernelGGL(gl_cond_rows<lp>, dim3(group_blocks(p.n_rows, LaneGroup<lp, kCT>::G)), dim3(kCT), 0, stream, a, p);
    });
    return hipGetLastError();
}

}  // namespace gecco
