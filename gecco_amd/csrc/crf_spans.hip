// Region posteriors: log P(y_t in S for every t in [begin, end) | x) on the whole-contig lattice, any
// number of queries behind ONE forward-backward pass of the batch.  The pass (gl_state + any arrangement of the marginals
// recursion, crf_general.hip) leaves in the plan's workspace the raw state scores, E, alpha, and in the caller's buffer the
// marginals; a query walks its own span only.
//
// Layout: one group of lanes per query, on the frame of crf_lane_group.hpp.
//
// Two recursions run side by side in the same lanes over the span, one over every label ("free"), one over the labels of
// the set ("masked").  Both take the RAW state scores: at every item the free one is shifted by the maximum over all labels,
// the masked one by the maximum over the labels of the set, so that a label outside the set that leads by hundreds costs a
// finite, exact amount instead of flushing the set's emissions to zero (the argument of §4.9f, per query).  Each vector is
// scaled to sum 1 at every step and the shifts and the logs of the sums are accumulated -- as the DIFFERENCE of the two
// recursions, which is all the result needs.
//   entering vector: the shifted emissions at the contig's first gene, else alpha[begin - 1] . M -- a direction only: any
//     common positive factor of the stored alpha cancels between the two recursions (gl_marginals_wave does not scale alpha to
//     sum 1 at every gene, and GenArgs::scale is not read here);
//   leaving vector: all ones at the contig's end, else beta = M . (E[end] o marg[end] / alpha[end]), 0 where alpha[end] is 0:
//     marg = alpha o beta up to a factor, so this is the backward vector's direction whatever the arrangement's scaling.
//   log P = sum over the span of ((shift_m - shift_f) + (log sum_m - log sum_f)) + log(v_m . beta) - log(v_f . beta),
//     clipped at 0.  A full set makes the two recursions the same operation sequence: exactly 0.0 (this file is compiled
//     without floating-point contraction, so that the compiler cannot fuse a multiply-add on one side only; fma() is
//     explicit).  -infinity when the masked recursion meets an item that allows no label of the set, or loses all its
//     mass; never NaN.
// A span of thousands of genes is one group's sequential walk (a few hundred us per thousand genes); it is not chunked.
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kST = 256;  // lanes per workgroup

template <int LP>
__global__ void __launch_bounds__(kST) gl_span_logp(GenArgs a, const SpanQuery *__restrict__ spans, const int n_spans,
                                                     double *__restrict__ logp) {
    __shared__ double vecs[2][kST];
    const LaneGroup<LP, kST> g{};
    const int j = g.j;
    double *vf = vecs[0] + g.slot, *vm = vecs[1] + g.slot;
    const long long q = g.item;
    if (q >= n_spans) return;
    const SpanQuery s = spans[q];
    const int L = a.L;
    const int g0 = a.contig_ptr[s.contig], g1 = a.contig_ptr[s.contig + 1];
    const int gb = g0 + s.begin, ge = g0 + s.end;
    const bool on = j < L, in = on && ((s.mask >> j) & 1u);
    const int jj = on ? j : 0;
    const double ninf = -__builtin_huge_val();
    double mcol[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) mcol[i] = (i < L && on) ? a.exp_trans[i * L + j] : 0.0;
    // what enters the span, before its first emission (the same for both recursions)
    double pf = 1.0, pm = 1.0;
    if (gb > g0) {
        pf = pm = sum_product(vf, j, on ? a.alpha[static_cast<size_t>(gb - 1) * L + jj] : 0.0, mcol);
    }
    const double *state = a.state + static_cast<size_t>(gb) * L + jj;
    double xf = 0.0, xm = 0.0, d = 0.0;
    double st = on ? state[0] : ninf;
    for (int t = gb; t < ge; ++t) {
        const double st_next = (t + 1 < ge && on) ? state[static_cast<size_t>(t + 1 - gb) * L] : ninf;
        // (a disallowed label has state -infinity: at least one label is allowed, so the free maximum is finite)
        const double mf = group_max<LP>(on ? st : ninf), mm = group_max<LP>(in ? st : ninf);
        if (!(mm > ninf)) {  // no label of the set is allowed here: P = 0
            if (j == 0) logp[q] = ninf;
            return;
        }
        const double ef = on ? exp(st - mf) : 0.0, em = in ? exp(st - mm) : 0.0;
        if (t > gb) {
            // (the pair of sums is written out, as in gl_run_walk: crf_runs.hip)
            vf[j] = xf;
            vm[j] = xm;
            __builtin_amdgcn_wave_barrier();
            double af = 0.0, am = 0.0;
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                af = fma(vf[i], mcol[i], af);
                am = fma(vm[i], mcol[i], am);
            }
            __builtin_amdgcn_wave_barrier();
            pf = af;
            pm = am;
        }
        xf = pf * ef;
        xm = pm * em;
        const double sf = group_sum<LP>(xf), sm = group_sum<LP>(xm);
        if (!(sm > 0.0)) {  // the set has lost all its mass (zero transitions into it, or underflow)
            if (j == 0) logp[q] = ninf;
            return;
        }
        xf = xf / sf;
        xm = xm / sm;
        d += (mm - mf) + (log(sm) - log(sf));
        st = st_next;
    }
    // what leaves the span: the backward vector's direction at its last gene
    double beta = on ? 1.0 : 0.0;
    if (ge < g1) {
        double w = 0.0;
        if (on) {
            const size_t at = static_cast<size_t>(ge) * L + j;
            const double al = a.alpha[at];
            w = al != 0.0 ? a.E[at] * a.marg[at] / al : 0.0;
        }
        // (written out: one product per query, its row read from memory and not kept in LP registers)
        vf[j] = w;
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        for (int k = 0; k < L; ++k) acc = fma(a.exp_trans[jj * L + k], vf[k], acc);
        __builtin_amdgcn_wave_barrier();
        beta = on ? acc : 0.0;
    }
    const double df = group_sum<LP>(xf * beta), dm = group_sum<LP>(xm * beta);
    double r = ninf;
    if (dm > 0.0) r = fmin(d + (log(dm) - log(df)), 0.0);  // (fmin drops a NaN: the free side cannot be smaller than the masked one)
    if (j == 0) logp[q] = r;
}

template <int LP>
void launch_spans(const GenArgs &a, const SpanQuery *spans, int32_t n_spans, double *logp, hipStream_t stream) {
    hipLaunchKernelGGL(gl_span_logp<LP>, dim3(group_blocks(n_spans, LaneGroup<LP, kST>::G)), dim3(kST), 0, stream, a, spans, n_spans,
                       logp);
}

}  // namespace

hipError_t launch_gen_spans(const GenArgs &a, const SpanQuery *spans, int32_t n_spans, double *logp, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || !a.state || !a.E || !a.alpha || !a.marg) return hipErrorNotSupported;
    if (n_spans <= 0) return hipSuccess;
    dispatch_lp(a.L, [&](auto lp) { launch_spans<lp>(a, spans, n_spans, logp, stream); });
    return hipGetLastError();
}

}  // namespace gecco
