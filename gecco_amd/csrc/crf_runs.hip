// Run posteriors: the exact distribution of where the run through an anchor starts and ends, and the
// probability that a run is exactly a given range, on the whole-contig lattice.  Fix an anchor gene a and a label set S; the
// run through a is the maximal stretch of genes around a whose labels all lie in S.
//   P(start = s) = P(y_s .. y_a in S, and s = 0 or y_{s-1} not in S | x), the ends mirrored;
//   P(run = [b, e)) = P(y_b .. y_{e-1} in S, b = 0 or y_{b-1} not in S, e = T or y_e not in S | x).
// Any number of queries behind ONE forward-backward pass of the batch (gl_state + any arrangement of the marginals recursion,
// crf_general.hip), which leaves the raw state scores, E, alpha and the marginals; a query walks away from its anchor only.
//
// Layout: one group of lanes per walk, on the frame of crf_lane_group.hpp.  A LEFT walk multiplies by the rows of
// exp(trans) (d(k) = sum_j M(k, j) c(j)), a RIGHT walk by its columns: the kernel is templated on the direction and a lane
// holds the one it needs, LP register pairs.  An anchor is two walks in two launches; a closed run is one right walk.
//
// The walk, leftwards (the rightward one mirrors it, with psi beta = E marg / alpha of the next gene in alpha's place):
//   c_a(j) = [j in S] psi_a(j) beta_a(j), beta_a = M . (E o marg / alpha)[a + 1] (ones at the contig's end; 0 where alpha is 0);
//   at t = a, a - 1, ...:  d(k) = sum_j M(k, j) c_t(j);   mass(start = t) = sum_{k not in S} alpha_{t-1}(k) d(k), or sum_j c_0(j)
//   at the contig's first gene;   c_{t-1}(k) = [k in S] psi_{t-1}(k) d(k).
// A free recursion over every label runs side by side in the same lanes; sum_k alpha_{t-1}(k) d_free(k) is Z in the same units,
// so log P = (what the two recursions' scalings differ by) + log mass - log mass_free, and any common factor of the stored alpha
// (a direction only) cancels.  Both take the RAW state scores, the free one shifted by the maximum over all labels, the masked
// one by the maximum over the labels of S, so that a label outside S that leads by hundreds costs its exact, finite amount
// (§4.9f/g).  Each vector is scaled at every step by the power of two that brings its sum into [1/2, 1) -- exact, and no
// logarithm on the way -- and the shifts and exponents accumulate as the DIFFERENCE of the two recursions: a start 400 genes away
// with probability 1e-250 keeps its relative accuracy.  The sum over EVERY k of the masked products is P(y_t .. y_a in S): the
// anchor's own probability at the first step, the mass beyond the reach at step reach + 1.
// A full set makes the two recursions the same operation sequence: log_anchor is exactly 0.0 (this file is compiled without
// floating-point contraction, so that the compiler cannot fuse a multiply-add on one side only; fma() is explicit) and every
// start but the contig's first gene has an empty complement, -infinity.  A walk that loses all its mass -- a gene that allows
// no label of S, zero transitions, underflow -- writes -infinity for the rest and stops; never NaN.  Results are clipped at 0.
// A walk is one fixed operation sequence: entry r does not depend on reach, nor on the other queries.  No atomics.
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kRT = 256;  // lanes per workgroup

// log(num / den) + d + e2 log 2 as a stored log-probability: -infinity for no mass, at most 0 (fmin drops a NaN)
__device__ __forceinline__ double run_logp(double d, int e2, double num, double den) {
    constexpr double kLn2 = 0.693147180559945309417232121458;
    return (num > 0.0 && den > 0.0) ? fmin((d + e2 * kLn2) + (log(num) - log(den)), 0.0) : -__builtin_huge_val();
}
// the power of two that brings a positive sum into [1/2, 1)
__device__ __forceinline__ int scale_exponent(double s) {
    int e;
    (void)__builtin_frexp(s, &e);
    return e;
}

// What a walk reads of the gene beyond its current one, loaded one step ahead of its use: alpha (a left walk's other side of the
// edge), and for a right walk E and marg as well -- psi beta as a direction is E marg / alpha, 0 where alpha is 0 (crf_spans.hip's
// leaving vector).  The division waits until the value is used, so that the loads stay in flight over a whole step.
template <bool RIGHT>
struct Neighbour {
    double al = 0.0, e = 0.0, mg = 0.0;
    __device__ __forceinline__ void load(const GenArgs &a, size_t at) {
        al = a.alpha[at];
        if (RIGHT) {
            e = a.E[at];
            mg = a.marg[at];
        }
    }
    __device__ __forceinline__ double value() const { return !RIGHT ? al : al != 0.0 ? e * mg / al : 0.0; }
};

// RIGHT = false: the left walks of the anchors, one group each: log_anchor, log_start, log_start_beyond.
// RIGHT = true: the right walks of the anchors (log_end, log_end_beyond), then the closed runs (log_run), one group each.
template <int LP, bool RIGHT>
__global__ void __launch_bounds__(kRT) gl_run_walk(GenArgs a, RunPosteriorArgs p) {
    __shared__ double vecs[2][kRT];
    const LaneGroup<LP, kRT> g{};
    const int j = g.j;
    double *vf = vecs[0] + g.slot, *vm = vecs[1] + g.slot;
    const long long q = g.item;
    const int n_walks = RIGHT ? p.n_anchors + p.n_runs : p.n_anchors;
    if (q >= n_walks) return;
    const bool closed = RIGHT && q >= p.n_anchors;
    int contig, first, r_lo, r_hi, r_last;  // entries r_lo .. r_hi are stored at out[r - r_lo]; the walk ends with step r_last
    uint32_t mask;
    double *out, *beyond = nullptr;
    if (closed) {
        const SpanQuery s = p.runs[q - p.n_anchors];
        contig = s.contig, first = s.begin, mask = s.mask;
        r_lo = r_hi = r_last = s.end - 1 - s.begin;
        out = p.log_run + (q - p.n_anchors);
    } else {
        const RunQuery s = p.anchors[q];
        contig = s.contig, first = s.anchor, mask = s.mask;
        r_lo = 0, r_hi = p.reach, r_last = p.reach + 1;
        out = (RIGHT ? p.log_end : p.log_start) + static_cast<size_t>(q) * (static_cast<size_t>(p.reach) + 1);
        beyond = (RIGHT ? p.log_end_beyond : p.log_start_beyond) + q;
    }
    const int L = a.L;
    const int g0 = a.contig_ptr[contig], g1 = a.contig_ptr[contig + 1];
    const int ga = g0 + first;
    const int edge = RIGHT ? g1 - 1 : g0;  // the last gene of the walk's direction
    constexpr int dir = RIGHT ? 1 : -1;
    const bool on = j < L, in = on && ((mask >> j) & 1u);
    const int jj = on ? j : 0;
    const double ninf = -__builtin_huge_val();
    // the lane's row (left) or column (right) of exp(trans)
    double mvec[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) mvec[i] = (i < L && on) ? (RIGHT ? a.exp_trans[i * L + j] : a.exp_trans[j * L + i]) : 0.0;

    // everything from entry r on is -infinity (all lanes of the group take part)
    auto no_mass_from = [&](int r) {
        for (int k = (r > r_lo ? r : r_lo) + j; k <= r_hi; k += LP) out[k - r_lo] = ninf;
        if (j == 0 && beyond) *beyond = ninf;
        if (!RIGHT && j == 0 && r == 0) p.log_anchor[q] = ninf;
    };

    // what reaches the anchor from the other side, the same for both recursions: left walk beta_a, right walk alpha_{a-1} . M.
    // A closed run is entered from outside the set: the masked recursion takes the complement's alpha only.
    double pf = on ? 1.0 : 0.0, pm = pf;
    if (RIGHT ? ga > g0 : ga < g1 - 1) {
        const size_t at = static_cast<size_t>(ga - dir) * L + jj;
        Neighbour<!RIGHT> other;  // (a left walk starts from psi beta of gene a + 1, a right walk from alpha of gene a - 1)
        if (on) other.load(a, at);
        const double w = on ? other.value() : 0.0;
        // (the pair of sums is written out, here and in the walk: with a helper for it the right walks compile to another schedule)
        vf[j] = w;
        vm[j] = (closed && in) ? 0.0 : w;
        __builtin_amdgcn_wave_barrier();
        double af = 0.0, am = 0.0;
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            af = fma(vf[i], mvec[i], af);
            am = fma(vm[i], mvec[i], am);
        }
        __builtin_amdgcn_wave_barrier();
        pf = af;
        pm = am;
    }
    double d = 0.0, xf, xm;
    int e2 = 0, t = ga;
    // the state scores of gene t and the neighbour's values of gene t + dir are loaded one step ahead (a step is a chain of
    // dependent reductions: what it reads next does not depend on it)
    double st = on ? a.state[static_cast<size_t>(ga) * L + jj] : ninf;
    Neighbour<RIGHT> nb;
    if (on && ga != edge) nb.load(a, static_cast<size_t>(ga + dir) * L + jj);
    for (int r = 0;; ++r, t += dir) {
        double st_next = ninf;
        Neighbour<RIGHT> nb_next;
        if (on && t != edge && r < r_last) {
            st_next = a.state[static_cast<size_t>(t + dir) * L + jj];
            if (t + dir != edge) nb_next.load(a, static_cast<size_t>(t + 2 * dir) * L + jj);
        }
        // the vectors at gene t from what the product handed over: the emission, scaled to a sum in [1/2, 1)
        // (a disallowed label has state -infinity: at least one label is allowed, so the free maximum is finite)
        const double mf = group_max<LP>(st), mm = group_max<LP>(in ? st : ninf);
        if (!(mm > ninf)) return no_mass_from(r);  // no label of the set is allowed here
        xf = pf * (on ? exp(st - mf) : 0.0);
        xm = pm * (in ? exp(st - mm) : 0.0);
        const double sf = group_sum<LP>(xf), sm = group_sum<LP>(xm);
        // the set has lost all its mass (zero transitions into it, or underflow; a free side without mass is outside the pass's range)
        if (!(sm > 0.0) || !(sf > 0.0)) return no_mass_from(r);
        // (scaled by exact powers of two: no rounding, no logarithm on the way; the exponents accumulate as an integer)
        const int ef = scale_exponent(sf), em = scale_exponent(sm);
        xf = ldexp(xf, -ef);
        xm = ldexp(xm, -em);
        d += mm - mf;
        e2 += em - ef;
        const bool want_all = !closed && (r == r_last || (!RIGHT && r == 0)), want_out = r >= r_lo && r <= r_hi;
        if (t == edge) {  // the run reaches the contig's end: it stops here, whatever the labels
            const double lp = run_logp(d, e2, ldexp(sm, -em), ldexp(sf, -ef));
            if (j == 0) {
                if (want_out) out[r - r_lo] = lp;
                if (!RIGHT && r == 0) p.log_anchor[q] = lp;
                if (r == r_last && beyond) *beyond = lp;
            }
            if (r < r_last) {  // no gene beyond: the later entries, and the mass beyond the reach
                for (int k = (r + 1 > r_lo ? r + 1 : r_lo) + j; k <= r_hi; k += LP) out[k - r_lo] = ninf;
                if (j == 0 && beyond) *beyond = ninf;
            }
            return;
        }
        vf[j] = xf;
        vm[j] = xm;
        __builtin_amdgcn_wave_barrier();
        double af = 0.0, am = 0.0;
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            af = fma(vf[i], mvec[i], af);
            am = fma(vm[i], mvec[i], am);
        }
        __builtin_amdgcn_wave_barrier();
        pf = af;
        pm = am;
        // the neighbour's side of the edge: alpha_{t-1} (left), psi beta of gene t + 1 (right)
        const double w = on ? nb.value() : 0.0;
        const double tf = w * af, tm = w * am;
        const double den = group_sum<LP>(tf);
        if (want_out) {
            const double lp = run_logp(d, e2, group_sum<LP>(in ? 0.0 : tm), den);
            if (j == 0) out[r - r_lo] = lp;
        }
        if (want_all) {
            const double lp = run_logp(d, e2, group_sum<LP>(tm), den);
            if (j == 0) {
                if (r == r_last) *beyond = lp;
                else p.log_anchor[q] = lp;
            }
        }
        if (r == r_last) return;
        st = st_next;
        nb = nb_next;
    }
}

template <int LP, bool RIGHT>
void launch_walks(const GenArgs &a, const RunPosteriorArgs &p, hipStream_t stream) {
    const long long n = RIGHT ? static_cast<long long>(p.n_anchors) + p.n_runs : p.n_anchors;
    if (n <= 0) return;
    hipLaunchKernelGGL((gl_run_walk<LP, RIGHT>), dim3(group_blocks(n, LaneGroup<LP, kRT>::G)), dim3(kRT), 0, stream, a, p);
}

}  // namespace

hipError_t launch_gen_runs(const GenArgs &a, const RunPosteriorArgs &p, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || !a.state || !a.E || !a.alpha || !a.marg) return hipErrorNotSupported;
    if (p.n_anchors < 0 || p.n_runs < 0 || p.reach < 0 || p.reach > kMaxRunReach) return hipErrorInvalidValue;
    dispatch_lp(a.L, [&](auto lp) {
        launch_walks<lp, false>(a, p, stream);
        launch_walks<lp, true>(a, p, stream);
    });
    return hipGetLastError();
}

}  // namespace gecco
