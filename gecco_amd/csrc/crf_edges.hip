// Edge posteriors: the pairwise marginals xi_t(i, j) = P(y_{t-1} = i, y_t = j | x) of the whole-contig lattice
// and what follows from them -- the probability that a run of labels of a set starts or ends at a gene, the expected
// transition counts of a contig, the entropy of its path distribution -- behind ONE forward-backward pass of the batch.  The
// pass (gl_state + any arrangement of the marginals recursion, crf_general.hip) leaves E and alpha in the plan's workspace and
// the marginals in the caller's buffer; an edge reads the two genes it joins and nothing else, so this is the lattice query
// that is parallel over genes.
//
// Layout: one group of lanes per run, on the frame of crf_lane_group.hpp (its geometry; the xi product below is the kernel's
// own).  A group walks one RUN: kEdgeRunGenes consecutive genes of one contig,
// counted from the contig's first gene (not the batch's), so that what a contig gets does not depend on its place in the
// batch.  Per gene every lane loads alpha, E and marg of its label once; the previous gene's come along in registers.
//   directions: alpha_{t-1} and w_t(j) = E_t(j) marg_t(j) / alpha_t(j) (0 where alpha_t(j) is 0; the backward direction of
//     gl_span_logp) are each divided by their own group maximum before any product is formed: no common factor of an
//     arrangement's alpha can overflow or flush a product, and the result does not depend on it (GenArgs::scale is not read);
//   u(i, j) = alpha_{t-1}(i) M(i, j) w_t(j) goes through one LDS slot per lane for alpha_{t-1}, xi = u / sum u;
//   enter[t] / leave[t - 1] of a set are the sums of xi over (i outside, j inside) / (i inside, j outside), formed from the
//     registers in a fixed order per set: a set's result depends on neither the other sets nor their order;
//   entropy by the chain rule: H(marg at the first gene) + sum_t sum_i marg_{t-1}(i) H(c_t(. | i)), c_t(j | i) = M(i, j) w_t(j) /
//     r(i), r(i) = sum_j' M(i, j') w_t(j').  Lane i walks row i of exp(trans) and of trans, which the workgroup keeps transposed
//     in LDS (lanes read consecutive words), and forms H(c(. | i)) = log r(i) - sum_j c(j | i) (trans(i, j) + log w_t(j)), terms
//     of c = 0 left out (0 log 0 = 0), clipped at 0: two logs per lane and edge instead of L, at an error of a few ulps of
//     |trans(i, j)| + |log w_t(j)| per row -- the size of ONE transition, weighted by marg_{t-1}(i), never that of log Z;
//   a disallowed (gene, label) pair has E = marg = alpha = 0: exact zeros in every product; a probability that a sum's last
//     rounding put above 1 is clipped at 1.
// The group keeps its L x L partial of the transition counts in registers and stores it per run; gl_edge_reduce adds a contig's
// partials in run order.  No atomics anywhere: equal calls give equal bytes.  (Nothing here is specified as an exact difference
// of two like recursions: the file is compiled with floating-point contraction left on.)
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kET = 256;  // lanes per workgroup

template <int LP>
__global__ void __launch_bounds__(kET) gl_edge_runs(GenArgs a, EdgeQuery q) {
    __shared__ double vecs[3][kET];
    __shared__ double mt[LP * LP], tt[LP * LP];  // mt[k * LP + i] = M(i, k), tt[k * LP + i] = trans(i, k); 0 beyond L
    const int L = a.L;
    for (int e = threadIdx.x; e < LP * LP; e += kET) {
        const int k = e / LP, i = e & (LP - 1);
        mt[e] = (i < L && k < L) ? a.exp_trans[i * L + k] : 0.0;
        tt[e] = (i < L && k < L) ? a.trans[i * L + k] : 0.0;
    }
    __syncthreads();
    const LaneGroup<LP, kET> g{};
    const int j = g.j;
    double *va = vecs[0] + g.slot, *vw = vecs[1] + g.slot, *vl = vecs[2] + g.slot;
    const long long r = g.item;
    if (r >= q.n_runs) return;
    const EdgeRun run = q.runs[r];
    const int g0 = a.contig_ptr[run.contig], g1 = a.contig_ptr[run.contig + 1];
    const int gb = g0 + run.begin, ge = min(gb + kEdgeRunGenes, g1);
    const bool on = j < L;
    const int jj = on ? j : 0;
    const size_t LL = static_cast<size_t>(L) * L, ns = static_cast<size_t>(q.n_sets);
    double mcol[LP], nacc[LP], xi[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) {
        mcol[i] = (i < L && on) ? a.exp_trans[i * L + j] : 0.0;
        nacc[i] = 0.0;
    }
    double hacc = 0.0;
    // the previous gene's alpha and marginal of this lane's label
    double al_p = 0.0, mg_p = 0.0;
    if (gb > g0 && on) {
        al_p = a.alpha[static_cast<size_t>(gb - 1) * L + j];
        mg_p = a.marg[static_cast<size_t>(gb - 1) * L + j];
    }
    // (a gene's three values are asked for one gene ahead: a step does not wait for its own loads)
    size_t at = static_cast<size_t>(gb) * L + jj;
    double al_n = on ? a.alpha[at] : 0.0, mg_n = on ? a.marg[at] : 0.0, em_n = on ? a.E[at] : 0.0;
    for (int t = gb; t < ge; ++t) {
        const double al = al_n, mg = mg_n, em = em_n;
        if (t + 1 < ge && on) {
            at += L;
            al_n = a.alpha[at];
            mg_n = a.marg[at];
            em_n = a.E[at];
        }
        if (t == g0) {
            // a contig's first gene: no edge enters it
            if (q.pair && on)
                for (int i = 0; i < L; ++i) q.pair[static_cast<size_t>(t) * LL + static_cast<size_t>(i) * L + j] = 0.0;
            if (q.enter)
                for (int s = 0; s < q.n_sets; ++s) {
                    const double p = fmin(group_sum<LP>(((q.set_mask[s] >> j) & 1u) ? mg : 0.0), 1.0);
                    if (j == 0) q.enter[static_cast<size_t>(t) * ns + s] = p;
                }
            if (q.hpart) hacc = group_sum<LP>(mg > 0.0 ? -mg * log(fmin(mg, 1.0)) : 0.0);
        } else {
            const double amax = group_max<LP>(al_p), cmax = group_max<LP>(al);
            const double ah = amax > 0.0 ? al_p / amax : 0.0, ch = cmax > 0.0 ? al / cmax : 0.0;
            const double w = ch > 0.0 ? fmin(em * mg / ch, DBL_MAX) : 0.0;
            const double wmax = group_max<LP>(w);
            const double wh = wmax > 0.0 ? w / wmax : 0.0;
            va[j] = ah;
            vw[j] = wh;
            if (q.hpart) vl[j] = wh > 0.0 ? log(wh) : 0.0;
            __builtin_amdgcn_wave_barrier();  // (the kernel's own exchange: three slots, read until the end of the step)
            double col = 0.0;
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                xi[i] = (va[i] * mcol[i]) * wh;
                col += xi[i];
            }
            const double total = group_sum<LP>(col);
            const double inv = total > 0.0 ? 1.0 / total : 0.0;
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                xi[i] = fmin(xi[i] * inv, 1.0);
                nacc[i] += xi[i];
            }
            if (q.pair && on) {
                double *row = q.pair + static_cast<size_t>(t) * LL + j;
#pragma unroll
                for (int i = 0; i < LP; ++i)
                    if (i < L) row[static_cast<size_t>(i) * L] = xi[i];
            }
            if (q.enter || q.leave)
                for (int s = 0; s < q.n_sets; ++s) {
                    const uint32_t m = q.set_mask[s];
                    const uint32_t in = (m >> j) & 1u;
                    double acc = 0.0;  // this column's mass from the labels on the other side of the set
#pragma unroll
                    for (int i = 0; i < LP; ++i) acc += (((m >> i) & 1u) != in) ? xi[i] : 0.0;
                    const double en = fmin(group_sum<LP>(in ? acc : 0.0), 1.0), lv = fmin(group_sum<LP>(in ? 0.0 : acc), 1.0);
                    if (j == 0) {
                        if (q.enter) q.enter[static_cast<size_t>(t) * ns + s] = en;
                        if (q.leave) q.leave[static_cast<size_t>(t - 1) * ns + s] = lv;
                    }
                }
            if (q.hpart) {
                // lane i: the conditional row c(. | i) and its entropy, weighted by marg_{t-1}(i)
                double rs = 0.0;
#pragma unroll
                for (int k = 0; k < LP; ++k) rs = fma(mt[k * LP + j], vw[k], rs);
                double h = 0.0;
                if (rs > 0.0 && mg_p > 0.0) {
                    // -sum_k c log c with log c = (trans(i, k) + log w(k)) - log r: sum_k p_k log p_k over the row, then one log
                    double sl = 0.0;
#pragma unroll
                    for (int k = 0; k < LP; ++k) {
                        const double p = mt[k * LP + j] * vw[k];
                        sl = fma(p, p > 0.0 ? tt[k * LP + j] + vl[k] : 0.0, sl);
                    }
                    h = fmax(log(rs) - sl / rs, 0.0);
                }
                hacc += group_sum<LP>(mg_p * h);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (t == g1 - 1 && q.leave)
            // a contig's last gene: a run that holds it ends there
            for (int s = 0; s < q.n_sets; ++s) {
                const double p = fmin(group_sum<LP>(((q.set_mask[s] >> j) & 1u) ? mg : 0.0), 1.0);
                if (j == 0) q.leave[static_cast<size_t>(t) * ns + s] = p;
            }
        al_p = al;
        mg_p = mg;
    }
    if (q.npart && on) {
        double *part = q.npart + static_cast<size_t>(r) * LL + j;
#pragma unroll
        for (int i = 0; i < LP; ++i)
            if (i < L) part[static_cast<size_t>(i) * L] = nacc[i];
    }
    if (q.hpart && j == 0) q.hpart[r] = hacc;
}

// transitions[c] and entropy[c]: the partials of contig c's runs, added in run order (one lane per entry; a contig without
// genes has no run: zeros)
__global__ void __launch_bounds__(kET) gl_edge_reduce(EdgeQuery q, const int L, const int n_contigs) {
    const long long per = static_cast<long long>(L) * L + 1;
    const long long e = static_cast<long long>(blockIdx.x) * kET + threadIdx.x;
    if (e >= per * n_contigs) return;
    const long long c = e / per, k = e - c * per;
    const int r0 = q.run_ptr[c], r1 = q.run_ptr[c + 1];
    double acc = 0.0;
    if (k < per - 1) {
        if (!q.transitions) return;
        for (int r = r0; r < r1; ++r) acc += q.npart[static_cast<size_t>(r) * (per - 1) + k];
        q.transitions[static_cast<size_t>(c) * (per - 1) + k] = acc;
    } else {
        if (!q.entropy) return;
        for (int r = r0; r < r1; ++r) acc += q.hpart[r];
        q.entropy[c] = acc;
    }
}

template <int LP>
void launch_runs(const GenArgs &a, const EdgeQuery &q, hipStream_t stream) {
    hipLaunchKernelGGL(gl_edge_runs<LP>, dim3(group_blocks(q.n_runs, LaneGroup<LP, kET>::G)), dim3(kET), 0, stream, a, q);
}

}  // namespace

hipError_t launch_gen_edges(const GenArgs &a, const EdgeQuery &q, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || !a.E || !a.alpha || !a.marg || !a.contig_ptr || !a.exp_trans || !a.trans) return hipErrorNotSupported;
    if (q.n_sets < 0 || q.n_sets > kMaxEdgeSets || q.n_runs < 0 || !q.run_ptr || (q.n_runs > 0 && !q.runs)) return hipErrorInvalidValue;
    if ((q.transitions && !q.npart) || (q.entropy && !q.hpart)) return hipErrorInvalidValue;
    if (q.n_runs > 0) {
        dispatch_lp(a.L, [&](auto lp) { launch_runs<lp>(a, q, stream); });
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    if ((q.transitions || q.entropy) && a.n_contigs > 0) {
        const long long entries = (static_cast<long long>(a.L) * a.L + 1) * a.n_contigs;
        hipLaunchKernelGGL(gl_edge_reduce, dim3(group_blocks(entries, kET)), dim3(kET), 0, stream, q, a.L, a.n_contigs);
    }
    return hipGetLastError();
}

}  // namespace gecco
