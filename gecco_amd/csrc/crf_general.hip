// Any number of labels (1 <= L <= 32): rows S, F and V of SURVEY.md §8a for CRFsuite models other than GECCO's 2-label
// one: the state scores and the whole-contig recursions.  The windowed marginals (rows A/B, P, W)
// are in crf_general_windowed.hip and read gl_state's E.  GECCO's own model never comes here;
// `GECCO_CRF_FORCE_GENERAL=1` routes 2-label models through these kernels so the tests can cross-check the specialised
// kernels on the device.
//
// Layout: a group of LP lanes per contig, chunk or chunk row, lane j holding component j of the alpha / beta / delta vector;
// crf_lane_group.hpp has the geometry and the products through the group's LDS slot, and describes the registers of the table.  (The
// wave-per-contig and matrix-core kernels below have layouts and exchanges of their own.)
//
// Arithmetic follows [EXT] CRFsuite crf1d_context.c in its own order (alpha: sum over the
// source label in index order, then * exp(state), then 1/sum scaling; beta: row . (beta o exp(state))
// then * scale; marginal = alpha * beta / scale; Viterbi: strict `<` update, first arg max), with
// one deliberate difference: exp(state - max_y state) instead of exp(state), which cancels in
// every marginal and is added back to the log-partition.
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kGT = 256;  // lanes per workgroup

// last gene + 1 of chunk ci: where the next chunk starts, or where its contig ends (the chunk table may list the long contigs
// of a batch only: the next chunk then belongs to a contig further on)
__device__ __forceinline__ int gl_chunk_end(const GenArgs &a, long long ci) {
    return min(a.ch_g0[ci + 1], a.contig_ptr[a.ch_contig[ci] + 1]);
}

// ---- row S: state scores of every gene (CSR order, bit-identical to sequential addition) ----
// state[g][y] = sum_a w[a][y]; E[g][y] = exp(state - max_y); smax[g] = max_y state.
// kValued (the *_valued entries): state[g][y] = sum_a v[a] * w[a][y], attr_value parallel to attr_id, every term
// added as fma(v, w, acc) in CSR order -- the one multiply-add form of every valued kernel, so that v = 1.0 gives the unvalued
// sum's bits (fma(1, w, acc) rounds acc + w once).  The unvalued instantiation is the kernel as it was (attr_value is not read
// there).
// kMasked (the *_constrained entries): allowed[g] has bit y set when gene g may take label y.  A disallowed
// (gene, label) pair leaves the lattice: state = -infinity, E = 0.0 exactly, and the maximum m -- smax, and the shift of E -- is
// taken over the ALLOWED labels only.  (Over all labels, a disallowed label that leads by 750 would flush every allowed
// emission to zero.)  Every gene then still has an emission equal to 1, which is what the range guards of the sum-product
// kernels are argued from.  The host has refused a mask without a bit below L.  The unmasked instantiations do not read
// `allowed` and keep their code.
template <int LP, bool kValued, bool kMasked>
__global__ void __launch_bounds__(kGT) gl_state(const int32_t *__restrict__ gene_ptr, const int32_t *__restrict__ attr_id,
                                                const double *__restrict__ wtab, int L, int A, int n_genes,
                                                double *__restrict__ state, double *__restrict__ E,
                                                double *__restrict__ smax, const double *__restrict__ attr_value,
                                                const uint32_t *__restrict__ allowed) {
    // (the gene from the flat lane index: LaneGroup's item is the same number, formed another way, and compiles to other code)
    const int j = threadIdx.x & (LP - 1);
    const long long g = (static_cast<long long>(blockIdx.x) * kGT + threadIdx.x) / LP;
    if (g >= n_genes) return;
    const int lo = gene_ptr[g], hi = gene_ptr[g + 1];
    const int jj = j < L ? j : 0;
    double acc = 0.0;
    for (int a = lo; a < hi; ++a) {
        const int id = attr_id[a];  // ids outside the model's dictionary are unknown attributes: no weight, whatever their value
        if (unsigned(id) < unsigned(A)) {
            if constexpr (kValued)
                acc = fma(attr_value[a], wtab[static_cast<size_t>(id) * L + jj], acc);
            else
                acc += wtab[static_cast<size_t>(id) * L + jj];
        }
    }
    if constexpr (kMasked) {
        const bool ok = j < L && ((allowed[g] >> j) & 1u);
        const double m = group_max<LP>(ok ? acc : -DBL_MAX);
        if (j < L) {
            if (state) state[static_cast<size_t>(g) * L + j] = ok ? acc : -__builtin_huge_val();
            if (E) E[static_cast<size_t>(g) * L + j] = ok ? exp(acc - m) : 0.0;
        }
        if (j == 0 && smax) smax[g] = m;
    } else {
        const double m = group_max<LP>(j < L ? acc : -DBL_MAX);
        if (j < L) {
            if (state) state[static_cast<size_t>(g) * L + j] = acc;
            if (E) E[static_cast<size_t>(g) * L + j] = exp(acc - m);
        }
        if (j == 0 && smax) smax[g] = m;
    }
}

// ---- row F: whole-contig marginals, one group per contig, CRFsuite's own sequential recursion ----
template <int LP>
__global__ void __launch_bounds__(kGT) gl_marginals_seq(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const long long ci = g.item;
    if (ci >= a.n_contigs) return;
    const int L = a.L;
    const int g0 = a.contig_ptr[ci], T = a.contig_ptr[ci + 1] - g0;
    if (T <= 0) {
        if (j == 0 && a.lognorm) a.lognorm[ci] = 0.0;
        return;
    }
    const bool on = j < L;
    const int jj = on ? j : 0;
    double mcol[LP], mrow[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) {
        const bool ok = i < L && on;
        mcol[i] = ok ? a.exp_trans[i * L + j] : 0.0;
        mrow[i] = ok ? a.exp_trans[j * L + i] : 0.0;
    }
    const double *E = a.E + static_cast<size_t>(g0) * L;
    double *alpha = a.alpha + static_cast<size_t>(g0) * L;
    double *scale = a.scale + g0;
    double lognorm = 0.0, v = 0.0, c = 1.0;
    double e = on ? E[jj] : 0.0;
    for (int t = 0; t < T; ++t) {
        const double e_next = (t + 1 < T && on) ? E[static_cast<size_t>(t + 1) * L + jj] : 0.0;
        const double sm = a.smax[g0 + t];
        if (t == 0) {
            v = e;
        } else {
            v = sum_product(vec, j, v, mcol) * e;
        }
        const double s = group_sum<LP>(v);
        c = s != 0.0 ? 1.0 / s : 1.0;
        v *= c;
        if (on) alpha[static_cast<size_t>(t) * L + j] = v;
        if (j == 0) scale[t] = c;
        lognorm += sm - log(c);
        e = e_next;
    }
    if (j == 0 && a.lognorm) a.lognorm[ci] = lognorm;
    // backward; alpha/scale of step t were written by this very lane / this group's lane 0
    double *marg = a.marg + static_cast<size_t>(g0) * L;
    double b = c;
    if (on) marg[static_cast<size_t>(T - 1) * L + j] = gl_prob(v * b / c);
    double al_p = (T >= 2 && on) ? alpha[static_cast<size_t>(T - 2) * L + j] : 0.0;
    double c_p = T >= 2 ? __shfl(j == 0 ? scale[T - 2] : 0.0, 0, LP) : 1.0;
    double e1 = (T >= 2 && on) ? E[static_cast<size_t>(T - 1) * L + jj] : 0.0;
    for (int t = T - 2; t >= 0; --t) {
        const double al_t = al_p, ct = c_p, et1 = e1;
        if (t > 0) {  // prefetch step t-1 while step t computes
            al_p = on ? alpha[static_cast<size_t>(t - 1) * L + j] : 0.0;
            c_p = __shfl(j == 0 ? scale[t - 1] : 0.0, 0, LP);
            e1 = on ? E[static_cast<size_t>(t) * L + jj] : 0.0;
        }
        b = sum_product<true>(vec, j, b * et1, mrow) * ct;
        if (on) marg[static_cast<size_t>(t) * L + j] = gl_prob(al_t * b / ct);
    }
}

// ---- row V: whole-contig Viterbi, one group per contig ------------------------------------------
constexpr int kBackRows = 32;  // back-pointer rows walked from LDS per global round trip

// FIX: only the contigs gl_chunk_vit flagged (a decision inside its margin), whose labels and score this overwrites with
// CRFsuite's; their flags are cleared again
template <int LP, bool FIX = false>
__global__ void __launch_bounds__(kGT) gl_viterbi_seq(GenArgs a) {
    __shared__ double vecs[kGT];
    __shared__ uint8_t rows[kGT * kBackRows];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    uint8_t *row = rows + g.slot * kBackRows;
    const long long ci = g.item;
    if (ci >= a.n_contigs) return;
    if (FIX && !a.fix_flag[ci]) return;  // (group-uniform)
    const int L = a.L;
    const int g0 = a.contig_ptr[ci], T = a.contig_ptr[ci + 1] - g0;
    if (FIX && j == 0) {
        a.fix_flag[ci] = 0;  // (every lane of the group has read it: they run in step)
        atomicAdd(a.vit_stats + 2, 1u);
        atomicAdd(a.vit_stats + 3, uint32_t(T));
    }
    if (T <= 0) {
        if (j == 0 && a.score) a.score[ci] = 0.0;
        return;
    }
    const bool on = j < L;
    const int jj = on ? j : 0;
    double tcol[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) tcol[i] = (i < L && on) ? a.trans[i * L + j] : 0.0;
    const double *st = a.state + static_cast<size_t>(g0) * L;
    uint8_t *back = a.back + static_cast<size_t>(g0) * L;
    double d = on ? st[jj] : -DBL_MAX;
    double s_next = (T > 1 && on) ? st[static_cast<size_t>(L) + jj] : 0.0;
    for (int t = 1; t < T; ++t) {
        const double s_t = s_next;
        if (t + 1 < T) s_next = on ? st[static_cast<size_t>(t + 1) * L + jj] : 0.0;
        const MaxPlusArg m = max_plus_arg(vec, j, d, tcol, L);
        if (on) back[static_cast<size_t>(t) * L + j] = static_cast<uint8_t>(m.arg < 0 ? 0 : m.arg);
        d = m.best + s_t;
    }
    // end label = first arg max; back-tracking by lane 0, rows staged through LDS in chunks (exchanges of their own: no product)
    vec[j] = d;
    __builtin_amdgcn_wave_barrier();
    int y = 0;
    {
        double best = -DBL_MAX;
        for (int i = 0; i < L; ++i)
            if (best < vec[i]) {
                best = vec[i];
                y = i;
            }
        if (j == 0 && a.score) a.score[ci] = best;
    }
    int8_t *yout = a.y + g0;
    if (j == 0) yout[T - 1] = static_cast<int8_t>(y);
    __threadfence();
    for (int hi = T - 1; hi >= 1; hi -= kBackRows) {
        const int lo = hi - kBackRows + 1 > 1 ? hi - kBackRows + 1 : 1;  // rows lo..hi
        const int nb = (hi - lo + 1) * L;
        const uint8_t *src = back + static_cast<size_t>(lo) * L;
        for (int k = j; k < nb; k += LP) row[k] = src[k];
        __builtin_amdgcn_wave_barrier();
        if (j == 0) {
            for (int t = hi; t >= lo; --t) {
                y = row[(t - lo) * L + y];
                yout[t - 1] = static_cast<int8_t>(y);
            }
        }
        y = __shfl(y, 0, LP);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- row V for 17 to 32 labels, batches of many contigs: one WAVE per contig ------------------------------------------
// The chunked recursions below pay for their parallelism inside a contig with L x the arithmetic (a chunk's transfer matrix is
// L forward recursions): 32 x at L = 32, where a batch of a thousand contigs has all the parallelism the chip can use in its
// contigs alone (C2's shape, L = 32: 1.42 ms chunked).  Here a contig is a wave walking it gene by gene, CRFsuite's own
// recursion ([EXT] crf1dc_viterbi: strict `<` update, first arg max).  The batch then takes as long as its LONGEST contig,
// and a lone wave issues one instruction every four cycles whatever the instruction is -- so the step is built to be short in
// instructions (~95 at L <= 32: 0.36 us), not in flops:
//   * lane (j, h), h = lane % H, holds target label j and the source labels [h PER, (h + 1) PER): H = 64 / LP partial maxima
//     per target in ONE quad of lanes, merged over h in ascending order by DPP quad permutes (ties keep the lower source
//     label, as the sequential loop does); a lane's maximum is a v_max_f64 chain, its first arg max a compare-select chain;
//   * no exec-mask juggling: lanes of labels that do not exist repeat label 0's work, every store is unconditional;
//   * the state scores of the next sixteen genes are loaded while the current sixteen are walked (one round trip to memory
//     per sixteen steps, hidden), the previous delta goes through one LDS slot per label;
//   * back-pointers leave as one dword per label and FOUR genes (a contig's region of `back`, dword-aligned inside it: the
//     regions of neighbouring contigs cannot meet); the last, incomplete quad never leaves its register;
//   * back-tracking reads sixteen quads per round (prefetched) and walks them on the scalar unit: the label is wave-uniform,
//     a step is v_readlane_b32 + s_bfe -- no dependent memory access.
// Measured (1 000 contigs, 0.22 M genes, longest 1 519; chunked -> wave): L = 32 1.42 -> 0.55 ms, L = 24 0.96 -> 0.55 ms;
// L = 16 0.30 -> 0.37 ms, L = 9 0.20 -> 0.36 ms: the plan takes this kernel above 16 labels when the longest contig is short
// against the batch (plan_run_viterbi), and tests force it from 9 labels up.
constexpr int kWaveK = 16;      // genes per staged block of state scores
constexpr int kWaveQuads = 16;  // back-pointer quads per back-tracking round

// lane l <- lane l ^ 1 / l ^ 2 inside its quad (DPP quad_perm: no LDS round trip)
template <int X>
__device__ __forceinline__ int gl_quad_xor(int v) {
    return __builtin_amdgcn_update_dpp(0, v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, true);
}
template <int X>
__device__ __forceinline__ double gl_quad_xor(double v) {
    return __hiloint2double(gl_quad_xor<X>(__double2hiint(v)), gl_quad_xor<X>(__double2loint(v)));
}

template <int LP>
__global__ void __launch_bounds__(kGT) gl_viterbi_wave(GenArgs a) {
    constexpr int H = 64 / LP, PER = LP / H, K = kWaveK, Q = kWaveQuads;
    __shared__ double vecs[kGT / 64][LP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const long long ci = static_cast<long long>(blockIdx.x) * (kGT / 64) + wave;
    if (ci >= a.n_contigs) return;
    const int L = a.L, h = lane & (H - 1), j = lane / H;  // (the H lanes of a target label share a quad)
    const int g0 = __builtin_amdgcn_readfirstlane(a.contig_ptr[ci]);
    const int T = __builtin_amdgcn_readfirstlane(a.contig_ptr[ci + 1]) - g0;
    if (T <= 0) {
        if (lane == 0 && a.score) a.score[ci] = 0.0;
        return;
    }
    if (a.wave_tmax > 0 && T > a.wave_tmax) return;  // (the batch's long tail: decoded by the chunked kernels before this launch)
    // lanes of labels that do not exist (L < LP) repeat label 0's work: their stores then carry label 0's values, and no store
    // needs a test (a single wave issues an instruction every four cycles whatever it is: exec-mask juggling costs as much as
    // arithmetic here)
    const bool on = j < L;
    const int jj = on ? j : 0;
    double tcol[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = h * PER + k;
        tcol[k] = i < L ? a.trans[i * L + jj] : -DBL_MAX;  // (a label that does not exist never wins a strict `<`)
    }
    double *vec = vecs[wave];
    double *vout = vec + j;  // (slots of missing labels: written with label 0's value -- finite --, read against -DBL_MAX)
    const double *vin = vec + h * PER;
    const double *st = a.state + static_cast<size_t>(g0) * L + jj;
    // the contig's back-pointer quads: dwords [q * L + j], from the first dword boundary inside its T * L bytes.  Row t (1 ..
    // T - 1; gene 0 has no back-pointer) is byte (t - 1) & 3 of quad (t - 1) >> 2: the whole quads of the T - 1 rows take at
    // most (T - 1) * L bytes, the alignment at most 3 < L (this kernel serves L >= 9): every store stays inside the contig's
    // own T * L bytes, whatever kernel decodes its neighbours (split mode: the chunked kernels on the side stream).
    const size_t byte0 = (static_cast<size_t>(g0) * L + 3) & ~size_t(3);
    uint32_t *backq = reinterpret_cast<uint32_t *>(a.back + byte0) + jj;
    const bool writer = on && h == 0;
    double d = st[0];
    double nxt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) nxt[k] = 1 + k < T ? st[static_cast<size_t>(1 + k) * L] : 0.0;
    uint32_t acc = 0;  // back-pointers of the quad in progress (byte t & 3 = row t)
    // one step of [EXT] crf1dc_viterbi for target label j: delta_t[j] = max_i (delta_{t-1}[i] + trans[i][j]) + state_t[j],
    // back-pointer = the FIRST source label that attains the maximum
    auto step = [&](const int t, const double s_t, const int sh) {
        *vout = d;  // (the H lanes of a label hold the same value)
        __builtin_amdgcn_wave_barrier();
        double sc[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) sc[u] = vin[u] + tcol[u];
        __builtin_amdgcn_wave_barrier();
        double best = sc[0];
#pragma unroll
        for (int u = 1; u < PER; ++u) best = fmax(best, sc[u]);
        int arg = h * PER + PER - 1;  // the first source label of the lane's range that attains its maximum
#pragma unroll
        for (int u = PER - 2; u >= 0; --u) arg = sc[u] == best ? h * PER + u : arg;
        // merge the partial maxima of the quad's lanes, the lower source range first (ties keep the lower label)
        if (H >= 2) {
            const double ob = gl_quad_xor<1>(best);
            const int oa = gl_quad_xor<1>(arg);
            const bool take = (lane & 1) ? !(ob < best) : (best < ob);
            best = take ? ob : best;
            arg = take ? oa : arg;
        }
        if (H >= 4) {
            const double ob = gl_quad_xor<2>(best);
            const int oa = gl_quad_xor<2>(arg);
            const bool take = (lane & 2) ? !(ob < best) : (best < ob);
            best = take ? ob : best;
            arg = take ? oa : arg;
        }
        d = best + s_t;
        const uint32_t bp = uint32_t(arg);
        acc = sh == 0 ? bp : (acc | (bp << sh));
        if (sh == 24) backq[static_cast<size_t>((t - 1) >> 2) * L] = acc;  // (every lane of the label, the same dword)
    };
    int tb = 1;
    for (; tb + K <= T; tb += K) {  // whole blocks of sixteen genes: nothing to test inside
        double cur[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cur[k] = nxt[k];
        if (tb + K < T) {
            const double *sp = st + static_cast<size_t>(tb + K) * L;
#pragma unroll
            for (int k = 0; k < K; ++k) nxt[k] = tb + K + k < T ? sp[static_cast<size_t>(k) * L] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) step(tb + k, cur[k], (k & 3) * 8);  // (tb = 1 mod 16: row tb + k is byte k & 3 of its quad)
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (tb + k < T) step(tb + k, nxt[k], (k & 3) * 8);  // the last, partial block (wave-uniform tests)
    // end label = first arg max (every lane computes it: wave-uniform)
    *vout = d;
    __builtin_amdgcn_wave_barrier();
    int y = 0;
    {
        double best = -DBL_MAX;
        for (int i = 0; i < L; ++i) {
            const double v = vec[i];
            if (best < v) {
                best = v;
                y = i;
            }
        }
        if (lane == 0 && a.score) a.score[ci] = best;
    }
    y = __builtin_amdgcn_readfirstlane(y);
    int8_t *yout = a.y + g0;
    if (lane == 0) yout[T - 1] = static_cast<int8_t>(y);
    if (T == 1) return;
    __threadfence();  // (the quads this wave stored are read back through other lanes)
    // rows T - 1 .. 1; quad q = rows 4 q + 1 .. 4 q + 4; the top quad is `acc` when it is incomplete
    const int q_top = (T - 2) >> 2;
    const bool top_in_reg = ((T - 2) & 3) != 3;
    auto load_quads = [&](int q_hi, uint32_t (&w)[Q]) {  // quads q_hi - Q + 1 .. q_hi (those below 0: unused)
#pragma unroll
        for (int r = 0; r < Q; ++r) {
            const int q = q_hi - (Q - 1) + r;
            const bool stored = q >= 0 && (q < q_top || !top_in_reg);
            w[r] = (stored && writer) ? backq[static_cast<size_t>(q) * L] : 0u;
        }
    };
    uint32_t wn[Q];
    load_quads(q_top, wn);
    for (int q_hi = q_top; q_hi >= 0; q_hi -= Q) {
        uint32_t w[Q];
#pragma unroll
        for (int r = 0; r < Q; ++r) w[r] = wn[r];
        if (q_hi == q_top && top_in_reg) w[Q - 1] = acc;
        if (q_hi - Q >= 0) load_quads(q_hi - Q, wn);
#pragma unroll
        for (int r = Q - 1; r >= 0; --r) {
            const int q = q_hi - (Q - 1) + r;
            if (q < 0) continue;  // (wave-uniform)
#pragma unroll
            for (int b = 3; b >= 0; --b) {
                const int t = 4 * q + b + 1;
                if (t <= T - 1) {  // (wave-uniform)
                    const uint32_t word = uint32_t(__builtin_amdgcn_readlane(int(w[r]), y * H));  // row t as label y_t's lane holds it
                    y = int((word >> (8 * b)) & 0xffu);                                       // = label of gene t - 1
                    if (lane == 0) yout[t - 1] = static_cast<int8_t>(y);
                }
            }
        }
    }
}

// ---- row F for 17 to 32 labels, batches of many contigs: one WAVE per contig ------------------------------------------
// The same arrangement as gl_viterbi_wave for CRFsuite's scaled forward-backward recursion ([EXT] crf1dc_alpha_score /
// beta_score / marginal_point): lane (j, h) holds label j and half of the other index, the halves' partial sums meet by one DPP
// quad permute, the per-step sum over the labels (the scale factor's 1 / sum) is a DPP reduction inside the rows of sixteen
// lanes and four v_readlane across them, emissions / alpha / scale factors are staged eight or sixteen genes ahead.  A
// partial sum adds its terms in another order than the sequential loop does: results agree with the oracle to 1e-12, like
// the matrix-core kernels', not bit for bit.  log Z comes from the product of the scale factors, renormalised by frexp at every
// factor (one log per contig instead of one per gene).
template <int X>
__device__ __forceinline__ double gl_row_dpp(double v) {  // X = 0: row_half_mirror, 1: row_mirror
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), X == 0 ? 0x141 : 0x140, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), X == 0 ? 0x141 : 0x140, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// sum over the labels of a value that every label's H lanes hold alike (lanes of missing labels hold 0): the lanes with one
// value of h are one lane per label, so the permutes that would add the H copies are left out; every lane gets the sum
template <int H>
__device__ __forceinline__ double gl_wave_label_sum(double v) {
    if (H < 2) v += gl_quad_xor<1>(v);
    if (H < 4) v += gl_quad_xor<2>(v);
    v += gl_row_dpp<0>(v);  // lanes 0-7 <-> 7-0 of every half row: with the quad sums in place, the half row's
    v += gl_row_dpp<1>(v);  // ... and the row's
    auto row = [&](int l) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
    };
    const double t = (row(0) + row(16)) + (row(32) + row(48));
    return t;
}

constexpr int kWaveFK = 8;  // genes per staged block of the forward-backward walk

template <int LP>
__global__ void __launch_bounds__(kGT) gl_marginals_wave(GenArgs a) {
    constexpr int H = 64 / LP, PER = LP / H, K = kWaveFK;
    __shared__ double vecs[kGT / 64][LP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const long long ci = static_cast<long long>(blockIdx.x) * (kGT / 64) + wave;
    if (ci >= a.n_contigs) return;
    const int L = a.L, h = lane & (H - 1), j = lane / H;
    const int g0 = __builtin_amdgcn_readfirstlane(a.contig_ptr[ci]);
    const int T = __builtin_amdgcn_readfirstlane(a.contig_ptr[ci + 1]) - g0;
    if (T <= 0) {
        if (lane == 0 && a.lognorm) a.lognorm[ci] = 0.0;
        return;
    }
    if (a.wave_tmax > 0 && T > a.wave_tmax) return;  // (the batch's long tail: the chunked kernels' next to this launch)
    // lanes of labels that do not exist repeat label 0's work (their stores carry label 0's values); only the sum over the
    // labels has to leave them out
    const bool on = j < L;
    const int jj = on ? j : 0;
    double mcol[PER], mrow[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = h * PER + u;
        mcol[u] = i < L ? a.exp_trans[i * L + jj] : 0.0;
        mrow[u] = i < L ? a.exp_trans[jj * L + i] : 0.0;
    }
    double *vec = vecs[wave];
    double *vout = vec + j;
    const double *vin = vec + h * PER;
    const double *E = a.E + static_cast<size_t>(g0) * L + jj;
    const double *smax = a.smax + g0;
    double *alpha = a.alpha + static_cast<size_t>(g0) * L + jj;
    double *scale = a.scale + g0;
    double *marg = a.marg + static_cast<size_t>(g0) * L + jj;
    // ---- forward ([EXT] crf1dc_alpha_score): alpha_t[j] = (sum_i alpha_{t-1}[i] M[i][j]) E_t[j], scaled to sum 1 -- at every
    // `period`-th gene and at the last one (the recursions hold for ANY positive scale factors as long as beta uses the same
    // ones and the last alpha sums to 1: a step whose factor is 1 skips the sum over the labels and two divisions; the host
    // allows period 4 when four unscaled steps cannot leave the range, as for gl_chunk_rows_mfma)
    const int period = a.rows_rescale_period;
    double v = 0.0, c = 1.0, prod = 1.0, sm_sum = 0.0;
    int ex_sum = 0;
    double en[K], sn[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        en[k] = k < T ? E[static_cast<size_t>(k) * L] : 0.0;
        sn[k] = k < T ? smax[k] : 0.0;
    }
    const size_t stride = size_t(L);
    const double *ep = E + static_cast<size_t>(K) * L;  // next emission block
    double *ap = alpha;                                  // alpha of the gene at hand
    auto fstep = [&](const int t, const double e_t, const double sm_t) {
        if (t > 0) {
            *vout = v;
            __builtin_amdgcn_wave_barrier();
            double acc = vin[0] * mcol[0];
#pragma unroll
            for (int u = 1; u < PER; ++u) acc = fma(vin[u], mcol[u], acc);
            __builtin_amdgcn_wave_barrier();
            if (H >= 2) acc += gl_quad_xor<1>(acc);
            if (H >= 4) acc += gl_quad_xor<2>(acc);
            v = acc * e_t;
        } else {
            v = e_t;
        }
        if (period == 1 || (t & (period - 1)) == period - 1 || t == T - 1) {  // (wave-uniform)
            const double s = gl_wave_label_sum<H>(on ? v : 0.0);
            c = s != 0.0 ? 1.0 / s : 1.0;
            v *= c;
            // the product of the scale factors, renormalised at every factor: one factor is as small as (L e^(max trans))^-period,
            // e^-600 at period 4 next to its guard, and the two of a block of eight genes already left the range when the frexp
            // was taken once per block (log Z = +-inf).  frexp is exact: the bits of a log Z that was finite are what they were
            int ex;
            prod = frexp(prod * c, &ex);
            ex_sum += ex;
        } else {
            c = 1.0;
        }
        *ap = v;
        ap += stride;
        scale[t] = c;
        sm_sum += sm_t;
    };
    for (int tb = 0; tb < T; tb += K) {
        double ec[K], sc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ec[k] = en[k];
            sc[k] = sn[k];
        }
        if (tb + K < T) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                en[k] = tb + K + k < T ? ep[static_cast<size_t>(k) * L] : 0.0;
                sn[k] = tb + K + k < T ? smax[tb + K + k] : 0.0;
            }
            ep += static_cast<size_t>(K) * L;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (tb + k < T) fstep(tb + k, ec[k], sc[k]);
    }
    if (lane == 0 && a.lognorm) a.lognorm[ci] = sm_sum - (log(prod) + double(ex_sum) * 0.6931471805599453);
    // ---- backward ([EXT] crf1dc_beta_score, marginal_point): beta_t[i] = (sum_k M[i][k] E_{t+1}[k] beta_{t+1}[k]) c_t,
    // p_t[j] = alpha_t[j] beta_t[j] / c_t.  alpha / scale of step t were stored by this very lane's label (or by label 0's
    // lanes for a missing label): the fence orders them before the loads below.
    __threadfence();
    double b = c;
    marg[static_cast<size_t>(T - 1) * L] = gl_prob(v * b / c);
    if (T == 1) return;
    // step t needs alpha_t, c_t, E_{t+1}; blocks of K steps t = hi, hi - 1, ... fetched one block ahead
    double an[K], cn[K], e1n[K];
    const double *al_p = alpha + static_cast<size_t>(T - 2) * L;  // alpha_t of the next block's first step
    const double *e1_p = E + static_cast<size_t>(T - 1) * L;      // E_{t+1} likewise
    double *mp = marg + static_cast<size_t>(T - 2) * L;
    auto fetch = [&](const int hi) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = hi - k;
            an[k] = t >= 0 ? *(al_p - static_cast<size_t>(k) * L) : 0.0;
            cn[k] = t >= 0 ? scale[t] : 1.0;
            e1n[k] = t >= 0 ? *(e1_p - static_cast<size_t>(k) * L) : 0.0;
        }
        al_p -= static_cast<size_t>(K) * L;  // (never dereferenced below the contig: the tests above)
        e1_p -= static_cast<size_t>(K) * L;
    };
    fetch(T - 2);
    for (int hi = T - 2; hi >= 0; hi -= K) {
        double ac[K], cc[K], e1c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ac[k] = an[k];
            cc[k] = cn[k];
            e1c[k] = e1n[k];
        }
        if (hi - K >= 0) fetch(hi - K);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = hi - k;
            if (t >= 0) {
                *vout = b * e1c[k];
                __builtin_amdgcn_wave_barrier();
                double acc = mrow[0] * vin[0];
#pragma unroll
                for (int u = 1; u < PER; ++u) acc = fma(mrow[u], vin[u], acc);
                __builtin_amdgcn_wave_barrier();
                if (H >= 2) acc += gl_quad_xor<1>(acc);
                if (H >= 4) acc += gl_quad_xor<2>(acc);
                const double ct = cc[k];
                if (__builtin_amdgcn_readfirstlane(__double2hiint(ct)) == 0x3ff00000 && __builtin_amdgcn_readfirstlane(__double2loint(ct)) == 0) {
                    b = acc;  // (a step without rescaling: c_t = 1)
                    *mp = gl_prob(ac[k] * b);
                } else {
                    b = acc * ct;
                    *mp = gl_prob(ac[k] * b / ct);
                }
                mp -= stride;
            }
        }
    }
}

// ==================================================================================================
// Long contigs, any number of labels ("matrix-product scan for C5").  The kernels
// above give a whole contig to ONE group of lanes: a 50 000-gene contig is a 50 000-step dependent chain
// (~50 ms).  Here a contig is cut into chunks of kChunk genes and the recursions become three short
// stages, each parallel over chunks or short in steps:
//   rows    one group per (chunk, row i): row i of the chunk's transfer matrix M_c = S_first .. S_last,
//           i.e. the forward recursion started from the unit vector e_i (sum-product with exact
//           power-of-two scaling and a per-row exponent; max-plus for Viterbi).  L x the work of the
//           sequential kernel, spread over n / kChunk groups;
//   vecs    one group per contig walks its CHUNKS (n / kChunk steps instead of n): v <- v M_c forwards
//           (alpha / delta entering every chunk), b <- M_c b backwards (beta leaving every chunk: the
//           backward step matrices are the same S_t);
//   replay  one group per chunk re-runs CRFsuite's own recursion inside the chunk from its entering
//           vector: alpha / scale / marginals, or back-pointers and labels.
// Values entering a chunk come from composed matrices, so they equal the strictly sequential ones
// whenever the arithmetic is exact (integer weights: ties included) and to rounding otherwise; marginals
// are normalised by their sum inside the chunk (CRFsuite divides by the scale factor, which is the same
// number up to rounding).
constexpr int kChunk = 64;
// The exponent of a row of a chunk's sum-product matrix that is all zeros (a label whose every exp(trans) is 0: nothing
// follows it; or a row that underflowed): below every exponent a row with mass can have, so that it never sets the alignment
// maximum of chunk_walk_fwd.  With the exponent the row happened to have (0), rows of exponents under -1074 next to it were
// shifted out of the double range and the walk lost every path.  Far from INT_MIN: the walks form differences of exponents.
constexpr int kZeroRowEx = -(1 << 24);

template <int LP, bool MAXPLUS>
__global__ void __launch_bounds__(kGT) gl_chunk_rows(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const int L = a.L;
    const long long q = g.item;
    if (q >= static_cast<long long>(a.n_chunks) * L) return;
    const int ci = int(q / L), i = int(q % L);
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    const int cfirst = a.contig_ptr[a.ch_contig[ci]];  // the contig's first gene has no transition into it
    const bool on = j < L;
    const int jj = on ? j : 0;
    const double ninf = -__builtin_huge_val();
    double mcol[LP];
#pragma unroll
    for (int k = 0; k < LP; ++k) mcol[k] = (k < L && on) ? (MAXPLUS ? a.trans[k * L + j] : a.exp_trans[k * L + j]) : (MAXPLUS ? ninf : 0.0);
    const double *src = MAXPLUS ? a.state : a.E;
    double v = MAXPLUS ? (j == i ? 0.0 : ninf) : (j == i ? 1.0 : 0.0);
    int ex = 0;
    double mx = 1.0;  // (sum-product: the row's maximum after the last gene)
    double e = on ? src[static_cast<size_t>(g0) * L + jj] : (MAXPLUS ? ninf : 0.0);
    for (int t = g0; t < g1; ++t) {
        const double e_next = (t + 1 < g1 && on) ? src[static_cast<size_t>(t + 1) * L + jj] : (MAXPLUS ? ninf : 0.0);
        if (t == cfirst) {
            v = e;  // every row: the first gene forgets what entered
        } else {
            v = MAXPLUS ? max_plus(vec, j, v, mcol, L) + e : sum_product(vec, j, v, mcol) * e;
        }
        if (!MAXPLUS) {  // exact power-of-two scaling of the row, exponent kept
            mx = group_max<LP>(on ? v : 0.0);
            if (mx > 0.0) {
                int e2;
                (void)frexp(mx, &e2);
                v = ldexp(v, -e2);
                ex += e2;
            }
        }
        e = e_next;
    }
    if (on) a.chM[(static_cast<size_t>(ci) * L + i) * L + j] = v;
    if (!MAXPLUS && j == 0) a.chEx[static_cast<size_t>(ci) * L + i] = mx > 0.0 ? ex : kZeroRowEx;
}

// The same transfer matrices for 9 to 32 labels on the fp64 matrix cores.  The L rows of a chunk's matrix are L forward
// recursions from the unit vectors: sixteen of them at once are the columns of X^T in  X'^T = diag(E_t) M^T X^T  -- the step
// of gl_windowed_mfma with "sixteen windows" replaced by "sixteen start labels of one chunk": result register r of a lane IS
// its B operand of K-slice r in the next step, the slices of M^T are per-lane constants, nothing crosses lanes between steps.
// One wave per (chunk, group of sixteen rows); ceil(L / 16) * ceil(L / 4) MFMAs per gene and wave against L broadcast reads
// from LDS per lane and step in the lane-group kernel above.  A column's power-of-two rescaling (maximum over its labels:
// the lane's registers, then the four lanes that share the column) is taken every `period` steps (1, or 4 when four
// un-normalised steps cannot leave the range: 4 max|trans| < 600).  Summation order differs from gl_chunk_rows: 1e-12, not bits.
template <int TILES, int NS>
__global__ void __launch_bounds__(kGT) gl_chunk_rows_mfma(GenArgs a, const int period) {
    const int L = a.L;
    const int lane = threadIdx.x & 63, w = lane & 15, g = lane >> 4;
    const int groups = (L + 15) / 16;
    const long long wv = static_cast<long long>(blockIdx.x) * (kGT / 64) + (threadIdx.x >> 6);
    if (wv >= static_cast<long long>(a.n_chunks) * groups) return;
    const int ci = int(wv / groups), cg = int(wv % groups);
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    const int cfirst = a.contig_ptr[a.ch_contig[ci]];
    const int col = 16 * cg + w;  // the start label of this lane's column
    double Af[TILES][NS];         // slices of M^T: row = output label, column = summed label
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int sidx = 0; sidx < NS; ++sidx) {
            const int row = 16 * t + w, k = 4 * sidx + g;
            Af[t][sidx] = (row < L && k < L) ? a.exp_trans[k * L + row] : 0.0;
        }
    auto label_of = [&](int t, int r) { return 16 * t + 4 * r + g; };
    gl_v4d D[TILES], E[TILES], En[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            D[t][r] = (label_of(t, r) == col && col < L) ? 1.0 : 0.0;
            E[t][r] = label_of(t, r) < L ? a.E[static_cast<size_t>(g0) * L + label_of(t, r)] : 0.0;
        }
    int ex = 0;
    double mx_last = 1.0;  // the column's maximum at its last rescaling, which the last gene always has
    for (int gi = g0; gi < g1; ++gi) {
        // (the next gene's emissions are requested before this gene's products)
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) En[t][r] = (gi + 1 < g1 && label_of(t, r) < L) ? a.E[static_cast<size_t>(gi + 1) * L + label_of(t, r)] : 0.0;
        if (gi == cfirst) {  // every row: the contig's first gene forgets what entered
#pragma unroll
            for (int t = 0; t < TILES; ++t) D[t] = col < L ? E[t] : gl_v4d{0.0, 0.0, 0.0, 0.0};
        } else {
            gl_v4d N[TILES];
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                N[t] = gl_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int sidx = 0; sidx < NS; ++sidx) N[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t][sidx], D[sidx / 4][sidx % 4], N[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < TILES; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) D[t][r] = N[t][r] * E[t][r];
        }
        if (period <= 1 || ((gi - g0) % period) == period - 1 || gi + 1 == g1) {  // exact power-of-two scaling of the column, exponent kept
            double mx = 0.0;
#pragma unroll
            for (int t = 0; t < TILES; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmax(mx, D[t][r]);
            mx = fmax(mx, __shfl_xor(mx, 16));
            mx = fmax(mx, __shfl_xor(mx, 32));
            mx_last = mx;
            if (mx > 0.0) {
                int e2;
                (void)frexp(mx, &e2);
#pragma unroll
                for (int t = 0; t < TILES; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) D[t][r] = ldexp(D[t][r], -e2);
                ex += e2;
            }
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) E[t] = En[t];
    }
    if (col < L) {
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (label_of(t, r) < L) a.chM[(static_cast<size_t>(ci) * L + col) * L + label_of(t, r)] = D[t][r];
        if (g == 0) a.chEx[static_cast<size_t>(ci) * L + col] = mx_last > 0.0 ? ex : kZeroRowEx;
    }
}

// The walks over the chunks of a contig: forwards, the vector entering every chunk (normalised alpha / delta of the gene
// before it); backwards (marginals), beta of the last gene of every chunk up to a factor.  One group of lanes per contig
// and direction (blockIdx.y), n / chunk dependent steps.  A step is a few dozen instructions; what it waited for in
// round 2 was the load of the chunk's matrix (~0.7 us from L2/HBM per step: 41 us for the 64 chunks of the longest contig
// of a 1 000-contig batch, 0.5 ms for a 50 000-gene contig).  The matrices do not depend on the walk, so a lane fetches
// its column (row) of the next kWalkAhead chunks in one go and then takes those steps from registers.
template <int LP>
struct WalkAhead {
    static constexpr int B = LP <= 4 ? 8 : LP == 8 ? 4 : LP == 16 ? 2 : 1;
};

template <int LP, bool MAXPLUS>
__device__ __forceinline__ void chunk_walk_fwd(const GenArgs &a, long long ct, int j, double *vec) {
    constexpr int B = WalkAhead<LP>::B;
    const int L = a.L;
    const bool on = j < L;
    const double ninf = -__builtin_huge_val();
    const int c0 = a.cc_ptr[ct], c1 = a.cc_ptr[ct + 1];
    double v = MAXPLUS ? (j == 0 ? 0.0 : ninf) : (j == 0 ? 1.0 : 0.0);
    // (round 5: the columns of the NEXT B chunks are on their way while the current B steps are taken -- the round trip to
    // memory per batch of chunks was all a step waited for)
    double mn[B][LP];
    int en[B];
    auto fetch = [&](const int cb) {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int c = cb + b;
            const bool live = on && c + 1 < c1;  // (nothing leaves the contig's last chunk)
            const double *M = a.chM + static_cast<size_t>(live ? c : c0) * L * L;
#pragma unroll
            for (int k = 0; k < LP; ++k) mn[b][k] = (live && k < L) ? M[static_cast<size_t>(k) * L + j] : (MAXPLUS ? ninf : 0.0);
            en[b] = (!MAXPLUS && live) ? a.chEx[static_cast<size_t>(c) * L + j] : 0;
        }
    };
    if (c0 < c1) fetch(c0);
    for (int cb = c0; cb < c1; cb += B) {
        double mc[B][LP];
        int ex[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            ex[b] = en[b];
#pragma unroll
            for (int k = 0; k < LP; ++k) mc[b][k] = mn[b][k];
        }
        if (cb + B < c1) fetch(cb + B);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int c = cb + b;
            if (c < c1) {
                if (on) a.chV[static_cast<size_t>(c) * L + j] = v;
                if (c + 1 < c1) {
                    double w = v;
                    if (!MAXPLUS) {  // rows carry their own power-of-two exponents
                        const double exm = group_max<LP>((on && v > 0.0) ? double(ex[b]) : -1e300);
                        w = (on && v > 0.0) ? ldexp(v, ex[b] - int(exm)) : 0.0;
                    }
                    double acc = MAXPLUS ? max_plus(vec, j, w, mc[b], L) : 0.0;
                    if (!MAXPLUS) {  // (written out: this sum, alone among the forward products, leaves out the labels that do not exist)
                        vec[j] = w;
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int k = 0; k < LP; ++k)
                            if (k < L) acc = fma(vec[k], mc[b][k], acc);
                        __builtin_amdgcn_wave_barrier();
                    }
                    if (MAXPLUS) {
                        v = acc;
                    } else {
                        const double sm = group_sum<LP>(on ? acc : 0.0);
                        v = sm != 0.0 ? acc / sm : acc;
                    }
                }
            }
        }
    }
}

template <int LP>
__device__ __forceinline__ void chunk_walk_bwd(const GenArgs &a, long long ct, int j, double *vec) {
    constexpr int B = WalkAhead<LP>::B;
    const int L = a.L;
    const bool on = j < L;
    const int c0 = a.cc_ptr[ct], c1 = a.cc_ptr[ct + 1];
    double bt = 1.0;
    double mn[B][LP];
    int en[B];
    auto fetch = [&](const int cb) {  // (the rows of the next B chunks towards the front: on their way during the current steps)
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int c = cb - b;
            const bool live = on && c > c0;  // (nothing is in front of the contig's first chunk)
            const double *row = a.chM + (static_cast<size_t>(live ? c : c0) * L + (on ? j : 0)) * L;
#pragma unroll
            for (int k = 0; k < LP; ++k) mn[b][k] = (live && k < L) ? row[k] : 0.0;
            en[b] = live ? a.chEx[static_cast<size_t>(c) * L + j] : 0;
        }
    };
    if (c1 > c0) fetch(c1 - 1);
    for (int cb = c1 - 1; cb >= c0; cb -= B) {
        double mr[B][LP];
        int ex[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            ex[b] = en[b];
#pragma unroll
            for (int k = 0; k < LP; ++k) mr[b][k] = mn[b][k];
        }
        if (cb - B >= c0) fetch(cb - B);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int c = cb - b;
            if (c >= c0) {
                if (on) a.chB[static_cast<size_t>(c) * L + j] = bt;
                if (c > c0) {  // beta of the gene before the chunk = M_c beta: lane j takes row j
                    // (written out: likewise, alone among the backward products)
                    vec[j] = on ? bt : 0.0;
                    __builtin_amdgcn_wave_barrier();
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < LP; ++k)
                        if (k < L) acc = fma(mr[b][k], vec[k], acc);
                    __builtin_amdgcn_wave_barrier();
                    const double exm = group_max<LP>((on && acc > 0.0) ? double(ex[b]) : -1e300);
                    acc = (on && acc > 0.0) ? ldexp(acc, ex[b] - int(exm)) : 0.0;
                    const double mx = group_max<LP>(acc);
                    bt = mx > 0.0 ? acc / mx : 1.0;
                }
            }
        }
    }
}

template <int LP, bool MAXPLUS>
__global__ void __launch_bounds__(kGT) gl_chunk_vecs(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    const long long ct = g.item;
    if (ct >= a.n_contigs) return;
    // a contig without genes has no chunk, so none of the chunk kernels writes its log-partition / path score: 0, as the
    // contig-sequential kernels give it
    if (j == 0 && blockIdx.y == 0 && a.cc_ptr[ct + 1] == a.cc_ptr[ct] && a.wave_tmax == 0) {  // (split batches: the waves' contigs)
        if (!MAXPLUS && a.lognorm) a.lognorm[ct] = 0.0;
        if (MAXPLUS && a.score) a.score[ct] = 0.0;
    }
    if (MAXPLUS || blockIdx.y == 0)
        chunk_walk_fwd<LP, MAXPLUS>(a, ct, j, vecs + g.slot);
    else
        chunk_walk_bwd<LP>(a, ct, j, vecs + g.slot);
}

// CRFsuite's forward recursion inside a chunk, from the vector that enters it
template <int LP>
__global__ void __launch_bounds__(kGT) gl_chunk_fwd(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const int L = a.L;
    const long long ci = g.item;
    if (ci >= a.n_chunks) return;
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    const int cfirst = a.contig_ptr[a.ch_contig[ci]];
    const bool on = j < L;
    const int jj = on ? j : 0;
    double mcol[LP];
#pragma unroll
    for (int k = 0; k < LP; ++k) mcol[k] = (k < L && on) ? a.exp_trans[k * L + j] : 0.0;
    double v = on ? a.chV[static_cast<size_t>(ci) * L + j] : 0.0, z = 0.0;
    double e = on ? a.E[static_cast<size_t>(g0) * L + jj] : 0.0;
    for (int t = g0; t < g1; ++t) {
        const double e_next = (t + 1 < g1 && on) ? a.E[static_cast<size_t>(t + 1) * L + jj] : 0.0;
        if (t == cfirst) {
            v = e;
        } else {
            v = sum_product(vec, j, v, mcol) * e;
        }
        const double sm = group_sum<LP>(v);
        const double c = sm != 0.0 ? 1.0 / sm : 1.0;
        v *= c;
        if (on) a.alpha[static_cast<size_t>(t) * L + j] = v;
        if (j == 0) a.scale[t] = c;
        z += a.smax[t] - log(c);
        e = e_next;
    }
    if (j == 0) a.chZ[ci] = z;
}

// backward recursion inside a chunk + marginals
template <int LP>
__global__ void __launch_bounds__(kGT) gl_chunk_bwd(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const int L = a.L;
    const long long ci = g.item;
    if (ci >= a.n_chunks) return;
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    const bool on = j < L;
    const int jj = on ? j : 0;
    double mrow[LP];
#pragma unroll
    for (int k = 0; k < LP; ++k) mrow[k] = (k < L && on) ? a.exp_trans[j * L + k] : 0.0;
    if (a.lognorm) {  // the contig's log-partition from the chunks' partial sums: the group of its first chunk adds them up
        const int ct = a.ch_contig[ci];
        if (g0 == a.contig_ptr[ct]) {
            double z = 0.0;
            for (int c = a.cc_ptr[ct] + j; c < a.cc_ptr[ct + 1]; c += LP) z += a.chZ[c];
            z = group_sum<LP>(z);
            if (j == 0) a.lognorm[ct] = z;
        }
    }
    double b = on ? a.chB[static_cast<size_t>(ci) * L + j] : 0.0;
    for (int t = g1 - 1; t >= g0; --t) {
        const double al = on ? a.alpha[static_cast<size_t>(t) * L + j] : 0.0;
        const double x = al * b;
        const double sm = group_sum<LP>(x);
        if (on) a.marg[static_cast<size_t>(t) * L + j] = sm != 0.0 ? x / sm : 0.0;
        if (t > g0) {
            b = sum_product<true>(vec, j, on ? b * a.E[static_cast<size_t>(t) * L + jj] : 0.0, mrow) * a.scale[t - 1];  // (CRFsuite's scaling)
        }
    }
}

// Viterbi inside a chunk: back-pointers; the contig's end label and score in its last chunk
template <int LP>
__global__ void __launch_bounds__(kGT) gl_chunk_vit(GenArgs a) {
    __shared__ double vecs[kGT];
    const LaneGroup<LP> g{};
    const int j = g.j;
    double *vec = vecs + g.slot;
    const int L = a.L;
    const long long ci = g.item;
    if (ci >= a.n_chunks) return;
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    const int ct = a.ch_contig[ci];
    const int cfirst = a.contig_ptr[ct], cend = a.contig_ptr[ct + 1];
    const bool on = j < L;
    const int jj = on ? j : 0;
    double tcol[LP];
#pragma unroll
    for (int k = 0; k < LP; ++k) tcol[k] = (k < L && on) ? a.trans[k * L + j] : 0.0;
    // The margin (crf_sequence.hip, v_margin, argues it for two labels; nothing in it depends on L): the entering vector is
    // composed from chunk products, so each delta_t[j] here -- and CRFsuite's -- is within t ulp(M) of the exact maximum,
    // M = nnz max|w| + (n + 2) max|trans| bounding every partial sum of the contig's paths.  Where the best candidate of a
    // decision leads the second best by at most (4 t + 8) ulp(M), t = the gene's position in its contig, the two sides may
    // disagree: the contig is flagged and gl_viterbi_seq<FIX> decodes it again, the way CRFsuite does.
    const double ulpM = (double(a.gene_ptr[cend] - a.gene_ptr[cfirst]) * a.v_wmax + double(cend - cfirst + 2) * a.v_tmax) *
                        2.220446049250313e-16;
    bool inside = false;
    double d = on ? a.chV[static_cast<size_t>(ci) * L + j] : -DBL_MAX;
    for (int t = g0; t < g1; ++t) {
        const double s_t = on ? a.state[static_cast<size_t>(t) * L + jj] : 0.0;
        if (t == cfirst) {
            d = on ? s_t : -DBL_MAX;
            continue;
        }
        const MaxPlusArg m = max_plus_arg<LP, true>(vec, j, d, tcol, L);
        if (on) a.back[static_cast<size_t>(t) * L + j] = static_cast<uint8_t>(m.arg < 0 ? 0 : m.arg);
        inside |= on && L > 1 && m.best - m.second <= (4.0 * double(t - cfirst) + 8.0) * ulpM;
        d = m.best + s_t;
    }
    if (g1 == cend) {  // first arg max of the final scores (no product: lane 0 alone reads the slot, and nothing is written to it again)
        vec[j] = d;
        __builtin_amdgcn_wave_barrier();
        if (j == 0) {
            double best = -DBL_MAX, second = -DBL_MAX;
            int y = 0;
            for (int k = 0; k < L; ++k) {
                if (best < vec[k]) {
                    second = best;
                    best = vec[k];
                    y = k;
                } else {
                    second = fmax(second, vec[k]);
                }
            }
            a.chY[ci] = static_cast<int8_t>(y);
            if (a.score) a.score[ct] = best;
            inside |= L > 1 && best - second <= (4.0 * double(cend - cfirst) + 8.0) * ulpM;
        }
    }
    // one flag and one count per chunk with a decision inside the margin (the first such lane of the group)
    const unsigned long long bal = __ballot(inside);
    const int lane = threadIdx.x & 63, gbase = lane & ~(LP - 1);
    const unsigned long long gm = (bal >> gbase) & ((1ull << LP) - 1ull);
    if (a.fix_flag && gm && lane == gbase + __builtin_ctzll(gm)) {
        a.fix_flag[ct] = 1;
        atomicAdd(a.vit_stats + 0, 1u);
        atomicAdd(a.vit_stats + 1, 1u);
    }
}

// per chunk: label of its last gene -> label of the gene before the chunk (lane y follows the back-pointers)
template <int LP>
__global__ void __launch_bounds__(kGT) gl_chunk_maps(GenArgs a) {
    const LaneGroup<LP> g{};
    const int j = g.j;
    const int L = a.L;
    const long long ci = g.item;
    if (ci >= a.n_chunks || j >= L) return;
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    if (g0 == a.contig_ptr[a.ch_contig[ci]]) return;  // nothing before a contig's first chunk
    int y = j;
    for (int t = g1 - 1; t >= g0; --t) y = a.back[static_cast<size_t>(t) * L + y];
    a.chMap[static_cast<size_t>(ci) * L + j] = static_cast<uint8_t>(y);
}

// per contig: the label of every chunk's last gene, back to front (n / chunk dependent steps).  One wave per contig:
// the maps of up to kEndsTile / L chunks are fetched into LDS in one go (they do not depend on the walk), then lane 0
// follows them there -- a step is an LDS read (~50 ns) instead of a dependent global load (~0.7 us).
constexpr int kEndsTile = 2048;  // bytes of chunk maps per wave and round
__global__ void __launch_bounds__(kGT) gl_chunk_ends(GenArgs a) {
    __shared__ uint8_t maps[(kGT / 64) * kEndsTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ct = static_cast<long long>(blockIdx.x) * (kGT / 64) + wave;
    if (ct >= a.n_contigs) return;
    const int L = a.L;
    const int c0 = a.cc_ptr[ct], c1 = a.cc_ptr[ct + 1];
    if (c1 <= c0) return;
    uint8_t *mp = maps + wave * kEndsTile;
    const int T = kEndsTile / L;  // chunks per round
    int y = a.chY[c1 - 1];
    for (int hi = c1 - 1; hi > c0; hi -= T) {  // chunks (lo, hi] map their last label to the label before them
        const int lo = hi - T > c0 ? hi - T : c0;
        const uint8_t *src = a.chMap + static_cast<size_t>(lo + 1) * L;
        const int bytes = (hi - lo) * L;
        for (int o = lane; o < bytes; o += 64) mp[o] = src[o];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            for (int c = hi; c > lo; --c) {
                y = mp[(c - lo - 1) * L + y];
                a.chY[c - 1] = static_cast<int8_t>(y);
            }
        }
        y = __shfl(y, 0);
        __builtin_amdgcn_wave_barrier();
    }
}

// per chunk: labels of its genes from the label of its last one
__global__ void __launch_bounds__(kGT) gl_chunk_backtrack(GenArgs a) {
    const long long ci = static_cast<long long>(blockIdx.x) * kGT + threadIdx.x;
    if (ci >= a.n_chunks) return;
    const int g0 = a.ch_g0[ci], g1 = gl_chunk_end(a, ci);
    if (g1 <= g0) return;
    int y = a.chY[ci];
    a.y[g1 - 1] = static_cast<int8_t>(y);
    for (int t = g1 - 1; t > g0; --t) {
        y = a.back[static_cast<size_t>(t) * a.L + y];
        a.y[t - 1] = static_cast<int8_t>(y);
    }
}

template <int LP>
hipError_t launch_chunked(int what, const GenArgs &a, hipStream_t stream) {
    constexpr int G = LaneGroup<LP>::G;
    const int rows_period = a.rows_rescale_period;
    auto blocks = [](long long items, int per) { return dim3(group_blocks(items, per)); };
    const long long rows = static_cast<long long>(a.n_chunks) * a.L;
    if (a.n_chunks <= 0) return hipSuccess;
    if (what == 2) {
        if (LP >= 16 && a.L > 8) {  // 9 to 32 labels: sixteen rows of a chunk's transfer matrix per wave on the matrix cores
            const int groups = (a.L + 15) / 16, ns = (a.L + 3) / 4;
            const dim3 grid = blocks(static_cast<long long>(a.n_chunks) * groups, kGT / 64);
            switch (ns) {
            case 3: hipLaunchKernelGGL((gl_chunk_rows_mfma<1, 3>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            case 4: hipLaunchKernelGGL((gl_chunk_rows_mfma<1, 4>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            case 5: hipLaunchKernelGGL((gl_chunk_rows_mfma<2, 5>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            case 6: hipLaunchKernelGGL((gl_chunk_rows_mfma<2, 6>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            case 7: hipLaunchKernelGGL((gl_chunk_rows_mfma<2, 7>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            default: hipLaunchKernelGGL((gl_chunk_rows_mfma<2, 8>), grid, dim3(kGT), 0, stream, a, rows_period); break;
            }
        } else {
            hipLaunchKernelGGL((gl_chunk_rows<LP, false>), blocks(rows, G), dim3(kGT), 0, stream, a);
        }
        hipLaunchKernelGGL((gl_chunk_vecs<LP, false>), dim3(blocks(a.n_contigs, G).x, 2), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_fwd<LP>, blocks(a.n_chunks, G), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_bwd<LP>, blocks(a.n_chunks, G), dim3(kGT), 0, stream, a);
    } else {
        hipLaunchKernelGGL((gl_chunk_rows<LP, true>), blocks(rows, G), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL((gl_chunk_vecs<LP, true>), blocks(a.n_contigs, G), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_vit<LP>, blocks(a.n_chunks, G), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_maps<LP>, blocks(a.n_chunks, G), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_ends, blocks(a.n_contigs, kGT / 64), dim3(kGT), 0, stream, a);
        hipLaunchKernelGGL(gl_chunk_backtrack, blocks(a.n_chunks, kGT), dim3(kGT), 0, stream, a);
        // contigs with a decision inside the margin: CRFsuite's recursion, one group of lanes per flagged contig
        if (a.fix_flag) hipLaunchKernelGGL((gl_viterbi_seq<LP, true>), blocks(a.n_contigs, G), dim3(kGT), 0, stream, a);
    }
    return hipGetLastError();
}

template <int LP, bool kValued, bool kMasked>
void launch_state(const GenArgs &a, hipStream_t stream, const double *attr_value, const uint32_t *allowed) {
    hipLaunchKernelGGL((gl_state<LP, kValued, kMasked>), dim3(group_blocks(a.n_genes, LaneGroup<LP>::G)), dim3(kGT), 0, stream,
                       a.gene_ptr, a.attr_id, a.wtab, a.L, a.A, a.n_genes, a.state, a.E, a.smax, attr_value, allowed);
}

template <int LP>
hipError_t launch_lp(int what, const GenArgs &a, hipStream_t stream, const double *attr_value = nullptr,
                     const uint32_t *allowed = nullptr) {
    const dim3 grid(group_blocks(a.n_contigs, LaneGroup<LP>::G));
    switch (what) {
    case 0:  // state scores
        if (a.n_genes > 0) {  // (attr_value, allowed: the same for every gene of the launch)
            if (allowed) {
                if (attr_value)
                    launch_state<LP, true, true>(a, stream, attr_value, allowed);
                else
                    launch_state<LP, false, true>(a, stream, attr_value, allowed);
            } else if (attr_value) {
                launch_state<LP, true, false>(a, stream, attr_value, allowed);
            } else {
                launch_state<LP, false, false>(a, stream, attr_value, allowed);
            }
        }
        break;
    case 2:
        if (a.n_contigs > 0) hipLaunchKernelGGL(gl_marginals_seq<LP>, grid, dim3(kGT), 0, stream, a);
        break;
    case 3:
        if (a.n_contigs > 0) hipLaunchKernelGGL(gl_viterbi_seq<LP>, grid, dim3(kGT), 0, stream, a);
        break;
    }
    return hipGetLastError();
}

hipError_t launch_any(int what, const GenArgs &a, hipStream_t stream, const double *attr_value = nullptr,
                      const uint32_t *allowed = nullptr) {
    if (a.L <= 0 || a.L > kGenMaxL) return hipErrorNotSupported;
    if ((what == 2 || what == 3) && a.n_chunks > 0)  // long contigs in the batch: chunked recursions
        return dispatch_lp(a.L, [&](auto lp) { return launch_chunked<lp>(what, a, stream); });
    return dispatch_lp(a.L, [&](auto lp) { return launch_lp<lp>(what, a, stream, attr_value, allowed); });
}

}  // namespace

hipError_t launch_gen_state(const GenArgs &a, hipStream_t stream, const double *attr_value, const uint32_t *allowed) {
    return launch_any(0, a, stream, attr_value, allowed);
}
hipError_t launch_gen_marginals(const GenArgs &a, hipStream_t stream) { return launch_any(2, a, stream); }
hipError_t launch_gen_viterbi(const GenArgs &a, hipStream_t stream) { return launch_any(3, a, stream); }
hipError_t launch_gen_marginals_wave(const GenArgs &a, hipStream_t stream) {
    if (a.L <= 8 || a.L > kGenMaxL) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    const dim3 grid(group_blocks(a.n_contigs, kGT / 64));
    dispatch_wave_lp(a.L, [&](auto lp) { hipLaunchKernelGGL(gl_marginals_wave<lp>, grid, dim3(kGT), 0, stream, a); });
    return hipGetLastError();
}
hipError_t launch_gen_viterbi_wave(const GenArgs &a, hipStream_t stream) {
    if (a.L <= 8 || a.L > kGenMaxL) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    const dim3 grid(group_blocks(a.n_contigs, kGT / 64));
    dispatch_wave_lp(a.L, [&](auto lp) { hipLaunchKernelGGL(gl_viterbi_wave<lp>, grid, dim3(kGT), 0, stream, a); });
    return hipGetLastError();
}
int gen_chunk_genes() { return kChunk; }

}  // namespace gecco
