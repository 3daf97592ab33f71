// Label paths drawn from p(y | x) on the whole-contig lattice: forward filtering, backward sampling.  The
// forward-backward pass of the batch (gl_state + any arrangement of the marginals recursion, crf_general.hip) leaves its
// forward vectors in GenArgs::alpha; one pass then serves any number of draws.
//   P(y_{T-1} = i | x) ~ alpha_{T-1}(i),        P(y_t = i | y_{t+1} = j, x) ~ alpha_t(i) . exp(trans[i][j]).
// Any common positive factor of alpha_t cancels, so how an arrangement scaled its alpha does not matter (GenArgs::scale is not
// read), and with allowed masks alpha is the restricted lattice's: exactly 0 at a disallowed pair.
//
// gl_sample_paths: one lane per (contig, sample); a workgroup is one wave, the 64 consecutive samples of one contig, so
// alpha[t][0..L) is the same for every lane (the wave stages it in LDS and reads it back as broadcasts) and a step's store is
// one run of consecutive bytes of the gene-major output y[g * n_samples + s].  Each lane walks from the contig's last gene to its
// first.  At gene t, given the label j drawn at t + 1:
//   w_i = alpha_t(i) . M(i, j)   (M = exp_trans; w_i = alpha_t(i) . 1 at the last gene),   c_i = w_0 + ... + w_i in label order,
//   the label is the smallest i with c_i > u . c_{L-1}.
// c is non-decreasing, so that i is the number of labels with c_i <= u . c_{L-1}.  A label whose weight is exactly 0 has
// c_i = c_{i-1} and can never be the smallest (a disallowed label, a pair with exp(trans) = 0, an underflowed alpha).  Where
// rounding leaves no such i (u . c_{L-1} rounds to c_{L-1}) the label is the last i with w_i > 0.  The file is compiled without
// floating-point contraction: w_i is the rounded product the rule names.
//   Fallback: c_{L-1} not > 0 or not finite (every alpha_t(i) . M(i, j) is 0, or alpha holds an infinity or a NaN) is outside
// the range gecco_crf_marginals_full documents; the label is then the first arg max of marg at that gene.  No label >= L is
// ever written.
//   u: Philox4x32-10 (Salmon et al., Random123) with key (seed & 0xffffffff, seed >> 32) and counter (t = gene offset inside
// the contig, s = sample, c = contig index in the batch, 0); u = double((uint64(x0) << 21) ^ (x1 >> 11)) . 2^-53 from the
// output words x0, x1: in [0, 1), stateless, and sample s of a contig is the same whatever n_samples is.
//   alpha's address does not depend on the drawn labels: the wave fetches it in tiles of 8 genes (more below 8 labels), coalesced,
// one tile ahead of the one it walks, into two LDS buffers, padded to LP labels with zeros.  M(., j) depends on the label: up
// to 4 labels M stays in registers and the column is selected, above that M lies transposed in LDS, rows padded by one double
// so that lanes with different j read different banks.  A column of ones stands for "no gene behind" at the last gene, so
// every step is the same instruction sequence.
// A contig is one sequential walk per sample; it is not chunked (profiles/EXPERIMENTS.md has the parallel-in-T idea).
//
// gl_sample_runs: one lane per (query, sample), the lanes of a wave consecutive samples of one query (coalesced reads of the
// gene-major y).  Where sample s has a label of the mask at the anchor: the maximal run of genes around the anchor whose labels
// are all in the mask, as offsets (first, last + 1) inside the contig; else (-1, -1).
#include "crf_device.hpp"
#include "crf_lanes.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kSW = 64;          // lanes per workgroup: one wave
constexpr unsigned kMaxGridY = 65535u;

__device__ __forceinline__ double philox_uniform(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
    uint32_t c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned long long bits = (static_cast<unsigned long long>(c0) << 21) ^ static_cast<unsigned long long>(c1 >> 11);
    return static_cast<double>(bits) * 0x1p-53;
}

template <int LP>
__global__ void __launch_bounds__(kSW) gl_sample_paths(const double *__restrict__ alpha, const double *__restrict__ exp_trans,
                                                       const double *__restrict__ marg, const int32_t *__restrict__ contig_ptr,
                                                       const int L, const int n_contigs, const int n_samples, const uint32_t k0,
                                                       const uint32_t k1, int8_t *__restrict__ y) {
    constexpr bool kInRegs = LP <= 4;
    constexpr int kRow = LP + 1;
    constexpr int G = LP >= 8 ? 8 : kSW / LP;  // genes per tile of alpha
    constexpr int E = G * LP / kSW;            // tile elements per lane
    // mt[j][i] = M(i, j); row LP is the column "no gene behind": 1 for every label.  Entries at or above L are 0, as are the
    // tile's, so that the padded labels carry no weight and no step asks whether a label exists.
    __shared__ double mt[kInRegs ? 1 : (LP + 1) * kRow];
    __shared__ double tile[2][G * LP];
    double mreg[kInRegs ? LP : 1][kInRegs ? LP + 1 : 1];
    if constexpr (kInRegs) {
#pragma unroll
        for (int i = 0; i < LP; ++i) {
#pragma unroll
            for (int j = 0; j < LP; ++j) mreg[i][j] = (i < L && j < L) ? exp_trans[i * L + j] : 0.0;
            mreg[i][LP] = i < L ? 1.0 : 0.0;
        }
    } else {
        for (int k = threadIdx.x; k < (LP + 1) * LP; k += kSW) {
            const int j = k / LP, i = k - j * LP;
            mt[j * kRow + i] = i >= L ? 0.0 : j == LP ? 1.0 : j < L ? exp_trans[i * L + j] : 0.0;
        }
    }
    const int lane = threadIdx.x;
    const int s = blockIdx.x * kSW + lane;
    const bool active = s < n_samples;
    const size_t N = static_cast<size_t>(n_samples);
    for (int c = blockIdx.y; c < n_contigs; c += gridDim.y) {
        const int g0 = contig_ptr[c], T = contig_ptr[c + 1] - g0;
        if (T <= 0) continue;
        // the wave brings alpha in tiles of G genes, coalesced, a tile ahead: alpha's address does not depend on the drawn labels
        double ahead[E];
        const auto fetch = [&](int k) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int f = e * kSW + lane, r = f / LP, i = f & (LP - 1), off = k * G + r;
                ahead[e] = (i < L && off < T) ? alpha[static_cast<size_t>(g0 + off) * L + i] : 0.0;
            }
        };
        const auto put = [&](int k) {
#pragma unroll
            for (int e = 0; e < E; ++e) tile[k & 1][e * kSW + lane] = ahead[e];
        };
        const int n_tiles = (T + G - 1) / G;
        fetch(n_tiles - 1);
        put(n_tiles - 1);
        __syncthreads();  // (one wave: the tile, and before the first contig mt, are in place)
        int j = LP;       // no gene behind the last one
        for (int k = n_tiles - 1; k >= 0; --k) {
            if (k > 0) fetch(k - 1);
            const int lo = k * G, hi = T < lo + G ? T : lo + G;
            for (int t = hi - 1; t >= lo; --t) {
                const double *row = tile[k & 1] + (t - lo) * LP;
                double cs[LP], run = 0.0;
                int last = 0;
#pragma unroll
                for (int i = 0; i < LP; ++i) {
                    double m;
                    if constexpr (kInRegs) {
                        m = mreg[i][0];
#pragma unroll
                        for (int jj = 1; jj <= LP; ++jj) m = j == jj ? mreg[i][jj] : m;
                    } else {
                        m = mt[j * kRow + i];
                    }
                    const double w = row[i] * m;
                    run += w;
                    cs[i] = run;
                    last = w > 0.0 ? i : last;
                }
                const double total = cs[LP - 1];
                const double thr =
                    philox_uniform(static_cast<uint32_t>(t), static_cast<uint32_t>(s), static_cast<uint32_t>(c), k0, k1) * total;
                int lab = 0;
#pragma unroll
                for (int i = 0; i < LP; ++i) lab += cs[i] > thr ? 0 : 1;
                lab = lab >= L ? last : lab;
                if (!(total > 0.0) || !(total <= DBL_MAX)) {  // outside the documented range: the first arg max of marg
                    const double *mg = marg + static_cast<size_t>(g0 + t) * L;
                    lab = 0;
                    for (int i = 1; i < L; ++i) lab = mg[i] > mg[lab] ? i : lab;
                }
                if (active) y[static_cast<size_t>(g0 + t) * N + static_cast<size_t>(s)] = static_cast<int8_t>(lab);
                j = lab;
            }
            // (the other half was last read a tile ago, before the barrier that ended it)
            if (k > 0) put(k - 1);
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kSW) gl_sample_runs(const int8_t *__restrict__ y, const int32_t *__restrict__ contig_ptr,
                                                      const RunQuery *__restrict__ queries, const int n_runs, const int n_samples,
                                                      int32_t *__restrict__ runs) {
    const int s = blockIdx.x * kSW + threadIdx.x;
    if (s >= n_samples) return;
    const size_t N = static_cast<size_t>(n_samples);
    for (int q = blockIdx.y; q < n_runs; q += gridDim.y) {
        const RunQuery r = queries[q];
        const int g0 = contig_ptr[r.contig], T = contig_ptr[r.contig + 1] - g0;
        const int8_t *col = y + static_cast<size_t>(g0) * N + static_cast<size_t>(s);
        int first = -1, end = -1;
        if ((r.mask >> (col[static_cast<size_t>(r.anchor) * N] & 31)) & 1u) {
            first = r.anchor;
            while (first > 0 && ((r.mask >> (col[static_cast<size_t>(first - 1) * N] & 31)) & 1u)) --first;
            end = r.anchor + 1;
            while (end < T && ((r.mask >> (col[static_cast<size_t>(end) * N] & 31)) & 1u)) ++end;
        }
        reinterpret_cast<int2 *>(runs)[static_cast<size_t>(q) * N + static_cast<size_t>(s)] = make_int2(first, end);
    }
}

template <int LP>
void launch_paths(const GenArgs &a, int32_t n_samples, uint64_t seed, int8_t *y, hipStream_t stream) {
    const unsigned sblocks = (static_cast<unsigned>(n_samples) + kSW - 1) / kSW;
    const unsigned rows = static_cast<unsigned>(a.n_contigs) < kMaxGridY ? static_cast<unsigned>(a.n_contigs) : kMaxGridY;
    hipLaunchKernelGGL(gl_sample_paths<LP>, dim3(sblocks, rows), dim3(kSW), 0, stream, a.alpha, a.exp_trans, a.marg, a.contig_ptr,
                       a.L, a.n_contigs, n_samples, static_cast<uint32_t>(seed & 0xffffffffull), static_cast<uint32_t>(seed >> 32), y);
}

}  // namespace

hipError_t launch_gen_sample_paths(const GenArgs &a, int32_t n_samples, uint64_t seed, int8_t *y, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || !a.alpha || !a.marg || !y || n_samples <= 0 || n_samples > kMaxSamples)
        return hipErrorNotSupported;
    if (a.n_contigs <= 0 || a.n_genes <= 0) return hipSuccess;
    dispatch_lp(a.L, [&](auto lp) { launch_paths<lp>(a, n_samples, seed, y, stream); });
    return hipGetLastError();
}

hipError_t launch_gen_sample_runs(const GenArgs &a, const int8_t *y, const RunQuery *queries, int32_t n_runs, int32_t n_samples,
                                  int32_t *runs, hipStream_t stream) {
    if (n_runs <= 0) return hipSuccess;
    if (!y || !queries || !runs || n_samples <= 0 || n_samples > kMaxSamples) return hipErrorNotSupported;
    const unsigned sblocks = (static_cast<unsigned>(n_samples) + kSW - 1) / kSW;
    const unsigned rows = static_cast<unsigned>(n_runs) < kMaxGridY ? static_cast<unsigned>(n_runs) : kMaxGridY;
    hipLaunchKernelGGL(gl_sample_runs, dim3(sblocks, rows), dim3(kSW), 0, stream, y, a.contig_ptr, queries, n_runs, n_samples, runs);
    return hipGetLastError();
}

}  // namespace gecco
