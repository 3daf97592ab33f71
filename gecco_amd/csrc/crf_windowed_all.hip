// Every label's windowed marginal in ONE forward-backward per window (rows A/B, P, W of SURVEY.md §8a for all L labels at
// once): p_all[g][l] = max over the windows covering gene g of P_w(y_g = l), and p_any[g] = max over the same windows of
// sum_{l != background} P_w(y_g = l) -- the probability that a gene lies in ANY cluster of a type-aware cluster CRF, which
// cannot be formed from the L columns (the maximum of a sum is not a sum of maxima).
//
// The single-label kernels of crf_general.hip run the full L-label recursions and keep one component, so L labels cost L
// passes there.  Here the alpha of every label is kept, and the backward pass emits all L marginals of a position.
//
// Two tiers, chosen by the model and the window alone (never by the batch, so a contig's bits do not depend on its
// neighbours):
//   * gl_all_small<L, WMAX>, 2 to 8 labels under the range guard of gl_windowed_small: one LANE per window start, the
//     window's L x W alphas in its registers, the maxima over the covering windows as L + 1 DPP diagonals.  No atomics,
//     every output slot stored once.
//   * gl_all_groups<LP>, everything else (1 label, 9 to 32 labels, long windows, transition spreads beyond the guard): one
//     GROUP of LP lanes per window start, CRFsuite's scaled recursion (no range limit), alpha-hat of the window in LDS.
//     Maxima by integer atomicMax on the bit patterns (see there).
// Both compute a window from its own emissions and the model only, in a fixed operation order; the maxima are exact
// (fmax / integer max of non-negative doubles are commutative and associative), so the result of a gene is a pure function
// of the set of windows that cover it.  Nothing is clipped at 1: with L = 2 and background 0, p_any is column 1 bit for bit.
#include "crf_device.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kAllGT = 256;  // lanes per workgroup (lane-group tier)

template <int LP>
__device__ __forceinline__ double all_group_sum(double v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LP);
    return v;
}

// ---- lane-group tier --------------------------------------------------------------------------------------------------
// gl_windowed's recursion (crf_general.hip: CRFsuite's scaled alpha / beta, sums over the source label in index order);
// lane j of a group emits the marginal of label j at every position.  The sum over the non-background labels goes
// through LDS and is added by lane 0 in label-index order.
// Outputs: atomicMax on the 64-bit patterns.  Marginals are non-negative (products and sums of non-negative numbers), and
// non-negative doubles order like their bit patterns; the buffers start as +0.0 (all bits zero), the identity of that
// maximum.  An integer maximum is commutative and associative, so the value left in a slot is the largest candidate
// whatever order the groups arrive in.
template <int LP>
__global__ void __launch_bounds__(kAllGT) gl_all_groups(AllArgs a) {
    extern __shared__ double lds[];
    constexpr int G = kAllGT / LP;
    const int j = threadIdx.x & (LP - 1), grp = threadIdx.x / LP;
    const int W = a.W, L = a.L;
    double *al = lds + static_cast<size_t>(grp) * W * LP;         // alpha-hat of every step
    double *sc = lds + static_cast<size_t>(G) * W * LP + grp * W;  // scale factors
    double *vec = lds + static_cast<size_t>(G) * W * (LP + 1) + grp * LP;
    const long long q = static_cast<long long>(blockIdx.x) * G + grp;
    const bool active = q < a.S && ((a.start_bits[q >> 6] >> (q & 63)) & 1);
    int g0 = 0, n = 0, off = 0;
    if (active) {
        int lo = 0, hi = a.K - 1;  // scored contig owning slot q
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.c_slot[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const int s0 = a.c_slot[lo], np = a.c_slot[lo + 1] - s0;
        n = a.c_n[lo];
        g0 = a.c_gene[lo];
        off = int(q - s0) - ((np - n) >> 1);  // gene index (within the contig) of window position 0
    }
    const bool lane_on = active && j < L;
    double mcol[LP], mrow[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) {
        const bool ok = i < L && j < L;
        mcol[i] = ok ? a.exp_trans[i * L + j] : 0.0;
        mrow[i] = ok ? a.exp_trans[j * L + i] : 0.0;
    }
    // emission of window position t: padding items have no attributes -> state 0 -> exp(0 - 0) = 1
    auto emis = [&](int t) -> double {
        if (!lane_on) return 0.0;
        const int gi = off + t;
        return (gi >= 0 && gi < n) ? a.E[static_cast<size_t>(g0 + gi) * L + j] : 1.0;
    };
    double e = emis(0), v = 0.0, c = 1.0;
    for (int t = 0; t < W; ++t) {
        const double e_next = t + 1 < W ? emis(t + 1) : 0.0;
        if (t == 0) {
            v = e;
        } else {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < LP; ++i) acc = fma(al[(t - 1) * LP + i], mcol[i], acc);
            v = acc * e;
        }
        const double s = all_group_sum<LP>(v);
        c = s != 0.0 ? 1.0 / s : 1.0;
        v *= c;
        al[t * LP + j] = v;
        if (j == 0) sc[t] = c;
        e = e_next;
        __builtin_amdgcn_wave_barrier();
    }
    unsigned long long *out_all = reinterpret_cast<unsigned long long *>(a.p_all);
    unsigned long long *out_any = reinterpret_cast<unsigned long long *>(a.p_any);
    const int bg = a.background;
    double b = c;  // beta_{W-1} = scale_{W-1}
    for (int t = W - 1; t >= 0; --t) {
        const double ct = sc[t];
        if (t < W - 1) {
            vec[j] = b * emis(t + 1);
            __builtin_amdgcn_wave_barrier();
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < LP; ++i) acc = fma(mrow[i], vec[i], acc);
            b = acc * ct;
            __builtin_amdgcn_wave_barrier();
        }
        const int gi = off + t;
        const bool gene_on = active && gi >= 0 && gi < n;
        const double pr = lane_on ? al[t * LP + j] * b / ct : 0.0;
        if (lane_on && gene_on)
            atomicMax(out_all + static_cast<size_t>(g0 + gi) * L + j, static_cast<unsigned long long>(__double_as_longlong(pr)));
        if (out_any) {
            vec[j] = pr;
            __builtin_amdgcn_wave_barrier();
            if (j == 0 && gene_on) {
                double s = 0.0;  // (+0.0 + x = x for the non-negative x here: a single term keeps its bits)
                for (int i = 0; i < L; ++i)
                    if (i != bg) s += vec[i];
                atomicMax(out_any + g0 + gi, static_cast<unsigned long long>(__double_as_longlong(s)));
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ---- lane-per-window tier ------------------------------------------------------------------------------------------------
// gl_windowed_small's formulation (crf_general.hip) with the alpha of EVERY label kept: un-normalised recurrences on
// max-normalised factors (exp(state - max state), exp(trans - max trans)), alpha_k . beta_k = Z at every position, 1/Z
// folded into the initial beta, so the marginal of label j at position k is alpha_k[j] beta_k[j].  The host checks that
// W - 1 such steps cannot leave the range (all_small_ok = gen_small_ok); models beyond it take the lane-group tier.
// Sums: alpha_k[j] over the source label i in index order, beta_{k-1}[i] over the target label j in index order, Z over the
// labels in index order, the non-background sum over the labels in index order.
// The maxima over the windows covering a gene are L + 1 DPP diagonals (the running best moves one lane up per step, the
// hand-over between waves goes through LDS), as in the two-label kernel: no atomics, every output stored once by the
// workgroup that owns its slot.  A workgroup of 256 window starts owns 256 - (W - 1) output slots.
constexpr int kAllNT = kGenTileThreads;  // (the tile table is laid out by gen_small_tile_out)
__device__ __forceinline__ double all_wave_shr1_zero(double v) {  // lane l <- lane l-1, lane 0 <- +0.0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
struct AllTrans {
    double m[64];  // exp(trans - max), row-major L x L (L <= 8)
};
template <int L, int WMAX>
__global__ void __launch_bounds__(kAllNT) gl_all_small(AllArgs a, AllTrans T, const int4 *__restrict__ tile_desc) {
    constexpr int NT = kAllNT, CAP = NT + WMAX - 1, NR = L + 1;  // (NR: the L columns and the non-background sum)
    __shared__ double Es[L * CAP];   // emissions of the tile's slots, one row per label (conflict-free lane stride)
    __shared__ uint32_t ginfo[CAP];  // bit 31: a window may start here; low bits: gene + 1 (0: none)
    __shared__ double carry[(NT / 64) * WMAX * NR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.W, OUT = NT - (W - 1), ns = NT + W - 1;
    const int q0 = blockIdx.x * OUT - (W - 1);
    const int4 td = tile_desc[blockIdx.x];
    for (int sl = tid; sl < ns; sl += NT) {
        const int q = q0 + sl;
        int gene = -1;
        bool start = false;
        if (q >= 0 && q < a.S) {
            start = (a.start_bits[q >> 6] >> (q & 63)) & 1ull;
            if (td.w & 1) {
                gene = q + td.x;
            } else {
                int lo = td.y, hi = td.z;  // largest k with c_slot[k] <= q among the contigs in reach
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (a.c_slot[mid] <= q) lo = mid; else hi = mid - 1;
                }
                const int pos = q - a.c_slot[lo], np = a.c_slot[lo + 1] - a.c_slot[lo], n = a.c_n[lo];
                const int gl = pos - ((np - n) >> 1);  // delta // 2 empty items in front
                if (gl >= 0 && gl < n) gene = a.c_gene[lo] + gl;
            }
        }
#pragma unroll
        for (int j = 0; j < L; ++j)  // padding items have no attributes: state 0, exp(0 - 0) = 1
            Es[j * CAP + sl] = gene >= 0 ? a.E[size_t(gene) * L + j] : 1.0;
        ginfo[sl] = (start ? 0x80000000u : 0u) | uint32_t(gene + 1);
    }
    __syncthreads();
    const uint32_t gi = ginfo[tid];
    const bool my_start = gi >> 31;
    const int my_gene = int(gi & 0x7fffffffu) - 1;
    const double *es = Es + tid;
    const int bg = a.background;
    // forward: alpha_0 = E_0; alpha_k[j] = (sum_i alpha_{k-1}[i] M[i][j]) E_k[j]; every alpha_k stays in registers
    double al[L], AL[WMAX][L];
#pragma unroll
    for (int j = 0; j < L; ++j) AL[0][j] = al[j] = es[j * CAP];
#pragma unroll
    for (int k = 1; k < WMAX; ++k) {
        if (k < W) {
            double nx[L];
#pragma unroll
            for (int j = 0; j < L; ++j) {
                double acc = al[0] * T.m[j];
#pragma unroll
                for (int i = 1; i < L; ++i) acc = fma(al[i], T.m[i * L + j], acc);
                nx[j] = acc * es[j * CAP + k];
            }
#pragma unroll
            for (int j = 0; j < L; ++j) AL[k][j] = al[j] = nx[j];
        }
    }
    asm volatile("" ::: "memory");  // re-read the emissions in the backward pass (VGPRs)
    double z = al[0];
#pragma unroll
    for (int j = 1; j < L; ++j) z += al[j];
    double rz = __builtin_amdgcn_rcp(z);
    rz = fma(fma(-z, rz, 1.0), rz, rz);
    double be[L];
#pragma unroll
    for (int j = 0; j < L; ++j) be[j] = my_start ? rz : 0.0;  // beta_{W-1} = 1, times 1/Z; lanes that start no window: 0
    double R[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) R[r] = 0.0;
#pragma unroll
    for (int k = WMAX - 1; k >= 0; --k) {
        if (k < W) {
            double cand[NR];
#pragma unroll
            for (int j = 0; j < L; ++j) cand[j] = AL[k][j] * be[j];
            cand[L] = bg == 0 ? 0.0 : cand[0];
#pragma unroll
            for (int j = 1; j < L; ++j) cand[L] += bg == j ? 0.0 : cand[j];  // (x + 0.0 = x: a single term keeps its bits)
            if (k < W - 1) {
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (lane == 63 && wave < NT / 64 - 1) carry[(wave * WMAX + k) * NR + r] = R[r];
                    R[r] = all_wave_shr1_zero(R[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) R[r] = fmax(R[r], cand[r]);
            if (k > 0) {  // beta_{k-1}[i] = sum_j M[i][j] E_k[j] beta_k[j]
                double u[L];
#pragma unroll
                for (int j = 0; j < L; ++j) u[j] = es[j * CAP + k] * be[j];
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    double acc = T.m[i * L] * u[0];
#pragma unroll
                    for (int j = 1; j < L; ++j) acc = fma(T.m[i * L + j], u[j], acc);
                    be[i] = acc;
                }
            }
        }
    }
    __syncthreads();
    if (wave > 0 && lane < W - 1) {
#pragma unroll
        for (int r = 0; r < NR; ++r) R[r] = fmax(R[r], carry[((wave - 1) * WMAX + lane) * NR + r]);
    }
    // genes no window covers (step > 1) keep 0.0, as in the single-label kernels
    if (tid >= W - 1 && my_gene >= 0) {
#pragma unroll
        for (int j = 0; j < L; ++j) a.p_all[size_t(my_gene) * L + j] = R[j];
        if (a.p_any) a.p_any[my_gene] = R[L];
    }
}

__global__ void __launch_bounds__(256) gl_all_fill_nan(double *__restrict__ p_all, double *__restrict__ p_any, int L,
                                                       const int2 *__restrict__ ranges, int n_ranges) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int r = blockIdx.y; r < n_ranges; r += gridDim.y) {
        const int2 rg = ranges[r];
        const long long cells = static_cast<long long>(rg.y - rg.x) * L;
        for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < cells;
             i += static_cast<long long>(gridDim.x) * blockDim.x)
            p_all[static_cast<long long>(rg.x) * L + i] = nan;
        if (p_any)
            for (int g = rg.x + blockIdx.x * blockDim.x + threadIdx.x; g < rg.y; g += gridDim.x * blockDim.x) p_any[g] = nan;
    }
}

template <int LP>
hipError_t launch_groups_lp(const AllArgs &a, hipStream_t stream) {
    constexpr int G = kAllGT / LP;
    const size_t lds = (size_t(G) * a.W * (LP + 1) + kAllGT) * sizeof(double);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gl_all_groups<LP>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    const unsigned blocks = unsigned((static_cast<long long>(a.S) + G - 1) / G);
    hipLaunchKernelGGL(gl_all_groups<LP>, dim3(blocks), dim3(kAllGT), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_all_windowed_groups(const AllArgs &a, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || a.W > kGenMaxW) return hipErrorNotSupported;
    if (a.S <= 0) return hipSuccess;
    if (a.L <= 2) return launch_groups_lp<2>(a, stream);
    if (a.L <= 4) return launch_groups_lp<4>(a, stream);
    if (a.L <= 8) return launch_groups_lp<8>(a, stream);
    if (a.L <= 16) return launch_groups_lp<16>(a, stream);
    return launch_groups_lp<32>(a, stream);
}

// the lane-per-window tier keeps L x W alphas per lane: 2 to 8 labels, windows of up to 32 genes at 2 to 4 labels and of up
// to 20 beyond, under the single-label kernel's guard on the spread of the transition weights
bool all_small_ok(int L, int W, const double *trans_host) { return L <= 8 && gen_small_ok(L, W, trans_host); }

hipError_t launch_all_windowed_small(const AllArgs &a, const double *trans_host, const int4 *d_tile_desc, int ntiles,
                                     hipStream_t stream) {
    if (ntiles <= 0) return hipSuccess;
    const int L = a.L;
    if (L < 2 || L > 8) return hipErrorNotSupported;
    AllTrans T{};
    double mx = trans_host[0];
    for (int i = 0; i < L * L; ++i) mx = trans_host[i] > mx ? trans_host[i] : mx;
    for (int i = 0; i < L * L; ++i) T.m[i] = exp(trans_host[i] - mx);
    const dim3 grid(ntiles), block(kAllNT);
#define GL_ALL(LL, WW) hipLaunchKernelGGL((gl_all_small<LL, WW>), grid, block, 0, stream, a, T, d_tile_desc)
    const bool w20 = a.W <= 20;
    switch (L) {
    case 2: if (w20) GL_ALL(2, 20); else GL_ALL(2, 32); break;
    case 3: if (w20) GL_ALL(3, 20); else GL_ALL(3, 32); break;
    case 4: if (w20) GL_ALL(4, 20); else GL_ALL(4, 32); break;
    case 5: GL_ALL(5, 20); break;
    case 6: GL_ALL(6, 20); break;
    case 7: GL_ALL(7, 20); break;
    case 8: GL_ALL(8, 20); break;
    }
#undef GL_ALL
    return hipGetLastError();
}

hipError_t launch_all_fill_nan(double *p_all, double *p_any, int L, const int2 *ranges, int n_ranges, hipStream_t stream) {
    if (n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(gl_all_fill_nan, dim3(4, unsigned(n_ranges < 1024 ? n_ranges : 1024)), dim3(256), 0, stream, p_all, p_any,
                       L, ranges, n_ranges);
    return hipGetLastError();
}

}  // namespace gecco
