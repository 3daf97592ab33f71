// Windowed marginals of models with any number of labels (1 <= L <= 32): rows A/B, P, W of SURVEY.md §8a, one
// forward-backward per window, with one of two outputs (GenWinArgs::label):
//   * one label (label >= 0):  p_out[g] = max over the windows covering gene g of P_w(y_g = label);
//   * every label (label < 0): p_out[g][l] = the same for all L labels at once, and p_any[g] = max over the same windows of
//     sum_{l != background} P_w(y_g = l) -- the probability that a gene lies in ANY cluster of a type-aware cluster CRF, which
//     cannot be formed from the L columns (the maximum of a sum is not a sum of maxima).
// Every stored value lies in [0, 1]: a marginal, or a sum of marginals, that rounds to 1 + a few ulp (a label that leads by
// 800 holds all the mass; 1 + 6.7e-15 seen in p_any at 32 labels) is stored as 1, by a comparison where it is stored (gl_prob,
// crf_lanes.hpp: a NaN stays a NaN), in every tier and both outputs.  Values up to 1 keep their bits.  The sum behind p_any
// adds the stored, clipped marginals in label order and is clipped in turn, so with L = 2 and background 0 p_any is still
// column 1 bit for bit.
// Each tier states its recursion ONCE; `kAll` only chooses what is kept of it (one component of alpha and one running
// maximum, or all L and the non-background sum).  A change to a recursion is made in that one kernel body and reaches both
// outputs.  The single-label form runs the full L-label recursions and keeps one component, so L labels cost L passes
// there; the all-label form emits all L marginals of a position in one.
//
// Tiers, chosen by the model and the window alone (never by the batch, so a contig's bits do not depend on its neighbours):
//   * gl_windowed_small<L, WMAX, kAll>, 2 to 8 labels under the range guard gen_small_ok: one LANE per window start, the
//     window's vectors in its registers, the maxima over the covering windows as DPP diagonals.  No atomics, every output
//     slot stored once.  (Tier names "gl_windowed_small" / "gl_all_small".)
//   * gl_windowed_mfma<TILES, NS, WMAX>, 9 to 32 labels under the same guard, one label only: sixteen windows per wave on the
//     fp64 matrix cores.  There is no matrix-core tier for the all-label output yet.
//   * gl_windowed<LP, kAll>, everything else (1 label, long windows, transition spreads beyond the guard; every label at 9 to
//     32 labels): one GROUP of LP lanes per window start, CRFsuite's scaled recursion (no range limit), alpha-hat of the
//     window in LDS.  Maxima by integer atomicMax on the bit patterns.  (Tier names "gl_windowed" / "gl_all_groups".)
// All compute a window from its own emissions (gl_state's E = exp(state - max state), crf_general.hip) and the model only,
// in a fixed operation order; the maxima are exact (fmax / integer max of non-negative doubles are commutative and
// associative), so the result of a gene is a pure function of the set of windows that cover it.
//
// Arithmetic of the lane-group tier follows [EXT] CRFsuite crf1d_context.c in its own order (alpha: sum over the source
// label in index order, then * exp(state), then 1/sum scaling; beta: row . (beta o exp(state)) then * scale; marginal =
// alpha * beta / scale).
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cfloat>

namespace gecco {
namespace {

constexpr int kGT = 256;  // lanes per workgroup (lane-group tier)

// ---- slots -> genes ---------------------------------------------------------------------------------------------------
// Tile form (the tile kernels stage every slot of a tile once): the gene of slot q, or -1 (outside slot space, or a padding
// item), and whether a window may start there.  Regular tiles map slots to genes by a constant shift; others look the slot
// up among the contigs in reach of the tile.  (The group form -- a group owns one window start and searches all K contigs
// -- is written out in gl_windowed, its one user: as a function of its own it compiled to another schedule, one percent
// slower at 16 labels; profiles/window_general_refactor_ab.txt.)
__device__ __forceinline__ int slot_gene(const GenWinArgs &a, const int4 td, int q, bool &start) {
    int gene = -1;
    start = false;
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
            const int gl = pos - ((np - n) >> 1);  // delta // 2 empty items in front (crf/__init__.py:227)
            if (gl >= 0 && gl < n) gene = a.c_gene[lo] + gl;
        }
    }
    return gene;
}

// ---- lane-group tier: one group per window start -------------------------------------------------------------------------
// Layout: one group of lanes per window, on the frame of crf_lane_group.hpp; the forward steps read alpha-hat of the window
// where it is kept in LDS and have no exchange of their own.
// Written for up to 32 labels, it spends most of its time on that exchange (1.6 G genes/s at L = 3, 0.34 G at L = 16, 0.10 G
// at L = 32, single label).
// Outputs: atomicMax on the 64-bit patterns.  Marginals are non-negative (products and sums of non-negative numbers), and
// non-negative doubles order like their bit patterns; the buffers start as +0.0 (all bits zero), the identity of that
// maximum.  An integer maximum is commutative and associative, so the value left in a slot is the largest candidate
// whatever order the groups arrive in.
// kAll = false: lane `label` emits its marginal.  kAll = true: lane j emits the marginal of label j at every position; the
// sum over the non-background labels goes through LDS and is added by lane 0 in label-index order.
template <int LP, bool kAll>
__global__ void __launch_bounds__(kGT) gl_windowed(GenWinArgs a) {
    extern __shared__ double lds[];
    const LaneGroup<LP, kGT> g{};
    const int j = g.j, grp = g.grp;
    const int W = a.W, L = a.L;
    double *al = lds + static_cast<size_t>(grp) * W * LP;         // alpha-hat of every step
    double *sc = lds + static_cast<size_t>(g.G) * W * LP + grp * W;  // scale factors
    double *vec = lds + static_cast<size_t>(g.G) * W * (LP + 1) + grp * LP;
    const long long q = g.item;
    const bool active = q < a.S && ((a.start_bits[q >> 6] >> (q & 63)) & 1);
    int g0 = 0, n = 0, off = 0;
    if (active) {  // the scored contig owning slot q: its first gene, its number of genes
        int lo = 0, hi = a.K - 1;
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
    // forward
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
        const double s = group_sum<LP>(v);
        c = s != 0.0 ? 1.0 / s : 1.0;
        v *= c;
        al[t * LP + j] = v;
        if (j == 0) sc[t] = c;
        e = e_next;
        __builtin_amdgcn_wave_barrier();
    }
    // backward + marginals + per-gene maxima over windows
    unsigned long long *out = reinterpret_cast<unsigned long long *>(a.p_out);
    [[maybe_unused]] unsigned long long *out_any = reinterpret_cast<unsigned long long *>(a.p_any);
    [[maybe_unused]] const int bg = a.background;
    double b = c;  // beta_{W-1} = scale_{W-1}
    for (int t = W - 1; t >= 0; --t) {
        const double ct = sc[t];
        if (t < W - 1) {
            b = sum_product<true>(vec, j, b * emis(t + 1), mrow) * ct;
        }
        const int gi = off + t;
        if constexpr (!kAll) {
            if (lane_on && j == a.label && gi >= 0 && gi < n) {
                const double pr = gl_prob(al[t * LP + j] * b / ct);
                atomicMax(out + g0 + gi, static_cast<unsigned long long>(__double_as_longlong(pr)));
            }
        } else {
            const bool gene_on = active && gi >= 0 && gi < n;
            const double pr = lane_on ? gl_prob(al[t * LP + j] * b / ct) : 0.0;
            if (lane_on && gene_on)
                atomicMax(out + static_cast<size_t>(g0 + gi) * L + j, static_cast<unsigned long long>(__double_as_longlong(pr)));
            if (out_any) {
                vec[j] = pr;
                __builtin_amdgcn_wave_barrier();
                if (j == 0 && gene_on) {
                    double s = 0.0;  // (+0.0 + x = x for the non-negative x here: a single term keeps its bits)
                    for (int i = 0; i < L; ++i)
                        if (i != bg) s += vec[i];
                    atomicMax(out_any + g0 + gi, static_cast<unsigned long long>(__double_as_longlong(gl_prob(s))));
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

// ---- lane-per-window tier: a handful of labels (up to 8), the two-label kernel's design ------------------------------------
// One LANE per window start, everything of the window in its registers (crf_kernels.hip): with L <= 8 the vectors are
// L doubles, a step is L*L FMAs + L multiplications, where the lane-group tier pays for every step with an exchange
// through LDS.
//   * un-normalised recurrences on max-normalised factors (exp(state - max state): gl_state; exp(trans - max trans)):
//     alpha_k . beta_k = Z at every position of the window, so the marginal of label j at position k is
//     alpha_k[j] beta_k[j] / Z with 1/Z folded into the initial beta.  The host checks that W - 1 steps cannot leave the range
//     (gen_small_ok: spread of the transition weights * (W - 1) < 600); models beyond that take the lane-group tier.
//     Sums: alpha_k[j] over the source label i in index order, beta_{k-1}[i] over the target label j in index order, Z over
//     the labels in index order, the non-background sum over the labels in index order.
//   * kAll = false: labels are permuted so that the queried one is component 0, and only alpha_k[0] is kept (W doubles); one
//     running maximum.  kAll = true: labels in their own order, the alpha of EVERY label kept (L x W doubles), L + 1 running
//     maxima (the L columns and the non-background sum).  Every maximum is clipped at 1 when it is stored (gl_prob).
//   * the maxima over the windows that cover a gene are DPP diagonals as in the two-label kernel (the running best moves one
//     lane up per step, the hand-over between waves goes through LDS): no atomics, every output stored once by the
//     workgroup that owns its slot.
//   * a workgroup of 256 window starts owns 256 - (W - 1) output slots; the emissions of its 256 + (W - 1) slots are
//     staged in LDS once (slot_gene).
constexpr int kTileNT = kGenTileThreads;  // (the tile table is laid out by gen_small_tile_out)
struct SmallTrans {
    double m[64];  // exp(trans - max), row-major L x L (L <= 8); one label: permuted, the queried label first
};
template <int L, int WMAX, bool kAll>
__global__ void __launch_bounds__(kTileNT) gl_windowed_small(GenWinArgs a, SmallTrans T, const int4 *__restrict__ tile_desc) {
    constexpr int NT = kTileNT, CAP = NT + WMAX - 1;
    constexpr int NK = kAll ? L : 1;      // components of alpha kept for the backward pass
    constexpr int NR = kAll ? L + 1 : 1;  // running maxima (kAll: the L columns and the non-background sum)
    __shared__ double Es[L * CAP];   // emissions of the tile's slots, one row per label (conflict-free lane stride)
    __shared__ uint32_t ginfo[CAP];  // bit 31: a window may start here; low bits: gene + 1 (0: none)
    __shared__ double carry[(NT / 64) * WMAX * NR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.W, OUT = NT - (W - 1), ns = NT + W - 1;
    const int q0 = blockIdx.x * OUT - (W - 1);
    const int4 td = tile_desc[blockIdx.x];
    int perm[L];  // one label: the queried label first, the others in their own order
    perm[0] = kAll ? 0 : a.label;
#pragma unroll
    for (int j = 1; j < L; ++j) perm[j] = (!kAll && j <= a.label) ? j - 1 : j;
    for (int sl = tid; sl < ns; sl += NT) {
        bool start;
        const int gene = slot_gene(a, td, q0 + sl, start);
#pragma unroll
        for (int j = 0; j < L; ++j)  // padding items have no attributes: state 0, exp(0 - 0) = 1
            Es[j * CAP + sl] = gene >= 0 ? a.E[size_t(gene) * L + perm[j]] : 1.0;
        ginfo[sl] = (start ? 0x80000000u : 0u) | uint32_t(gene + 1);
    }
    __syncthreads();
    const uint32_t gi = ginfo[tid];
    const bool my_start = gi >> 31;
    const int my_gene = int(gi & 0x7fffffffu) - 1;
    const double *es = Es + tid;
    [[maybe_unused]] const int bg = a.background;
    // forward: alpha_0 = E_0; alpha_k[j] = (sum_i alpha_{k-1}[i] M[i][j]) E_k[j]; the kept components stay in registers
    double al[L], AL[WMAX][NK];
#pragma unroll
    for (int j = 0; j < L; ++j) al[j] = es[j * CAP];
#pragma unroll
    for (int j = 0; j < NK; ++j) AL[0][j] = al[j];
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
            for (int j = 0; j < L; ++j) al[j] = nx[j];
#pragma unroll
            for (int j = 0; j < NK; ++j) AL[k][j] = al[j];
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
            for (int j = 0; j < NK; ++j) cand[j] = AL[k][j] * be[j];
            if constexpr (kAll) {
                cand[L] = bg == 0 ? 0.0 : cand[0];
#pragma unroll
                for (int j = 1; j < L; ++j) cand[L] += bg == j ? 0.0 : cand[j];  // (x + 0.0 = x: a single term keeps its bits)
            }
            if (k < W - 1) {
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (lane == 63 && wave < NT / 64 - 1) carry[(wave * WMAX + k) * NR + r] = R[r];
                    R[r] = wave_shr1_zero(R[r]);
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
    // genes no window covers (step > 1) keep 0.0 like numpy.zeros (crf/__init__.py:251)
    if (tid >= W - 1 && my_gene >= 0) {
        if constexpr (kAll) {
#pragma unroll
            for (int j = 0; j < L; ++j) a.p_out[size_t(my_gene) * L + j] = gl_prob(R[j]);
            if (a.p_any) a.p_any[my_gene] = gl_prob(R[L]);
        } else {
            a.p_out[my_gene] = gl_prob(R[0]);
        }
    }
}

// ---- matrix-core tier, 9 to 32 labels, one label: sixteen windows per wave on the fp64 matrix cores -----------------------
// Above eight labels the L-vectors of a window no longer fit one lane's registers, and the lane-group tier pays for every
// step with L broadcast reads from LDS per lane (0.34 G genes/s at L = 16, 0.10 G at L = 32).
// A step of the recurrences over SIXTEEN windows at once is a matrix product, alpha'^T = M^T alpha^T (labels x windows):
//   v_mfma_f64_16x16x4_f64:  D (16 x 16) += A (16 x 4) B (4 x 16);  lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and
//   D[(l >> 4) + 4 r][l & 15] in its result register r   (cdna_hip_programming.md, fragment layout of the f64 form).
// With windows as columns, result register r of a lane IS its B operand of K-slice r in the next step (row (l >> 4) + 4 r of
// D = row l >> 4 of slice r of B): alpha and beta never leave their registers, nothing crosses lanes between steps, the
// slices of M^T (forward) and M (backward) are per-lane constants.  Per step and 16 windows: ceil(L / 16) * ceil(L / 4)
// MFMAs + one multiplication by the emission per register.
//   * formulation of gl_windowed_small: un-normalised recurrences on max-normalised factors, alpha_k . beta_k = Z at every
//     position, 1 / Z folded into the initial beta, queried label permuted to component 0 (lanes 0-15 of a wave own its
//     alpha_k: W doubles per lane), same range guard on the transition weights (gen_small_ok).  The summation order of a
//     step differs from CRFsuite's (four terms per MFMA, in hardware order): results agree with the oracle to 1e-12, as
//     the other kernels of this file do, not bit for bit.
//   * the maximum over the windows that cover a gene: returnless LDS atomics (ds_max_u64 on the bit pattern of the
//     non-negative candidate) on best[slot] -- sixteen lanes per step, next to 4-16 MFMAs: the LDS port is idle here (in
//     the two-label kernel, where a step is seven VALU instructions, the same atomics lose: profiles/r04_window_kernel_ab.txt).
//   * a workgroup = 256 window starts (4 waves x 4 batches of 16) owning 256 - (W - 1) output slots, emissions staged once
//     in LDS, one row per label with a stride that keeps the 16 x 4 lanes of a read on distinct banks.
__host__ __device__ constexpr int gl_mfma_stride(int wmax) { return ((kTileNT + wmax - 1 + 15) / 32) * 32 + 16; }  // = 16 mod 32, >= slots
template <int TILES, int NS, int WMAX>
__global__ void __launch_bounds__(kTileNT) gl_windowed_mfma(GenWinArgs a, double tmax, const int4 *__restrict__ tile_desc) {
    constexpr int NT = kTileNT, S = gl_mfma_stride(WMAX);
    extern __shared__ double gl_dyn[];
    const int L = a.L;
    double *Es = gl_dyn;                                                       // [L][S] emissions, label-major
    unsigned long long *best = reinterpret_cast<unsigned long long *>(gl_dyn + size_t(L) * S);  // [NT + WMAX]
    uint32_t *ginfo = reinterpret_cast<uint32_t *>(best + NT + WMAX);          // [NT + WMAX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = lane & 15, g = lane >> 4;
    const int W = a.W, OUT = NT - (W - 1), ns = NT + W - 1;
    const int q0 = blockIdx.x * OUT - (W - 1);
    const int4 td = tile_desc[blockIdx.x];
    auto perm = [&](int j) { return j == 0 ? a.label : (j <= a.label ? j - 1 : j); };  // queried label first
    // per-lane constants: slices of M^T (forward: row = output label, column = input label) and of M (backward)
    double Af[TILES][NS], Ab[TILES][NS];
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int sidx = 0; sidx < NS; ++sidx) {
            const int row = 16 * t + w, col = 4 * sidx + g;  // (row: label on the matrix side of the product, col: the summed label)
            const bool ok = row < L && col < L;
            Af[t][sidx] = ok ? exp(a.trans[perm(col) * L + perm(row)] - tmax) : 0.0;  // M^T[row][col] = M[col][row]
            Ab[t][sidx] = ok ? exp(a.trans[perm(row) * L + perm(col)] - tmax) : 0.0;
        }
    // ---- stage 1: slots -> genes, emissions -> LDS (consecutive lanes read consecutive doubles of the [gene][label] array)
    for (int sl = tid; sl < NT + WMAX; sl += NT) {
        int gene = -1;
        bool start = false;
        if (sl < ns) gene = slot_gene(a, td, q0 + sl, start);
        ginfo[sl] = (start ? 0x80000000u : 0u) | uint32_t(gene + 1);
        best[sl] = 0ull;
    }
    __syncthreads();
    for (int idx = tid; idx < ns * L; idx += NT) {
        const int sl = idx / L, j = idx - sl * L;
        const int gene = int(ginfo[sl] & 0x7fffffffu) - 1;
        // (j-th label of the gene's row in memory = permuted component pj: component 0 is the queried label)
        const int pj = j == a.label ? 0 : (j < a.label ? j + 1 : j);
        Es[pj * S + sl] = gene >= 0 ? a.E[size_t(gene) * L + j] : 1.0;  // padding items have no attributes: exp(0 - 0) = 1
    }
    __syncthreads();
    // the emission of (component of result register r of tile t, this lane's window, step k); components >= L: any finite
    // number (their alpha / beta are exact zeros: the matrix rows are)
    auto em = [&](int t, int r, int slot) { return Es[min(16 * t + 4 * r + g, L - 1) * S + slot]; };
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
        const int sl0 = wave * 64 + b * 16 + w;  // slot of this lane's window start
        gl_v4d D[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) D[t][r] = (16 * t + 4 * r + g) < L ? em(t, r, sl0) : 0.0;
        double A0[WMAX];
        A0[0] = D[0][0];
#pragma unroll
        for (int k = 1; k < WMAX; ++k) {
            if (k < W) {
                gl_v4d N[TILES];
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    N[t] = gl_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int sidx = 0; sidx < NS; ++sidx)
                        N[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t][sidx], D[sidx / 4][sidx % 4], N[t], 0, 0, 0);
                }
#pragma unroll
                for (int t = 0; t < TILES; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) D[t][r] = N[t][r] * em(t, r, sl0 + k);
                A0[k] = D[0][0];
            }
        }
        // Z of the lane's window: all components, i.e. all registers of the four lanes w, w + 16, w + 32, w + 48
        double z = 0.0;
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) z += D[t][r];
        z += __shfl_xor(z, 16);
        z += __shfl_xor(z, 32);
        double rz = __builtin_amdgcn_rcp(z);
        rz = fma(fma(-z, rz, 1.0), rz, rz);
        const bool my_start = ginfo[sl0] >> 31;
        gl_v4d B[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) B[t][r] = (my_start && (16 * t + 4 * r + g) < L) ? rz : 0.0;  // beta_{W-1} = 1, times 1/Z
#pragma unroll
        for (int k = WMAX - 1; k >= 0; --k) {
            if (k < W) {
                const double cand = A0[k] * B[0][0];  // lanes 0-15: component 0 = the queried label
                if (g == 0)
                    (void)__hip_atomic_fetch_max(best + sl0 + k, static_cast<unsigned long long>(__double_as_longlong(cand)),
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (k > 0) {  // beta_{k-1} = M (E_k o beta_k)
                    gl_v4d U[TILES], N[TILES];
#pragma unroll
                    for (int t = 0; t < TILES; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) U[t][r] = B[t][r] * em(t, r, sl0 + k);
#pragma unroll
                    for (int t = 0; t < TILES; ++t) {
                        N[t] = gl_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int sidx = 0; sidx < NS; ++sidx)
                            N[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ab[t][sidx], U[sidx / 4][sidx % 4], N[t], 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < TILES; ++t) B[t] = N[t];
                }
            }
        }
    }
    __syncthreads();
    const int my_gene = int(ginfo[tid] & 0x7fffffffu) - 1;
    // genes no window covers (step > 1) keep 0.0 like numpy.zeros (crf/__init__.py:251)
    if (tid >= W - 1 && my_gene >= 0) a.p_out[my_gene] = gl_prob(__longlong_as_double(static_cast<long long>(best[tid])));
}

// NaN ("no prediction") in the `cols` columns of p and in p_any (may be null) for the gene ranges of skipped contigs
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

template <int LP, bool kAll>
hipError_t launch_groups(const GenWinArgs &a, hipStream_t stream) {
    constexpr int G = LaneGroup<LP, kGT>::G;
    const size_t lds = (size_t(G) * a.W * (LP + 1) + kGT) * sizeof(double);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gl_windowed<LP, kAll>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    const unsigned blocks = group_blocks(a.S, G);
    hipLaunchKernelGGL((gl_windowed<LP, kAll>), dim3(blocks), dim3(kGT), lds, stream, a);
    return hipGetLastError();
}
template <int LP>
hipError_t launch_groups_lp(const GenWinArgs &a, hipStream_t stream) {
    return a.label < 0 ? launch_groups<LP, true>(a, stream) : launch_groups<LP, false>(a, stream);
}

}  // namespace

hipError_t launch_gen_windowed(const GenWinArgs &a, hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || a.W > kGenMaxW) return hipErrorNotSupported;
    if (a.S <= 0) return hipSuccess;
    if (a.L <= 2) return launch_groups_lp<2>(a, stream);
    if (a.L <= 4) return launch_groups_lp<4>(a, stream);
    if (a.L <= 8) return launch_groups_lp<8>(a, stream);
    if (a.L <= 16) return launch_groups_lp<16>(a, stream);
    return launch_groups_lp<32>(a, stream);
}

int gen_small_tile_out(int W) { return kTileNT - (W - 1); }

// the lane-per-window kernel takes 3 to 8 labels (2 too: tests), windows of up to 32 genes (20 beyond 4 labels: W doubles of
// alpha per lane next to four L-vectors) and transition weights whose spread cannot take W - 1 un-normalised steps out
// of the range
bool gen_small_ok(int L, int W, const double *trans_host) {
    // (9 to 32 labels: the matrix-core kernel, same geometry and range guard, windows of up to 32 genes)
    if (L < 2 || L > kGenMaxL || W < 1 || W > (L <= 4 || L > 8 ? 32 : 20) || !trans_host) return false;
    double lo = trans_host[0], hi = trans_host[0];
    for (int i = 0; i < L * L; ++i) {
        lo = trans_host[i] < lo ? trans_host[i] : lo;
        hi = trans_host[i] > hi ? trans_host[i] : hi;
    }
    return hi - lo == hi - lo && (hi - lo) * double(W - 1) < 600.0;  // (finite)
}
// every label: the lane-per-window tier keeps L x W alphas per lane, 2 to 8 labels under the same guard (no matrix-core tier)
bool all_small_ok(int L, int W, const double *trans_host) { return L <= 8 && gen_small_ok(L, W, trans_host); }

hipError_t launch_gen_windowed_small(const GenWinArgs &a, const double *trans_host, const int4 *d_tile_desc, int ntiles,
                                     hipStream_t stream) {
    if (ntiles <= 0) return hipSuccess;
    const int L = a.L;
    const bool all = a.label < 0;
    if (L < 2 || L > (all ? 8 : kGenMaxL)) return hipErrorNotSupported;
    double mx = trans_host[0];
    for (int i = 0; i < L * L; ++i) mx = trans_host[i] > mx ? trans_host[i] : mx;
    if (L > 8) {  // sixteen windows per wave on the fp64 matrix cores
        const int wmax = a.W <= 20 ? 20 : 32, ns = (L + 3) / 4;
        const size_t lds = size_t(L) * gl_mfma_stride(wmax) * 8 + size_t(kTileNT + wmax) * 12;
        hipError_t attr_rc = hipSuccess;
#define GL_MFMA(TT, NN)                                                                                                              \
    do {                                                                                                                             \
        if (wmax == 20) {                                                                                                            \
            attr_rc = hipFuncSetAttribute(reinterpret_cast<const void *>(&gl_windowed_mfma<TT, NN, 20>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)); \
            if (attr_rc != hipSuccess) return attr_rc; /* (a device whose LDS cannot hold L label rows of a tile: fail loudly) */ \
            hipLaunchKernelGGL((gl_windowed_mfma<TT, NN, 20>), dim3(ntiles), dim3(kTileNT), lds, stream, a, mx, d_tile_desc);        \
        } else {                                                                                                                     \
            attr_rc = hipFuncSetAttribute(reinterpret_cast<const void *>(&gl_windowed_mfma<TT, NN, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)); \
            if (attr_rc != hipSuccess) return attr_rc;                                                                               \
            hipLaunchKernelGGL((gl_windowed_mfma<TT, NN, 32>), dim3(ntiles), dim3(kTileNT), lds, stream, a, mx, d_tile_desc);        \
        }                                                                                                                            \
    } while (0)
        switch (ns) {
        case 3: GL_MFMA(1, 3); break;
        case 4: GL_MFMA(1, 4); break;
        case 5: GL_MFMA(2, 5); break;
        case 6: GL_MFMA(2, 6); break;
        case 7: GL_MFMA(2, 7); break;
        case 8: GL_MFMA(2, 8); break;
        default: return hipErrorNotSupported;
        }
#undef GL_MFMA
        return hipGetLastError();
    }
    SmallTrans T{};
    int perm[8];  // one label: the queried label first, the others in their own order
    perm[0] = all ? 0 : a.label;
    for (int j = 1; j < L; ++j) perm[j] = (!all && j <= a.label) ? j - 1 : j;
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) T.m[i * L + j] = exp(trans_host[perm[i] * L + perm[j]] - mx);
    const dim3 grid(ntiles), block(kTileNT);
#define GL_SMALL(LL, WW)                                                                                         \
    do {                                                                                                         \
        if (all)                                                                                                 \
            hipLaunchKernelGGL((gl_windowed_small<LL, WW, true>), grid, block, 0, stream, a, T, d_tile_desc);    \
        else                                                                                                     \
            hipLaunchKernelGGL((gl_windowed_small<LL, WW, false>), grid, block, 0, stream, a, T, d_tile_desc);   \
    } while (0)
    const bool w20 = a.W <= 20;
    switch (L) {
    case 2: if (w20) GL_SMALL(2, 20); else GL_SMALL(2, 32); break;
    case 3: if (w20) GL_SMALL(3, 20); else GL_SMALL(3, 32); break;
    case 4: if (w20) GL_SMALL(4, 20); else GL_SMALL(4, 32); break;
    case 5: GL_SMALL(5, 20); break;
    case 6: GL_SMALL(6, 20); break;
    case 7: GL_SMALL(7, 20); break;
    case 8: GL_SMALL(8, 20); break;
    }
#undef GL_SMALL
    return hipGetLastError();
}

hipError_t launch_all_fill_nan(double *p_all, double *p_any, int L, const int2 *ranges, int n_ranges, hipStream_t stream) {
    if (n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(gl_all_fill_nan, dim3(4, unsigned(n_ranges < 1024 ? n_ranges : 1024)), dim3(256), 0, stream, p_all, p_any,
                       L, ranges, n_ranges);
    return hipGetLastError();
}

}  // namespace gecco
