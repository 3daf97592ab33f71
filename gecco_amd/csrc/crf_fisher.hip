// Two-sided Fisher exact test over a batch of 2x2 tables in fp64 (gecco_crf_fisher_exact).
//
// Semantics: scipy.stats.fisher_exact(table, alternative="two-sided") as of scipy 1.15, which GECCO's feature selection
// calls once per domain (gecco/crf/select.py).  For [[a, b], [c, d]] the count a follows the hypergeometric law of n = a + c
// draws from N = a + b + c + d items of which K = a + b are marked; its support is [max(0, n - (c + d)), min(n, K)] and
// mode = int((n + 1) * (K + 1) / (N + 2)) (computed as scipy computes it, in floating point).
//   * a zero row or column sum gives exactly 1.0;
//   * pmf(a) within a relative 1e-14 of pmf(mode) gives exactly 1.0;
//   * otherwise p = every term from a outward on a's side of the mode, plus every term on the other side whose pmf is at
//     most pmf(a) * (1 + 1e-14); then min(p, 1.0).
//
// Algorithm.  One wave per table.  Only ratios to the mode are formed: L(k) = log(pmf(k) / pmf(mode)) is the prefix sum,
// outward from the mode, of the per-step logs log(pmf(k +- 1) / pmf(k)), and p = (sum of the selected exp(L)) / (sum of all
// exp(L)), so pmf(mode) itself (a ~10^7-nat lgamma difference at N ~ 10^6) is never needed.  A step's ratio is P / Q with
// P, Q exact int64 products of two factors below 2^31; its log is log1p((P - Q) / Q) when P / Q >= 1/2 (accurate near the
// mode, where the steps are tiny) and log(P / Q) below.  Each side is walked in chunks of 64 steps: one step per lane, an
// inclusive double-double scan across the wave (fixed Hillis-Steele order), plus the carry of the chunk before.  The error of
// L(k) is then a few ulps of |L(k)|: every step's log is accurate to ~3 ulps of itself and all steps of a side share a sign.
// a's side is walked first (it yields L(a)); a side stops once its last term is below 2^-60 of both the running total and
// pmf(a) (the terms fall faster than geometrically away from the mode), or at the end of the support.  The work per table is
// therefore about the spread of the distribution, not its support.  If a's side falls below e^-720 of the mode before a is
// reached, p < 2^31 e^-720 < 1e-300 and the result is 0.
//
// The tie rule.  A term on the other side is included when L(k) <= L(a) + 1e-14 + |L(a)| * 2^-50.  The scipy tolerance alone
// (1e-14) is not enough where L carries a few ulps of error; the extra 4 ulps of |L(a)| are.  Terms that are mathematically
// equal arise from the two symmetries of the hypergeometric law: K = N / 2 (k <-> n - k) and n = N / 2 (k <-> K - k).  In both,
// the step from the mode outward by j on one side and the mirrored step on the other have the same (P, Q) integer pair (the
// factors of the two products swap places, and integer products commute), so the step logs are bit-identical, and with the
// mode at the centre the two scans run in the same order on the same values: equal L bits.  With an odd span the mode is one
// of two equal terms and the other side's scan starts with an exact log(1) = 0, shifting its alignment by one lane; the
// double-double sums then agree to ~2^-100 and their rounded values to within an ulp, inside the tolerance.  The cost is that a
// mathematically larger term within 4 ulps of |L(a)| (6.6e-13 relative at most) counts as a tie; scipy's own pmf error is of
// that order there.
//
// Range: non-negative cells with a total up to 2^31 - 1 (checked on the host: every product of two factors fits int64).
// Accuracy: relative 1e-10 against scipy where p >= 1e-280, both below 1e-250 under it; scipy itself is up to ~3e-9 off at
// N ~ 10^7, and there the result matches the exact value to 1e-12.  A table's bits depend only on the
// table: its wave does the same operations in the same order wherever the table sits in the batch.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "../../include/gecco_crf.h"
#include "crf_fisher.hpp"
#include "crf_model.hpp"
#include "crf_plan.hpp"

namespace gecco {

namespace {

constexpr int kFisherWave = 64;
constexpr int kFisherWavesPerBlock = 4;
constexpr int64_t kFisherMaxBlocks = 1 << 16;  // grid-stride beyond 2^18 tables
constexpr double kFisherStop = 42.0;           // e^-42 < 2^-60
constexpr double kFisherZeroCut = -720.0;      // a's side below e^-720 of the mode before a: p = 0
constexpr double kFisherUnderflow = -746.0;    // exp() is 0 below
constexpr double kScipyEps = 1e-14;

struct DD {
    double hi, lo;
};

__device__ inline DD dd_add(DD a, DD b) {
    const double s = a.hi + b.hi;
    const double bb = s - a.hi;
    double e = (a.hi - (s - bb)) + (b.hi - bb);
    e += a.lo + b.lo;
    const double h = s + e;
    return {h, e - (h - s)};
}

__device__ inline double wave_sum(double v) {
    for (int o = kFisherWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return __shfl(v, 0);  // (lane 0's order: the same bits whatever the lanes computed)
}

// log(pmf(k0 + dir) / pmf(k0)); M = N - K - n.  Factors are below 2^31, so P, Q < 2^62 are exact.
__device__ inline double fisher_step(int64_t K, int64_t n, int64_t M, int64_t k0, int dir) {
    int64_t P, Q;
    if (dir > 0) {
        P = (K - k0) * (n - k0);
        Q = (k0 + 1) * (M + k0 + 1);
    } else {
        P = k0 * (M + k0);
        Q = (K - k0 + 1) * (n - k0 + 1);
    }
    if (2 * P < Q) return log(double(P) / double(Q));
    return log1p(double(P - Q) / double(Q));
}

// One side of the mode: steps s = 0 .. len - 1 reach k = m + dir * (s + 1).  On a's side (da = |a - m| > 0) the terms from a
// outward are selected and L(a) is captured; on the other side (da = 0) the terms with L <= thr.  Returns false when a's side
// proves p = 0.
__device__ bool fisher_walk(int lane, int64_t K, int64_t n, int64_t M, int64_t m, int dir, int64_t len, int64_t da, double thr,
                            double &total, double &incl, double &La) {
    DD carry{0.0, 0.0};
    for (int64_t base = 0; base < len; base += kFisherWave) {
        const int64_t s = base + lane;
        const bool valid = s < len;
        DD x{valid ? fisher_step(K, n, M, m + dir * s, dir) : 0.0, 0.0};
        for (int d = 1; d < kFisherWave; d <<= 1) {
            const DD y{__shfl_up(x.hi, d), __shfl_up(x.lo, d)};
            if (lane >= d) x = dd_add(y, x);
        }
        const DD L = dd_add(carry, x);
        const bool reached = base + kFisherWave >= da;
        if (da > 0 && reached && base < da) La = __shfl(L.hi, int(da - 1 - base));
        const double e = valid ? exp(L.hi) : 0.0;
        const bool take = valid && (da > 0 ? s >= da - 1 : L.hi <= thr);
        total += wave_sum(e);
        incl += wave_sum(take ? e : 0.0);
        const int64_t last = len - 1 - base < kFisherWave - 1 ? len - 1 - base : kFisherWave - 1;
        const double Llast = __shfl(L.hi, int(last));
        if (!reached && Llast < kFisherZeroCut) return false;
        if (reached && (Llast < fmin(log(total), La) - kFisherStop || Llast < kFisherUnderflow)) break;
        carry = DD{__shfl(L.hi, kFisherWave - 1), __shfl(L.lo, kFisherWave - 1)};
    }
    return true;
}

__device__ double fisher_one(const int64_t *__restrict__ tab, int lane) {
    const int64_t a = tab[0], b = tab[1], c = tab[2], d = tab[3];
    const int64_t K = a + b, n2 = c + d, n = a + c;
    if (K == 0 || n2 == 0 || n == 0 || b + d == 0) return 1.0;
    const int64_t N = K + n2, M = n2 - n;
    const int64_t lo = n - n2 > 0 ? n - n2 : 0, hi = n < K ? n : K;
    int64_t m = static_cast<int64_t>(double((n + 1) * (K + 1)) / double(N + 2));
    m = m < lo ? lo : (m > hi ? hi : m);
    if (a == m) return 1.0;
    const int dir = a > m ? 1 : -1;
    double total = 1.0, incl = 0.0, La = 0.0;
    if (!fisher_walk(lane, K, n, M, m, dir, dir > 0 ? hi - m : m - lo, dir > 0 ? a - m : m - a, 0.0, total, incl, La))
        return 0.0;
    if (fabs(expm1(La)) <= kScipyEps * fmax(1.0, exp(La))) return 1.0;
    const double thr = La + kScipyEps + fabs(La) * 0x1p-50;
    fisher_walk(lane, K, n, M, m, -dir, dir > 0 ? m - lo : hi - m, 0, thr, total, incl, La);
    const double p = incl / total;
    return p < 1.0 ? p : 1.0;
}

__global__ void __launch_bounds__(kFisherWave *kFisherWavesPerBlock)
    fisher_kernel(const int64_t *__restrict__ tables, int64_t n_tables, double *__restrict__ pvalue) {
    const int lane = threadIdx.x % kFisherWave;
    const int64_t stride = int64_t(gridDim.x) * kFisherWavesPerBlock;
    for (int64_t t = int64_t(blockIdx.x) * kFisherWavesPerBlock + threadIdx.x / kFisherWave; t < n_tables; t += stride) {
        const double p = fisher_one(tables + 4 * t, lane);
        if (lane == 0) pvalue[t] = p;
    }
}

int fail(const std::string &msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

}  // namespace

int fisher_check(const int64_t *tables, int64_t n, const double *pvalue) {
    if (n < 0) return fail("fisher_exact: n must be >= 0");
    if (n == 0) return GECCO_CRF_OK;
    if (!tables || !pvalue) return fail("fisher_exact: null buffer");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t *t = tables + 4 * i;
        if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[3] < 0)
            return fail("fisher_exact: table " + std::to_string(i) + " has a negative cell");
        if (t[0] > INT32_MAX || t[1] > INT32_MAX || t[2] > INT32_MAX || t[3] > INT32_MAX ||
            t[0] + t[1] + t[2] + t[3] > INT32_MAX)
            return fail("fisher_exact: the total of table " + std::to_string(i) + " exceeds 2^31 - 1");
    }
    return GECCO_CRF_OK;
}

int fisher_exact(int32_t device, const int64_t *tables, int64_t n, double *pvalue) {
    int rc = set_device(device);
    if (rc) return rc;
    Stream stream;
    DeviceBlock<int64_t> d_tables;
    DeviceBlock<double> d_p;
    if ((rc = stream.create())) return rc;
    if ((rc = d_tables.alloc(size_t(n) * 4, "fisher alloc"))) return rc;
    if ((rc = d_p.alloc(size_t(n), "fisher alloc"))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(d_tables.get(), tables, size_t(n) * 4 * sizeof(int64_t), hipMemcpyHostToDevice, stream.get()),
                        "fisher upload")))
        return rc;
    const int64_t want = (n + kFisherWavesPerBlock - 1) / kFisherWavesPerBlock;
    const unsigned blocks = unsigned(want < kFisherMaxBlocks ? want : kFisherMaxBlocks);
    fisher_kernel<<<blocks, kFisherWave * kFisherWavesPerBlock, 0, stream.get()>>>(d_tables.get(), n, d_p.get());
    if ((rc = check_hip(hipGetLastError(), "fisher kernel"))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(pvalue, d_p.get(), size_t(n) * sizeof(double), hipMemcpyDeviceToHost, stream.get()),
                        "fisher download")))
        return rc;
    return check_hip(hipStreamSynchronize(stream.get()), "fisher synchronize");
}

}  // namespace gecco
