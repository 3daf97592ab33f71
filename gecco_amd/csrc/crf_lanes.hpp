// Lane-level moves and reductions of the any-L kernels (crf_general.hip, crf_general_windowed.hip): a reduction over a
// group of LP consecutive lanes (LP a power of two, a group never straddles a wave) and the one-lane shift of the DPP
// diagonals, the clip of a stored probability, and the accumulator type of the fp64 matrix-core kernels.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace gecco {
namespace {

// every lane of a group gets the group's sum / maximum (butterfly: the same order of additions in every lane)
template <int LP>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LP);
    return v;
}
template <int LP>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, LP));
    return v;
}

__device__ __forceinline__ double wave_shr1_zero(double v) {  // lane l <- lane l-1, lane 0 <- +0.0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// alpha beta / c (or alpha beta / Z, or a sum of such) as a stored probability.  Where one label holds all the mass the
// quotient can round to 1 + a few ulp (1 + 3.5e-15 seen on a whole contig, 1 + 6.7e-15 in a window, with a label that leads by
// 800): at most 1 is stored.  A comparison, not fmin: a NaN stays a NaN.
__device__ __forceinline__ double gl_prob(double x) { return x > 1.0 ? 1.0 : x; }

typedef double gl_v4d __attribute__((ext_vector_type(4)));  // the four result registers of v_mfma_f64_16x16x4_f64

// Host side: the group width of a model of L labels (1 .. 32) -- the next power of two, 2 at the least -- as a constant:
// f(std::integral_constant<int, LP>{}).  Every launcher of a kernel templated on LP picks its instance here.
template <class F>
auto dispatch_lp(int L, F &&f) {
    if (L <= 2) return f(std::integral_constant<int, 2>{});
    if (L <= 4) return f(std::integral_constant<int, 4>{});
    if (L <= 8) return f(std::integral_constant<int, 8>{});
    if (L <= 16) return f(std::integral_constant<int, 16>{});
    return f(std::integral_constant<int, 32>{});
}
// the same for the wave-per-contig kernels (gl_marginals_wave, gl_viterbi_wave: 9 to 32 labels), which have two instances
template <class F>
auto dispatch_wave_lp(int L, F &&f) {
    if (L <= 16) return f(std::integral_constant<int, 16>{});
    return f(std::integral_constant<int, 32>{});
}

}  // namespace
}  // namespace gecco
