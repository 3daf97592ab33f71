// Lane-level moves and reductions of the any-L kernels (crf_general.hip, crf_general_windowed.hip): a reduction over a
// group of LP consecutive lanes (LP a power of two, a group never straddles a wave) and the one-lane shift of the DPP
// diagonals, and the accumulator type of the fp64 matrix-core kernels.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

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

typedef double gl_v4d __attribute__((ext_vector_type(4)));  // the four result registers of v_mfma_f64_16x16x4_f64

}  // namespace
}  // namespace gecco
