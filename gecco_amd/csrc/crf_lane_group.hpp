// The frame of the any-label kernels that give one item to a group of lanes: the recursions of crf_general.hip, gl_windowed
// (crf_general_windowed.hip) and the lattice queries gl_span_logp, gl_run_walk, gl_edge_runs.  gfx950 only.
// Layout.  LP = L rounded up to a power of two (dispatch_lp); LP consecutive lanes ("a group", never straddling a wave) own one
// item -- a contig, a chunk, a chunk row, a window, a query --, lane j holds component j of its vector; `on = j < L`: the label
// exists, `jj = on ? j : 0`: its index for an address that is not used.  A step is a vector x (L x L) product: every lane writes
// its component to the group's LDS slot and reads all LP back as broadcast reads, against its column (forward) or row (backward)
// of the table, which it keeps in LP registers indexed by unrolled loops only.  LDS traffic of a wave is in order and a group
// lives inside a wave: a scheduling barrier on either side of the reads is all a step needs, and groups may run different trip
// counts.  The barriers are in the products below; a kernel writes its own only around an exchange that is none of these, and
// says why.  fma() is spelled out, in the operand order of the recursion: nothing here relies on contraction.  Kept in the
// kernels, because as functions they compiled to another instruction order (tools/isa_same.py): `on`, `jj`, the register loads
// of the table, the pair of sums of the queries and their backward direction E marg / alpha.
#pragma once
#include "crf_lanes.hpp"

#include <cfloat>

namespace gecco {
namespace {

// Host side: workgroups for `items` items at `per_block` to a workgroup
inline unsigned group_blocks(const long long items, const int per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }

// `const LaneGroup<LP> g{};` -- an aggregate, so that its members are formed in place, as if the kernel had written them out
template <int LP, int LANES = 256>
struct LaneGroup {
    static constexpr int G = LANES / LP;  // items per workgroup
    int j = threadIdx.x & (LP - 1);       // the lane's label
    int grp = threadIdx.x / LP;           // its group in the workgroup
    int slot = grp * LP;                  // where the group's slot begins in an LDS array of LANES doubles
    long long item = static_cast<long long>(blockIdx.x) * G + grp;  // the group's item: the caller tests it against its count
};

// ---- the products through the slot `vec`: x is the lane's component, m its registers ---------------------------------------
// sum_i vec[i] m[i], m the lane's column (a forward step); ROW: sum_i m[i] vec[i], m its row (a backward step)
template <bool ROW = false, int LP>
__device__ __forceinline__ double sum_product(double *vec, const int j, const double x, const double (&m)[LP]) {
    vec[j] = x;
    __builtin_amdgcn_wave_barrier();
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LP; ++i) acc = ROW ? fma(m[i], vec[i], acc) : fma(vec[i], m[i], acc);
    __builtin_amdgcn_wave_barrier();
    return acc;
}
// max_i (vec[i] + m[i]) over the L labels that exist; -infinity without one
template <int LP>
__device__ __forceinline__ double max_plus(double *vec, const int j, const double x, const double (&m)[LP], const int L) {
    vec[j] = x;
    __builtin_amdgcn_wave_barrier();
    double acc = -__builtin_huge_val();
#pragma unroll
    for (int i = 0; i < LP; ++i)
        if (i < L) acc = fmax(acc, vec[i] + m[i]);
    __builtin_amdgcn_wave_barrier();
    return acc;
}
// the same with its FIRST arg max ([EXT] CRFsuite crf1dc_viterbi: strict `<` update; -1 and -DBL_MAX without one) and, with
// SECOND, the runner-up, which is the maximum again when two labels attain it
struct MaxPlusArg {
    double best, second;
    int arg;
};
template <int LP, bool SECOND = false>
__device__ __forceinline__ MaxPlusArg max_plus_arg(double *vec, const int j, const double x, const double (&m)[LP], const int L) {
    vec[j] = x;
    __builtin_amdgcn_wave_barrier();
    int arg = -1;  // (declared in this order: the compiler's registers follow it)
    double best = -DBL_MAX, second = -DBL_MAX;
#pragma unroll
    for (int i = 0; i < LP; ++i) {
        if (i < L) {
            const double s = vec[i] + m[i];
            if (best < s) {
                second = best;
                best = s;
                arg = i;
            } else if (SECOND) {
                second = fmax(second, s);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    return MaxPlusArg{best, second, arg};
}

}  // namespace
}  // namespace gecco
