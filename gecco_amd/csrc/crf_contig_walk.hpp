// The frame of the whole-contig lattice walks that keep a column of values per label: crf_kbest.hip (the K best prefixes),
// crf_minrun.hip (a run-length counter, forward and backward) and crf_counts.hip (a run counter).  Each of those files holds
// its recursion, its tie rule and its layout; what they share is here, once.  gfx950 only.
//
// Geometry.  A group of LP = next-pow2(L) lanes per contig, one lane per label (the destination label of a forward walk, the
// source label of a backward one), 64 / LP contigs per wave, and a workgroup is one wave.  Lanes of labels that do not exist carry
// state -infinity and the transition 0.0; contigs beyond the batch have no genes.  The lane's column (or row) of trans is in
// LP registers, indexed by unrolled loops only.
// Columns.  A lane's values of one gene lie in LDS, two generations, [2][64 rows][slots | 1] doubles: the row length is odd, so
// that lanes reading different rows at one slot hit different banks.
// The walk.  A contig is one sequential walk (it is not chunked; profiles/EXPERIMENTS.md has the parallel-in-T idea).  The state
// score of a step is loaded eight steps ahead, as in gl_viterbi_wave.  The groups of a wave end at different steps; a group that
// has ended keeps its values and stores nothing, and the wave goes on while any group does.  A step ends in its one barrier,
// which stands outside every divergent branch: every lane of the wave takes every step.
// The semirings.  A destination's sources come as a functor `sources(f)` that calls f(label, value, second) for every source
// in ascending (label, slot) order, the second-slot source of a label directly behind its first, and -infinity for what is no
// source.  The sum semiring is a max-shifted log-sum-exp in two passes, in which -infinity stays -infinity; the max semiring a
// strict `>` update, so the earlier source wins a tie, which packs a back-pointer byte: the source label in the low five bits
// and kWalkSecond for a second-slot source.  Values are (previous + trans) + state, every addition rounded on its own: the
// files that include this header are compiled without floating-point contraction.
// The end of a contig.  An arg max across the group's lanes by xor-shuffles, the smaller label winning a tie, and a log-sum-exp
// over the group by crf_lanes.hpp's butterflies: one order of operations in every lane.  No atomics anywhere.
#pragma once
#include "crf_device.hpp"
#include "crf_lane_group.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kWalkLanes = 64;           // lanes per workgroup: one wave
constexpr int kWalkAhead = 8;            // steps of state scores fetched ahead
constexpr int kWalkBack = 256;           // lanes per workgroup of a backtrack
constexpr uint8_t kWalkSecond = 0x20;    // back-pointer bit: the source was the second slot of its label
constexpr double kWalkNinf = -INFINITY;

template <int LP>
struct WalkGroup {
    static constexpr int G = kWalkLanes / LP;  // contigs per wave
    int lane, j, row0;  // the lane, its label, the first lane of its group
    long long c;        // the contig
    bool valid, on;     // the contig exists; the label exists
    int g0, T, jj;      // first gene and number of genes (0 without a contig); the label, or 0 for an address that is not used

    __device__ __forceinline__ WalkGroup(const int32_t *__restrict__ contig_ptr, const int n_contigs, const int L)
        : lane(threadIdx.x), j(lane & (LP - 1)), row0(lane - j), c(static_cast<long long>(blockIdx.x) * G + lane / LP),
          valid(c < n_contigs), on(j < L), g0(0), T(0), jj(on ? j : 0) {
        if (valid) {
            g0 = contig_ptr[c];
            T = contig_ptr[c + 1] - g0;
            T = T < 0 ? 0 : T;
        }
    }
    // the lane's column of trans (every source label into j), or with ROW its row (j into every successor label)
    template <bool ROW = false>
    __device__ __forceinline__ void load_trans(const double *__restrict__ trans, const int L, double (&t)[LP]) const {
#pragma unroll
        for (int i = 0; i < LP; ++i) t[i] = i < L ? trans[ROW ? jj * L + i : i * L + jj] : 0.0;
    }
    // the lane's state scores: column() is gene 0 of the contig, state_at(column, ., in, t) gene t; 0.0 where the walk has left the
    // contig (`in` false: nothing is loaded)
    __device__ __forceinline__ const double *column(const double *__restrict__ state, const int L) const {
        return state + static_cast<size_t>(g0) * L + jj;
    }
    __device__ __forceinline__ double state_at(const double *__restrict__ st, const int L, const bool in, const int t) const {
        return in ? (on ? st[static_cast<size_t>(t) * L] : kWalkNinf) : 0.0;
    }
};

// the two generations of columns in LDS; gen(t) is the one of parity t
struct WalkColumns {
    int KS;
    double *buf0, *buf1;
    __device__ __forceinline__ WalkColumns(double *lds, const int slots) : KS(slots | 1), buf0(lds), buf1(lds + kWalkLanes * KS) {}
    __device__ __forceinline__ double *gen(const int t) const { return (t & 1) ? buf1 : buf0; }
    // generation 0: `value` at slot `first` of the lane's row (no slot if first < 0), -infinity elsewhere and in generation 1
    __device__ __forceinline__ void fill(const int lane, const int first, const double value) const {
        for (int k = 0; k < KS; ++k) {
            buf0[lane * KS + k] = k == first ? value : kWalkNinf;
            buf1[lane * KS + k] = kWalkNinf;
        }
    }
};

// The steps first .. end - 1 of every group of the wave (`end` may differ between groups, and a group may have no step):
// step(s, v) gets v = value_of_step(s), which was asked for eight steps earlier.  `step` ends in the step's barrier.  A forward
// walk numbers its steps by their genes, 1 .. T - 1; a backward walk counts them from the last gene.
template <class Value, class Step>
__device__ __forceinline__ void contig_walk(const int first, const int end, Value &&value_of_step, Step &&step) {
    double nxt[kWalkAhead];
#pragma unroll
    for (int k = 0; k < kWalkAhead; ++k) nxt[k] = value_of_step(first + k);
    for (int sb = first; __any(sb < end); sb += kWalkAhead) {
        double cur[kWalkAhead];
#pragma unroll
        for (int k = 0; k < kWalkAhead; ++k) cur[k] = nxt[k];
#pragma unroll
        for (int k = 0; k < kWalkAhead; ++k) nxt[k] = value_of_step(sb + kWalkAhead + k);
#pragma unroll
        for (int k = 0; k < kWalkAhead; ++k) {
            if (!__any(sb + k < end)) break;  // (wave-uniform)
            step(sb + k, cur[k]);
        }
    }
}

// the log-sum-exp of a destination's sources: `finite` is false, and `value` -infinity, when every source is -infinity
struct WalkSum {
    double value;
    bool finite;
};
template <class Sources>
__device__ __forceinline__ WalkSum walk_sum(Sources &&sources) {
    double mx = kWalkNinf;
    sources([&](int, double v, bool) { mx = v > mx ? v : mx; });
    const double shift = mx > kWalkNinf ? mx : 0.0;
    double sum = 0.0;
    sources([&](int, double v, bool) { sum += v > kWalkNinf ? exp(v - shift) : 0.0; });
    return WalkSum{mx > kWalkNinf ? mx + log(sum) : kWalkNinf, mx > kWalkNinf};
}
// their maximum and its back-pointer byte (0 when every source is -infinity)
template <class Sources>
__device__ __forceinline__ double walk_max(Sources &&sources, int &arg) {
    double best = kWalkNinf;
    arg = 0;
    sources([&](int i, double v, bool second) {
        const bool take = v > best;  // strict: the earlier source wins a tie
        best = take ? v : best;
        arg = take ? (i | (second ? kWalkSecond : 0)) : arg;
    });
    return best;
}
// a forward destination's value in either semiring: the reduction of its sources, then the state score
template <bool SUM, class Sources>
__device__ __forceinline__ double walk_value(Sources &&sources, const double s_t, int &arg) {
    if constexpr (SUM) {
        arg = 0;
        const WalkSum r = walk_sum(sources);
        return r.finite ? r.value + s_t : kWalkNinf;
    } else {
        return walk_max(sources, arg) + s_t;
    }
}

template <class T>
__device__ __forceinline__ T walk_pick(const bool take, const T other, const T mine) {
    return take ? other : mine;
}
// every lane of a group gets the group's maximum of v and in `label` the lane's label that holds it, the smaller label among equal
// values; `payload` travels with the label
template <int LP, class... Payload>
__device__ __forceinline__ void group_argmax(double &v, int &label, Payload &...payload) {
#pragma unroll
    for (int off = LP / 2; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int ol = __shfl_xor(label, off);
        const bool take = ov > v || (ov == v && ol < label);
        ((payload = walk_pick(take, __shfl_xor(payload, off), payload)), ...);  // (every lane shuffles: no shuffle under `take`)
        v = take ? ov : v;
        label = take ? ol : label;
    }
}
// every lane of a group gets the log-sum-exp of the group's v; -infinity when every v is
template <int LP>
__device__ __forceinline__ double group_lse(const double v) {
    const double mx = group_max<LP>(v);
    const double shift = mx > kWalkNinf ? mx : 0.0;
    const double sum = group_sum<LP>(v > kWalkNinf ? exp(v - shift) : 0.0);
    return mx > kWalkNinf ? mx + log(sum) : kWalkNinf;
}

// Host side: a launch of one wave per 64 / LP contigs, and the LDS bytes of its columns
template <int LP>
unsigned walk_blocks(const int32_t n_contigs) {
    return group_blocks(n_contigs, kWalkLanes / LP);
}
inline size_t walk_lds_bytes(const int32_t slots) { return size_t(2) * kWalkLanes * size_t(slots | 1) * sizeof(double); }
// what a launcher of a counter lattice takes: a label count and a counter limit inside the kernels' range, and a label set that
// is not empty and holds no label at or above L
inline bool walk_counter_ok(const GenArgs &a, const uint32_t set_mask, const int32_t limit, const int32_t max_limit) {
    const uint32_t beyond = a.L >= 32 ? 0u : ~0u << a.L;
    return a.L > 0 && a.L <= kGenMaxL && limit >= 1 && limit <= max_limit && set_mask != 0 && !(set_mask & beyond);
}

}  // namespace
}  // namespace gecco
