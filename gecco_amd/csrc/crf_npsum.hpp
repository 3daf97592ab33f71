// numpy's float64 summation order on the device: the one statement of it that every kernel reproducing a numpy.sum /
// numpy.mean of the reference uses (crf_composition.hip: Cluster.domain_composition; crf_segment.hip: the "antismash"
// criterion's mean).
//
// [EXT] numpy/_core/src/umath/loops_utils.h.src `pairwise_sum`: fewer than 8 terms are added left to right; up to 128
// terms go through 8 interleaved accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus a left-to-right
// tail; longer ranges split at n/2 rounded down to a multiple of 8, left + right.  The reduction starts from 0.0 and
// takes the array in chunks of 8192 elements (numpy's reduction buffer, numpy.getbufsize()), adding each chunk's
// pairwise sum in turn -- whatever SIMD width numpy was built for.
#pragma once
#include <hip/hip_runtime.h>

namespace gecco {

constexpr int kNpChunk = 8192;  // numpy.getbufsize()
constexpr int kNpLeaf = 128;    // pairwise_sum's PW_BLOCKSIZE
constexpr int kNpDepth = 8;     // splits on the path to a leaf of an 8192-term chunk: at most 7 (n = 7689 .. 7693)

// numpy's pairwise_sum for n <= 128 contiguous terms
__device__ __forceinline__ double np_leaf(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// pairwise_sum's recursion over [0, n), n <= kNpChunk, as a loop: descend left to a leaf, then climb while the pending
// node is complete.  leaf(off, len, index) supplies the value of the index-th leaf in left-to-right order (first index:
// `idx`, advanced past the last leaf).  Leaves come in order, so a right child starts where the last leaf ended: a
// pending split keeps only the length of its right child and, once that is under way, the sum of its left child.
template <class Leaf>
__device__ double np_pairwise_tree(int n, int &idx, Leaf leaf) {
    int r_len[kNpDepth];  // < 0: the right child is under way, lsum[] holds the left child's sum
    double lsum[kNpDepth];
    int top = 0, off = 0, len = n;
    for (;;) {
        while (len > kNpLeaf) {
            int n2 = len / 2;
            n2 -= n2 % 8;
            r_len[top++] = len - n2;
            len = n2;
        }
        double v = leaf(off, len, idx++);
        off += len;
        for (;;) {
            if (top == 0) return v;
            if (r_len[top - 1] > 0) {  // the left child is done: go right
                lsum[top - 1] = v;
                len = r_len[top - 1];
                r_len[top - 1] = -1;
                break;
            }
            v = lsum[top - 1] + v;  // both children done
            --top;
        }
    }
}

// numpy.sum of n contiguous doubles; leaf(off, len, index) as above, indices running over all chunks
template <class Leaf>
__device__ double np_sum_with(int n, Leaf leaf) {
    double res = 0.0;
    int idx = 0;
    for (int lo = 0; lo < n; lo += kNpChunk) {
        const int len = n - lo < kNpChunk ? n - lo : kNpChunk;
        res += np_pairwise_tree(len, idx, [&](int off, int l, int i) { return leaf(lo + off, l, i); });
    }
    return res;
}

// numpy.sum(a[0:n]) (0.0 for n = 0)
__device__ __forceinline__ double np_sum(const double *a, int n) {
    if (n <= kNpLeaf) return 0.0 + np_leaf(a, n);
    return np_sum_with(n, [&](int off, int len, int) { return np_leaf(a + off, len); });
}

}  // namespace gecco
