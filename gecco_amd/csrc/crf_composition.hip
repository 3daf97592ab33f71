// Weighted domain composition of called clusters on packed arrays:
// /root/reference/gecco/model.py:458-503 `Cluster.domain_composition(all_possible)` as assembled
// for the type classifier at /root/reference/gecco/types/__init__.py:118 -- one dense row per
// cluster over the classifier's domain list, entry i = numpy.sum of the weights (1 - pvalue) of
// the cluster's domains named all_possible[i], the row divided by `row.sum() or 1`.
//
// The only arithmetic is numpy.sum, so bit-identical output means reproducing numpy's pairwise
// summation order (crf_npsum.hpp).
//
// One workgroup per cluster.  Domain rows of a cluster are contiguous (genes of a cluster are
// consecutive, domain rows are stored per gene), so the cluster is a row range [r0, r1):
//   1. zero the output row;
//   2. every row finds its slot in a stable sort by column (rank by counting: clusters hold tens
//      of rows) and parks its weight there, so each column's terms are contiguous and in cluster
//      order; the first row of every column sums its terms;
//   3. the row total: leaves of the pairwise tree in parallel (one lane each), combined by lane 0.
#include "crf_device.hpp"
#include "crf_npsum.hpp"

namespace gecco {
namespace {

constexpr int kCT = 256;
constexpr int kMaxLeaves = 2048;  // leaves of the row-total tree held in LDS (n_cols <= ~130 k)

__global__ void __launch_bounds__(kCT) composition_kernel(const int32_t *__restrict__ seg, const int32_t *__restrict__ dom_ptr,
                                                          const int32_t *__restrict__ dom_col,
                                                          const double *__restrict__ dom_w, double *__restrict__ tmp,
                                                          int n_cols, int normalize, double *__restrict__ out) {
    __shared__ double leafv[kMaxLeaves];
    __shared__ double total_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    double *row = out + static_cast<size_t>(b) * n_cols;
    const int r0 = dom_ptr[seg[4 * b + 2]], r1 = dom_ptr[seg[4 * b + 3]];
    for (int i = tid; i < n_cols; i += kCT) row[i] = 0.0;
    // stable counting rank of every row among the rows of this cluster (absent columns last)
    for (int r = r0 + tid; r < r1; r += kCT) {
        const int c = dom_col[r];
        const unsigned key = c < 0 ? 0xffffffffu : unsigned(c);
        int before = 0;
        for (int q = r0; q < r1; ++q) {
            const int cq = dom_col[q];
            const unsigned kq = cq < 0 ? 0xffffffffu : unsigned(cq);
            before += (kq < key || (kq == key && q < r)) ? 1 : 0;
        }
        tmp[r0 + before] = dom_w[r];
    }
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += kCT) {
        const int c = dom_col[r];
        if (c < 0 || c >= n_cols) continue;
        int smaller = 0, same = 0;
        bool first = true;
        for (int q = r0; q < r1; ++q) {
            const int cq = dom_col[q];
            smaller += (cq >= 0 && cq < c) ? 1 : 0;
            same += cq == c ? 1 : 0;
            first = first && !(cq == c && q < r);
        }
        if (first) row[c] = np_sum(tmp + r0 + smaller, same);
    }
    if (!normalize) return;
    __syncthreads();
    // composition.sum(): leaves in parallel, then the tree by one lane
    if (n_cols <= 128 * 8 || n_cols > kMaxLeaves * 64) {
        if (tid == 0) total_s = np_sum(row, n_cols);
    } else {
        np_sum_with(n_cols, [&](int off, int len, int idx) {
            if (idx % kCT == tid) leafv[idx] = np_leaf(row + off, len);
            return 0.0;
        });
        __syncthreads();
        if (tid == 0) total_s = np_sum_with(n_cols, [&](int, int, int idx) { return leafv[idx]; });
    }
    __syncthreads();
    const double total = total_s;
    const double den = total == 0.0 ? 1.0 : total;  // `composition.sum() or 1`
    for (int i = tid; i < n_cols; i += kCT) row[i] = row[i] / den;
}

}  // namespace

hipError_t launch_composition(const int32_t *d_seg, int n_seg, const int32_t *d_dom_ptr, const int32_t *d_dom_col,
                              const double *d_dom_w, double *d_tmp, int n_cols, int normalize, double *d_out,
                              hipStream_t stream) {
    if (n_seg <= 0 || n_cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(composition_kernel, dim3(n_seg), dim3(kCT), 0, stream, d_seg, d_dom_ptr, d_dom_col, d_dom_w, d_tmp,
                       n_cols, normalize, d_out);
    return hipGetLastError();
}

}  // namespace gecco
