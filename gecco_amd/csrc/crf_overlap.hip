// Interval join of genes and clusters (gecco_crf_cluster_overlaps) and the member-list form of the domain composition
// (gecco_crf_domain_composition_members); DESIGN.md 4.11.
//
// What is joined: GECCO's `label_genes` and `gecco train`'s `_assign_clusters` (gecco/cli/commands/_common.py,
// gecco/cli/commands/train.py) both ask, for every gene, which clusters of its sequence it overlaps, bounds inclusive:
// cluster_start <= gene.end and gene.start <= cluster_end.  The first wants a flag per gene, the second the genes of every
// cluster in gene order (a gene in several clusters is in each).
//
// Labels: one thread per gene.  The clusters of a sequence are sorted by start; the running maximum of their ends is
// non-decreasing, so a binary search finds the first cluster that can reach the gene's start (every cluster before it ends
// earlier, even where a long cluster covers later short ones), and the walk stops at the first cluster that starts after
// the gene's end.
//
// Members: count -> scan -> fill, one thread per cluster for the count and the fill, without atomics, so the order is the
// genes' order by construction.  The genes of a sequence are contiguous and sorted by start (checked on the device first);
// a gene that overlaps a cluster starts no earlier than cluster_start - (longest gene), so a binary search bounds the walk
// from below and the first gene starting after cluster_end ends it.  The scans are the three-pass reduce / scan-of-sums /
// rescan form over tiles of 1024, in int64.
//
// Compositions by member list: the domain rows of every member, in member order, are gathered into one contiguous array
// (degree -> scan -> gather), and the composition kernel of crf_composition.hip runs on it unchanged with one segment per
// cluster: the sums see the rows in the order `Cluster.domain_composition` sees them, so the bits are those of the
// contiguous form.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "../../include/gecco_crf.h"
#include "crf_device.hpp"
#include "crf_model.hpp"
#include "crf_overlap.hpp"
#include "crf_plan.hpp"

namespace gecco {

namespace {

constexpr int kOT = 256;                 // threads per workgroup of every kernel here
constexpr int kScanItems = 4;            // items per thread of a scan tile
constexpr int kScanTile = kOT * kScanItems;
constexpr int64_t kCoordLimit = int64_t(1) << 60;  // |coordinate| bound: cluster_start - longest gene cannot overflow

// ---------------------------------------------------------------- workgroup helpers
// exclusive prefix of v over the workgroup (fixed Hillis-Steele order); `total` = the sum over the workgroup
__device__ int64_t wg_exclusive(int64_t v, int64_t *lds, int64_t &total) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int off = 1; off < kOT; off <<= 1) {
        const int64_t t = tid >= off ? lds[tid - off] : 0;
        __syncthreads();
        lds[tid] += t;
        __syncthreads();
    }
    const int64_t incl = lds[tid];
    total = lds[kOT - 1];
    __syncthreads();
    return incl - v;
}

// ---------------------------------------------------------------- exclusive scan, int32 in, int64 out [n + 1]
__global__ void __launch_bounds__(kOT) scan_tile_sums(const int32_t *__restrict__ in, int64_t n, int64_t *__restrict__ bsum) {
    __shared__ int64_t lds[kOT];
    const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanItems;
    int64_t s = 0;
    for (int i = 0; i < kScanItems; ++i)
        if (base + i < n) s += in[base + i];
    int64_t total;
    wg_exclusive(s, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum[b] becomes the exclusive prefix of the tile sums, bsum[nb] the grand total
__global__ void __launch_bounds__(kOT) scan_block_sums(int64_t *__restrict__ bsum, int nb) {
    __shared__ int64_t lds[kOT];
    int64_t carry = 0;
    for (int base = 0; base < nb; base += kOT) {
        const int i = base + int(threadIdx.x);
        const int64_t v = i < nb ? bsum[i] : 0;
        int64_t total;
        const int64_t ex = wg_exclusive(v, lds, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ void __launch_bounds__(kOT) scan_tiles(const int32_t *__restrict__ in, int64_t n, const int64_t *__restrict__ bsum,
                                                  int nb, int64_t *__restrict__ out) {
    __shared__ int64_t lds[kOT];
    const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanItems;
    int64_t v[kScanItems], s = 0;
    for (int i = 0; i < kScanItems; ++i) {
        v[i] = base + i < n ? in[base + i] : 0;
        s += v[i];
    }
    int64_t total;
    int64_t run = bsum[blockIdx.x] + wg_exclusive(s, lds, total);
    for (int i = 0; i < kScanItems; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

// ---------------------------------------------------------------- the join
// per workgroup: any gene out of order (sequence code outside [0, n_seqs), codes decreasing, starts decreasing inside a
// sequence) or with a coordinate beyond 2^60, and the longest gene (end - start, at least 0)
__global__ void __launch_bounds__(kOT) check_genes(int32_t n, const int32_t *__restrict__ seq, const int64_t *__restrict__ start,
                                                   const int64_t *__restrict__ end, int32_t n_seqs, int64_t *__restrict__ blk) {
    __shared__ int64_t bad_s[kOT], len_s[kOT];
    const int tid = threadIdx.x;
    const int64_t g = int64_t(blockIdx.x) * kOT + tid;
    int64_t bad = 0, len = 0;
    if (g < n) {
        const int32_t s = seq[g];
        bad = (s < 0 || s >= n_seqs) ? 1 : 0;
        if (g > 0) {
            const int32_t sp = seq[g - 1];
            bad |= (sp > s || (sp == s && start[g - 1] > start[g])) ? 1 : 0;
        }
        bad |= (start[g] <= -kCoordLimit || start[g] >= kCoordLimit || end[g] <= -kCoordLimit || end[g] >= kCoordLimit) ? 1 : 0;
        const int64_t l = end[g] - start[g];
        len = l > 0 ? l : 0;
    }
    bad_s[tid] = bad;
    len_s[tid] = len;
    __syncthreads();
    for (int off = kOT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            bad_s[tid] |= bad_s[tid + off];
            len_s[tid] = len_s[tid] > len_s[tid + off] ? len_s[tid] : len_s[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        blk[2 * blockIdx.x] = bad_s[0];
        blk[2 * blockIdx.x + 1] = len_s[0];
    }
}

// one workgroup: out[0] = any gene out of order, out[1] = the longest gene
__global__ void __launch_bounds__(kOT) reduce_check(const int64_t *__restrict__ blk, int nb, int64_t *__restrict__ out) {
    __shared__ int64_t bad_s[kOT], len_s[kOT];
    const int tid = threadIdx.x;
    int64_t bad = 0, len = 0;
    for (int b = tid; b < nb; b += kOT) {
        bad |= blk[2 * b];
        len = len > blk[2 * b + 1] ? len : blk[2 * b + 1];
    }
    bad_s[tid] = bad;
    len_s[tid] = len;
    __syncthreads();
    for (int off = kOT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            bad_s[tid] |= bad_s[tid + off];
            len_s[tid] = len_s[tid] > len_s[tid + off] ? len_s[tid] : len_s[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = bad_s[0];
        out[1] = len_s[0];
    }
}

// running maximum of the cluster ends inside every sequence (one thread per sequence: a sequence holds a few clusters)
__global__ void __launch_bounds__(kOT) cluster_runmax(int32_t n_seqs, const int32_t *__restrict__ cptr,
                                                      const int64_t *__restrict__ cend, int64_t *__restrict__ cmax) {
    const int64_t s = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (s >= n_seqs) return;
    int64_t m = INT64_MIN;
    for (int32_t j = cptr[s]; j < cptr[s + 1]; ++j) {
        m = cend[j] > m ? cend[j] : m;
        cmax[j] = m;
    }
}

__global__ void __launch_bounds__(kOT) label_genes(int32_t n, const int32_t *__restrict__ seq, const int64_t *__restrict__ start,
                                                   const int64_t *__restrict__ end, const int32_t *__restrict__ cptr,
                                                   const int64_t *__restrict__ cstart, const int64_t *__restrict__ cend,
                                                   const int64_t *__restrict__ cmax, uint8_t *__restrict__ label) {
    const int64_t g = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (g >= n) return;
    const int32_t s = seq[g];
    const int64_t gs = start[g], ge = end[g];
    int32_t lo = cptr[s];
    int32_t hi = cptr[s + 1];
    const int32_t c1 = hi;
    while (lo < hi) {  // first cluster whose running end maximum reaches the gene's start
        const int32_t mid = lo + (hi - lo) / 2;
        if (cmax[mid] < gs)
            lo = mid + 1;
        else
            hi = mid;
    }
    uint8_t hit = 0;
    for (int32_t j = lo; j < c1 && cstart[j] <= ge; ++j)
        if (cend[j] >= gs) {
            hit = 1;
            break;
        }
    label[g] = hit;
}

// sptr[s] = first gene of sequence s (s = 0 .. n_seqs): a lower bound over the non-decreasing codes
__global__ void __launch_bounds__(kOT) seq_gene_ptr(int32_t n, const int32_t *__restrict__ seq, int32_t n_seqs,
                                                    int32_t *__restrict__ sptr) {
    const int64_t s = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (s > n_seqs) return;
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (seq[mid] < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    sptr[s] = lo;
}

// the genes of cluster k, in gene order: emit(g) for each (the count and the fill walk identically)
template <class Emit>
__device__ void cluster_members(int32_t k, int32_t n_seqs, const int32_t *__restrict__ cptr, const int64_t *__restrict__ cstart,
                                const int64_t *__restrict__ cend, const int32_t *__restrict__ sptr,
                                const int64_t *__restrict__ start, const int64_t *__restrict__ end, int64_t maxlen, Emit emit) {
    int32_t lo = 0, hi = n_seqs + 1;  // the sequence of k: the last s with cptr[s] <= k
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (cptr[mid] <= k)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int32_t s = lo - 1;
    const int64_t cs = cstart[k], ce = cend[k], first = cs - maxlen;
    int32_t a = sptr[s];
    hi = sptr[s + 1];
    const int32_t g1 = hi;
    while (a < hi) {  // first gene that starts late enough to reach the cluster's start
        const int32_t mid = a + (hi - a) / 2;
        if (start[mid] < first)
            a = mid + 1;
        else
            hi = mid;
    }
    for (int32_t g = a; g < g1 && start[g] <= ce; ++g)
        if (end[g] >= cs) emit(g);
}

__global__ void __launch_bounds__(kOT) count_members(int32_t m, int32_t n_seqs, const int32_t *__restrict__ cptr,
                                                     const int64_t *__restrict__ cstart, const int64_t *__restrict__ cend,
                                                     const int32_t *__restrict__ sptr, const int64_t *__restrict__ start,
                                                     const int64_t *__restrict__ end, const int64_t *__restrict__ check,
                                                     int32_t *__restrict__ cnt) {
    const int64_t k = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (k >= m) return;
    int32_t c = 0;
    cluster_members(int32_t(k), n_seqs, cptr, cstart, cend, sptr, start, end, check[1], [&](int32_t) { ++c; });
    cnt[k] = c;
}

__global__ void __launch_bounds__(kOT) fill_members(int32_t m, int32_t n_seqs, const int32_t *__restrict__ cptr,
                                                    const int64_t *__restrict__ cstart, const int64_t *__restrict__ cend,
                                                    const int32_t *__restrict__ sptr, const int64_t *__restrict__ start,
                                                    const int64_t *__restrict__ end, const int64_t *__restrict__ check,
                                                    const int64_t *__restrict__ mptr, int32_t *__restrict__ members) {
    const int64_t k = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (k >= m) return;
    int32_t *out = members + mptr[k];
    int64_t i = 0;
    cluster_members(int32_t(k), n_seqs, cptr, cstart, cend, sptr, start, end, check[1], [&](int32_t g) { out[i++] = g; });
}

// ---------------------------------------------------------------- compositions by member list
__global__ void __launch_bounds__(kOT) member_degrees(int64_t n_members, const int32_t *__restrict__ members,
                                                      const int32_t *__restrict__ dom_ptr, int32_t *__restrict__ deg) {
    const int64_t j = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (j >= n_members) return;
    const int32_t g = members[j];
    deg[j] = dom_ptr[g + 1] - dom_ptr[g];
}

__global__ void __launch_bounds__(kOT) gather_rows(int64_t n_members, const int32_t *__restrict__ members,
                                                   const int32_t *__restrict__ dom_ptr, const int32_t *__restrict__ dom_col,
                                                   const double *__restrict__ dom_w, const int64_t *__restrict__ vptr,
                                                   int32_t *__restrict__ vptr32, int32_t *__restrict__ gcol,
                                                   double *__restrict__ gw) {
    const int64_t j = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (j >= n_members) return;
    const int32_t g = members[j], r0 = dom_ptr[g], r1 = dom_ptr[g + 1];
    const int64_t base = vptr[j];
    for (int32_t r = r0; r < r1; ++r) {
        gcol[base + (r - r0)] = dom_col[r];
        gw[base + (r - r0)] = dom_w[r];
    }
    vptr32[j] = int32_t(base);
    if (j == n_members - 1) vptr32[n_members] = int32_t(vptr[n_members]);
}

// segment rows of the composition kernel (crf_composition.hip reads columns 2 and 3): cluster k = member slots
// [mptr[k], mptr[k + 1])
__global__ void __launch_bounds__(kOT) member_segments(int32_t m, const int32_t *__restrict__ mptr, int32_t *__restrict__ seg) {
    const int64_t k = int64_t(blockIdx.x) * kOT + threadIdx.x;
    if (k >= m) return;
    seg[4 * k] = 0;
    seg[4 * k + 1] = int32_t(k) + 1;
    seg[4 * k + 2] = mptr[k];
    seg[4 * k + 3] = mptr[k + 1];
}

// ---------------------------------------------------------------- host side
int fail(const std::string &msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

inline unsigned grid(int64_t n) { return unsigned((n + kOT - 1) / kOT); }

struct JoinBuffers {  // device buffers and the stream of one call, released on every way out
    Stream stream;  // (before the blocks: destroyed after them)
    std::vector<DeviceBlock<char>> bufs;
    ~JoinBuffers() {
        if (stream.get()) (void)hipStreamSynchronize(stream.get());
    }
    template <class T>
    int alloc(T **p, int64_t n, const char *what) {
        bufs.emplace_back();
        int rc = bufs.back().alloc(size_t(n > 0 ? n : 1) * sizeof(T), what);
        *p = bufs.back().at<T>(0);
        return rc;
    }
    template <class T>
    int upload(T **p, const T *src, int64_t n, const char *what) {
        int rc = alloc(p, n, what);
        if (rc || n <= 0) return rc;
        return check_hip(hipMemcpyAsync(*p, src, size_t(n) * sizeof(T), hipMemcpyHostToDevice, stream.get()), what);
    }
};

// exclusive scan of in[0, n) into out[0, n] (out[n] = total) on the arena's stream
int exclusive_scan(JoinBuffers &A, const int32_t *d_in, int64_t n, int64_t *d_out) {
    if (n == 0) return check_hip(hipMemsetAsync(d_out, 0, sizeof(int64_t), A.stream.get()), "scan");
    const int64_t nb = (n + kScanTile - 1) / kScanTile;
    if (nb > INT32_MAX - 1) return fail("scan: too many items");
    int64_t *d_bsum = nullptr;
    int rc = A.alloc(&d_bsum, nb + 1, "scan alloc");
    if (rc) return rc;
    scan_tile_sums<<<unsigned(nb), kOT, 0, A.stream.get()>>>(d_in, n, d_bsum);
    scan_block_sums<<<1, kOT, 0, A.stream.get()>>>(d_bsum, int(nb));
    scan_tiles<<<unsigned(nb), kOT, 0, A.stream.get()>>>(d_in, n, d_bsum, int(nb), d_out);
    return check_hip(hipGetLastError(), "scan kernels");
}

int download_sync(JoinBuffers &A, void *dst, const void *src, size_t bytes, const char *what) {
    int rc = check_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, A.stream.get()), what);
    if (rc) return rc;
    return check_hip(hipStreamSynchronize(A.stream.get()), what);
}

}  // namespace

int overlaps_check(int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start, const int64_t *gene_end,
                   int32_t n_seqs, const int32_t *cluster_ptr, const int64_t *cluster_start, const int64_t *cluster_end,
                   const uint8_t *label_out, const int32_t *member_ptr_out, int64_t max_members, const int64_t *n_members) {
    if (n_genes < 0 || n_seqs < 0 || max_members < 0 || !n_members) return fail("cluster_overlaps: bad arguments");
    if (!cluster_ptr || !member_ptr_out) return fail("cluster_overlaps: null cluster_ptr or member_ptr_out");
    if (n_genes > 0 && (!gene_seq || !gene_start || !gene_end || !label_out))
        return fail("cluster_overlaps: null gene arrays");
    if (cluster_ptr[0] != 0) return fail("cluster_overlaps: cluster_ptr must start at 0");
    for (int32_t s = 0; s < n_seqs; ++s)
        if (cluster_ptr[s + 1] < cluster_ptr[s]) return fail("cluster_overlaps: cluster_ptr must be non-decreasing");
    const int32_t m = cluster_ptr[n_seqs];
    if (m > 0 && (!cluster_start || !cluster_end)) return fail("cluster_overlaps: null cluster arrays");
    for (int32_t s = 0; s < n_seqs; ++s)
        for (int32_t j = cluster_ptr[s]; j < cluster_ptr[s + 1]; ++j) {
            if (cluster_start[j] <= -kCoordLimit || cluster_start[j] >= kCoordLimit || cluster_end[j] <= -kCoordLimit ||
                cluster_end[j] >= kCoordLimit)
                return fail("cluster_overlaps: cluster " + std::to_string(j) + " has a coordinate beyond 2^60");
            if (j > cluster_ptr[s] && cluster_start[j] < cluster_start[j - 1])
                return fail("cluster_overlaps: the clusters of sequence " + std::to_string(s) + " are not sorted by start");
        }
    return GECCO_CRF_OK;
}

int cluster_overlaps(int32_t device, int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start,
                     const int64_t *gene_end, int32_t n_seqs, const int32_t *cluster_ptr, const int64_t *cluster_start,
                     const int64_t *cluster_end, uint8_t *label_out, int32_t *member_ptr_out, int32_t *member_gene_out,
                     int64_t max_members, int64_t *n_members) {
    const int32_t m = cluster_ptr[n_seqs];
    *n_members = 0;
    if (m == 0 && n_genes == 0) {
        member_ptr_out[0] = 0;
        return GECCO_CRF_OK;
    }
    int rc = set_device(device);
    if (rc) return rc;
    JoinBuffers A;
    if ((rc = A.stream.create())) return rc;
    int32_t *d_seq = nullptr, *d_cptr = nullptr, *d_sptr = nullptr, *d_cnt = nullptr, *d_members = nullptr;
    int64_t *d_start = nullptr, *d_end = nullptr, *d_cs = nullptr, *d_ce = nullptr, *d_cmax = nullptr, *d_blk = nullptr,
            *d_check = nullptr, *d_mptr = nullptr;
    uint8_t *d_label = nullptr;
    const int64_t n = n_genes, nbg = (n + kOT - 1) / kOT;
    if ((rc = A.upload(&d_seq, gene_seq, n, "H2D gene_seq")) || (rc = A.upload(&d_start, gene_start, n, "H2D gene_start")) ||
        (rc = A.upload(&d_end, gene_end, n, "H2D gene_end")) ||
        (rc = A.upload(&d_cptr, cluster_ptr, int64_t(n_seqs) + 1, "H2D cluster_ptr")) ||
        (rc = A.upload(&d_cs, cluster_start, m, "H2D cluster_start")) || (rc = A.upload(&d_ce, cluster_end, m, "H2D cluster_end")) ||
        (rc = A.alloc(&d_cmax, m, "alloc cluster running max")) || (rc = A.alloc(&d_blk, 2 * nbg, "alloc check")) ||
        (rc = A.alloc(&d_check, 2, "alloc check")) || (rc = A.alloc(&d_sptr, int64_t(n_seqs) + 1, "alloc sequence ranges")) ||
        (rc = A.alloc(&d_cnt, m, "alloc member counts")) || (rc = A.alloc(&d_mptr, int64_t(m) + 1, "alloc member_ptr")) ||
        (rc = A.alloc(&d_label, n, "alloc labels")))
        return rc;
    // 1. the genes' order, and the longest gene
    int64_t check[2] = {0, 0};
    if (n > 0) {
        check_genes<<<unsigned(nbg), kOT, 0, A.stream.get()>>>(n_genes, d_seq, d_start, d_end, n_seqs, d_blk);
        reduce_check<<<1, kOT, 0, A.stream.get()>>>(d_blk, int(nbg), d_check);
        if ((rc = check_hip(hipGetLastError(), "check kernels"))) return rc;
        if ((rc = download_sync(A, check, d_check, sizeof(check), "D2H check"))) return rc;
        if (check[0])
            return fail("cluster_overlaps: genes must be grouped by sequence code (0 <= code < n_seqs, non-decreasing), "
                        "sorted by start inside a sequence, with coordinates below 2^60");
    } else if ((rc = check_hip(hipMemsetAsync(d_check, 0, sizeof(check), A.stream.get()), "memset check"))) {
        return rc;
    }
    // 2. labels: one thread per gene over the clusters' running maximum of ends
    if (n_seqs > 0) cluster_runmax<<<grid(n_seqs), kOT, 0, A.stream.get()>>>(n_seqs, d_cptr, d_ce, d_cmax);
    if (n > 0)
        label_genes<<<grid(n), kOT, 0, A.stream.get()>>>(n_genes, d_seq, d_start, d_end, d_cptr, d_cs, d_ce, d_cmax, d_label);
    // 3. members: count -> scan -> fill, one thread per cluster
    seq_gene_ptr<<<grid(int64_t(n_seqs) + 1), kOT, 0, A.stream.get()>>>(n_genes, d_seq, n_seqs, d_sptr);
    if (m > 0)
        count_members<<<grid(m), kOT, 0, A.stream.get()>>>(m, n_seqs, d_cptr, d_cs, d_ce, d_sptr, d_start, d_end, d_check, d_cnt);
    if ((rc = check_hip(hipGetLastError(), "join kernels"))) return rc;
    if ((rc = exclusive_scan(A, d_cnt, m, d_mptr))) return rc;
    int64_t total = 0;
    if ((rc = download_sync(A, &total, d_mptr + m, sizeof(total), "D2H member count"))) return rc;
    if (total > INT32_MAX) return fail("cluster_overlaps: more than 2^31 - 1 cluster members");
    *n_members = total;
    if (n > 0 && (rc = check_hip(hipMemcpyAsync(label_out, d_label, size_t(n), hipMemcpyDeviceToHost, A.stream.get()), "D2H labels")))
        return rc;
    std::vector<int64_t> mptr(size_t(m) + 1);
    rc = download_sync(A, mptr.data(), d_mptr, (size_t(m) + 1) * sizeof(int64_t), "D2H member_ptr");
    for (int32_t k = 0; !rc && k <= m; ++k) member_ptr_out[k] = int32_t(mptr[k]);
    if (rc) return rc;
    if (total > max_members) return fail("cluster_overlaps: member_gene_out too small (n_members holds the size needed)");
    if (total == 0) return GECCO_CRF_OK;
    if (!member_gene_out) return fail("cluster_overlaps: null member_gene_out");
    if ((rc = A.alloc(&d_members, total, "alloc members"))) return rc;
    fill_members<<<grid(m), kOT, 0, A.stream.get()>>>(m, n_seqs, d_cptr, d_cs, d_ce, d_sptr, d_start, d_end, d_check, d_mptr,
                                                d_members);
    if ((rc = check_hip(hipGetLastError(), "fill kernel"))) return rc;
    return download_sync(A, member_gene_out, d_members, size_t(total) * sizeof(int32_t), "D2H members");
}

int composition_members_check(const int32_t *member_ptr, int32_t n_clusters, const int32_t *member_gene,
                              const int32_t *dom_ptr, int32_t n_genes, const int32_t *dom_col, const double *dom_weight,
                              int32_t n_cols, const double *comp_out) {
    if (n_clusters < 0 || n_genes < 0 || n_cols < 0) return fail("domain_composition_members: bad arguments");
    if (n_clusters == 0 || n_cols == 0) return GECCO_CRF_OK;
    if (!member_ptr || !dom_ptr || !comp_out) return fail("domain_composition_members: null arrays");
    if (member_ptr[0] != 0) return fail("domain_composition_members: member_ptr must start at 0");
    for (int32_t k = 0; k < n_clusters; ++k)
        if (member_ptr[k + 1] < member_ptr[k]) return fail("domain_composition_members: member_ptr must be non-decreasing");
    const int32_t n_members = member_ptr[n_clusters];
    if (n_members > 0 && !member_gene) return fail("domain_composition_members: null member_gene");
    for (int32_t j = 0; j < n_members; ++j)
        if (member_gene[j] < 0 || member_gene[j] >= n_genes)
            return fail("domain_composition_members: member " + std::to_string(j) + " outside the gene range");
    if (dom_ptr[0] != 0) return fail("domain_composition_members: dom_ptr must start at 0");
    for (int32_t g = 0; g < n_genes; ++g)
        if (dom_ptr[g + 1] < dom_ptr[g]) return fail("domain_composition_members: dom_ptr must be non-decreasing");
    if (dom_ptr[n_genes] > 0 && (!dom_col || !dom_weight)) return fail("domain_composition_members: null domain arrays");
    return GECCO_CRF_OK;
}

int composition_members(int32_t device, const int32_t *member_ptr, int32_t n_clusters, const int32_t *member_gene,
                        const int32_t *dom_ptr, int32_t n_genes, const int32_t *dom_col, const double *dom_weight,
                        int32_t n_cols, int32_t normalize, double *comp_out) {
    int rc = set_device(device);
    if (rc) return rc;
    JoinBuffers A;
    if ((rc = A.stream.create())) return rc;
    const int64_t M = member_ptr[n_clusters], rows = dom_ptr[n_genes], m = n_clusters;
    int32_t *d_mptr = nullptr, *d_members = nullptr, *d_dptr = nullptr, *d_dcol = nullptr, *d_deg = nullptr, *d_vptr32 = nullptr,
            *d_gcol = nullptr, *d_seg = nullptr;
    double *d_dw = nullptr, *d_out = nullptr;
    int64_t *d_vptr = nullptr;
    if ((rc = A.upload(&d_mptr, member_ptr, m + 1, "H2D member_ptr")) || (rc = A.upload(&d_members, member_gene, M, "H2D members")) ||
        (rc = A.upload(&d_dptr, dom_ptr, int64_t(n_genes) + 1, "H2D dom_ptr")) ||
        (rc = A.upload(&d_dcol, dom_col, rows, "H2D dom_col")) || (rc = A.upload(&d_dw, dom_weight, rows, "H2D dom_weight")) ||
        (rc = A.alloc(&d_deg, M, "alloc degrees")) || (rc = A.alloc(&d_vptr, M + 1, "alloc row offsets")) ||
        (rc = A.alloc(&d_vptr32, M + 1, "alloc row offsets")) || (rc = A.alloc(&d_seg, 4 * m, "alloc segments")) ||
        (rc = A.alloc(&d_out, m * int64_t(n_cols), "alloc compositions")))
        return rc;
    if (M > 0) member_degrees<<<grid(M), kOT, 0, A.stream.get()>>>(M, d_members, d_dptr, d_deg);
    if ((rc = check_hip(hipGetLastError(), "degree kernel"))) return rc;
    if ((rc = exclusive_scan(A, d_deg, M, d_vptr))) return rc;
    int64_t total = 0;
    if ((rc = download_sync(A, &total, d_vptr + M, sizeof(total), "D2H row count"))) return rc;
    if (total > INT32_MAX) return fail("domain_composition_members: more than 2^31 - 1 domain rows over the members");
    double *d_tmp = nullptr, *d_gw = nullptr;
    if ((rc = A.alloc(&d_gcol, total, "alloc gathered columns")) || (rc = A.alloc(&d_gw, total, "alloc gathered weights")) ||
        (rc = A.alloc(&d_tmp, total, "alloc composition scratch")))
        return rc;
    if (M > 0)
        gather_rows<<<grid(M), kOT, 0, A.stream.get()>>>(M, d_members, d_dptr, d_dcol, d_dw, d_vptr, d_vptr32, d_gcol, d_gw);
    else if ((rc = check_hip(hipMemsetAsync(d_vptr32, 0, sizeof(int32_t), A.stream.get()), "memset row offsets")))
        return rc;
    member_segments<<<grid(m), kOT, 0, A.stream.get()>>>(n_clusters, d_mptr, d_seg);
    if ((rc = check_hip(hipGetLastError(), "gather kernels"))) return rc;
    if ((rc = check_hip(launch_composition(d_seg, n_clusters, d_vptr32, d_gcol, d_gw, d_tmp, n_cols, normalize ? 1 : 0, d_out,
                                           A.stream.get()),
                        "composition launch")))
        return rc;
    return download_sync(A, comp_out, d_out, size_t(m) * size_t(n_cols) * sizeof(double), "D2H compositions");
}

}  // namespace gecco
