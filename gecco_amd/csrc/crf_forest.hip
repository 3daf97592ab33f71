// Random-forest fit and predict of GECCO's cluster type classifier (gecco_crf_forest_*).
//
// Semantics: sklearn 1.7's RandomForestClassifier as GECCO's TypeClassifier configures it (criterion "gini",
// max_features "sqrt", bootstrap, no depth limit, min_samples_split 2, min_samples_leaf 1, no class weights, sparse CSC
// float32 input), tree for tree and bit for bit: the depth-first builder of sklearn/tree/_tree.pyx (right child pushed
// first, so node ids are pre-order with the left subtree first), node_split_best of _splitter.pyx with the sparse
// partitioner of _partitioner.pyx, and the Gini criterion of _criterion.pyx.  The host draws the random streams (per-tree
// seeds, bootstrap counts, the splitter's initial rand_r state); the device runs sklearn's our_rand_r / rand_int.
//
// One workgroup builds one tree.  Three things are sequential in sklearn and stay so here, on lane 0: the feature draw loop
// with its n_known / n_found / n_drawn constants bookkeeping on the tree-wide `features` / `constant_features`
// permutation, the pop order of the builder's stack, and the comparison of each evaluated feature's best split with the
// best so far (strict >: the first drawn feature wins a tie).  The work inside a node is spread over the workgroup:
//   * a pre-pass marks the features that have a nonzero value in the node (one sweep over the node's CSR rows); a drawn
//     feature without one is all zeros there, hence constant, and the draw loop moves on without any cooperative work;
//   * a drawn feature's node nonzeros are gathered from its CSC column through `index_to_samples` and sorted (bitonic);
//     the node's zeros form one block between the negatives and the positives, as in the sparse partitioner;
//   * per output, one workgroup scan gives the class weights left of every position, and each position accumulates its
//     Gini terms in sklearn's output order; the proxy improvement of every valid position follows, and an argmax that keeps
//     the first position in scan order among equal values.
// Which position is "valid" is the sklearn 1.7.2 build's: Xf[p] > Xf[p - 1] between sorted float32 neighbours (the zero
// block compares as zeros), and a feature is constant in a node when Xf[end - 1] <= Xf[start].  sklearn's source adds a
// FEATURE_THRESHOLD of 1e-7 to the right-hand sides, but in the released build that constant acts as 0: two values one
// ulp apart, or the zero block and the smallest denormal, are split (tests/test_gpu_forest_edges.py pins
// it).  The order of samples within a node, which sklearn's in-place partitioning leaves implementation-defined among
// equal values, changes no stored number: every quantity of a node is a function of its sample set.
//
// Why the parallel sums give sklearn's bits: bootstrap weights are small integers (counts of a sample in the draw), so every
// weighted class count, node weight and left / right weight is an integer below 2^24, exact in fp64 whatever the order of
// summation.  They are summed here as int32 and converted.  Nothing else is summed in parallel: each Gini term, impurity,
// proxy, threshold and node value is formed from those integers with sklearn's own operations in sklearn's order (this file
// is compiled with -ffp-contract=off: no fused multiply-add where the source has none).
//
// Range (checked on the host): n_samples <= 4096, n_features <= 8192, n_outputs <= 64, 1 or 2 classes per output.  Node
// and stack storage is sized per tree (2 n - 1 nodes, n + 1 stack records) and every write is bounds-checked on the device;
// a tree that would overflow stops and reports a status instead.
//
// Several forests in one launch (gecco_crf_forest_fit_batch): the grid is n_problems x n_trees workgroups, and
// workgroup b builds tree b % n_trees of problem b / n_trees.  What the builder knows of its problem is one FitArgs record,
// read from a table in device memory instead of the kernel arguments; every pointer in it addresses that problem's own
// arrays, so a tree reads and writes nothing of another problem and its bits are those of the problem fitted alone.  The lone
// fit is a batch of one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_forest.hpp"
#include "crf_model.hpp"
#include "crf_plan.hpp"

#pragma clang fp contract(off)

namespace gecco {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = kForestMaxSamples / kThreads;  // positions per thread in the scans
constexpr uint16_t kNone = 0xFFFF;
constexpr double kEpsilon = 2.220446049250313e-16;  // np.finfo(np.double).eps (_tree.pyx EPSILON)
constexpr uint32_t kRandRMax = 2147483647u;       // sklearn/utils/_random.pxd RAND_R_MAX

enum ForestStatus : int32_t { kOk = 0, kNodeOverflow = 1, kStackOverflow = 2, kPartitionMismatch = 3, kGatherOverflow = 4 };

__device__ __forceinline__ uint32_t our_rand_r(uint32_t &seed) {
    if (seed == 0) seed = 1;  // DEFAULT_SEED
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed % (kRandRMax + 1u);
}

struct FitArgs {
    int32_t n, F, n_out, mc, max_features, cap, stack_cap;
    uint64_t two_class;  // bit k: output k has 2 classes
    const int32_t *col_ptr, *row_idx;
    const float *val;
    const int32_t *row_ptr, *col_idx;  // CSR of the nonzero-valued entries (the node feature pre-pass)
    const uint64_t *ybits;             // bit k of sample i: its class index for output k
    const int32_t *counts;             // [T][n] bootstrap counts
    const uint32_t *rand_state;        // [T]
    int32_t *stack;                    // [T][stack_cap][6]
    int32_t *left, *right, *feature, *n_node;
    double *threshold, *impurity, *weighted, *value;
    int32_t *node_count, *max_depth, *status;  // [T]
    uint8_t *ncls;                              // [n_out], for predict
};

struct Shared {
    uint16_t samples[kForestMaxSamples];   // sklearn's `samples`, the node ranges of the tree
    uint16_t pos[kForestMaxSamples];       // index_to_samples (kNone: not drawn into this tree)
    uint16_t w[kForestMaxSamples];         // bootstrap count by sample id
    uint16_t feat[kForestMaxFeatures];     // `features`
    uint16_t cfeat[kForestMaxFeatures];    // `constant_features`
    uint32_t nzmask[kForestMaxFeatures / 32];
    float key[kForestMaxSamples];          // a feature's gathered node nonzeros ...
    uint16_t id[kForestMaxSamples];        // ... and their samples
    uint16_t tmp[kForestMaxSamples];       // partition scratch
    uint8_t side[kForestMaxSamples];       // 1: goes left
    int32_t wave_i[kWaves];
    double wave_d[kWaves];
    int32_t wave_j[kWaves];
    int32_t nodeY[kForestMaxOutputs], leftY[kForestMaxOutputs];  // class-1 weight per output: the node, its left child
    int32_t nodeW, leftW;
    int32_t m, nneg, cmd, fconst, fbest_j, fleft, stack_top, node_start, node_end, n_known, n_total, err;
    double fbest_proxy, fthr;
};

// Exclusive scan of one int per thread over the workgroup (integers: exact in any order).  `total` is the sum.
__device__ int block_excl_scan(int v, Shared &s, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s.wave_i[wave] = x;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < kWaves; ++k) {
        off += k < wave ? s.wave_i[k] : 0;
        tot += s.wave_i[k];
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

// Argmax over the workgroup: the largest proxy, the smallest position among equal ones.  Result on every thread.
__device__ void block_argmax(double &p, int &j, Shared &s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d > 0; d >>= 1) {
        const double q = __shfl_xor(p, d, 64);
        const int k = __shfl_xor(j, d, 64);
        if (q > p || (q == p && k < j)) {
            p = q;
            j = k;
        }
    }
    if (lane == 0) {
        s.wave_d[wave] = p;
        s.wave_j[wave] = j;
    }
    __syncthreads();
    p = s.wave_d[0];
    j = s.wave_j[0];
    for (int k = 1; k < kWaves; ++k) {
        const double q = s.wave_d[k];
        const int jj = s.wave_j[k];
        if (q > p || (q == p && jj < j)) {
            p = q;
            j = jj;
        }
    }
    __syncthreads();
}

// Weight and per-output class-1 weight of samples[a, b) into *Wout / Y[0, n_out).
__device__ void node_sums(const FitArgs &A, Shared &s, int a, int b, int32_t *Wout, int32_t *Y) {
    int tot;
    int wsum = 0;
    for (int p = a + int(threadIdx.x); p < b; p += kThreads) wsum += s.w[s.samples[p]];
    (void)block_excl_scan(wsum, s, tot);
    if (threadIdx.x == 0) *Wout = tot;
    for (int k = 0; k < A.n_out; ++k) {
        int ysum = 0;
        for (int p = a + int(threadIdx.x); p < b; p += kThreads) {
            const int smp = s.samples[p];
            ysum += int((A.ybits[smp] >> k) & 1u) * s.w[smp];
        }
        (void)block_excl_scan(ysum, s, tot);
        if (threadIdx.x == 0) Y[k] = tot;
    }
    __syncthreads();
}

// Gini impurity of a sample set with weight W and class-1 weights Y[k] (_criterion.pyx Gini.node_impurity).
__device__ double gini(const FitArgs &A, int W, const int32_t *Y) {
    const double wd = double(W);
    double g = 0.0;
    for (int k = 0; k < A.n_out; ++k) {
        double sq = 0.0;
        const double c0 = double(W - Y[k]);
        sq += c0 * c0;
        if ((A.two_class >> k) & 1u) {
            const double c1 = double(Y[k]);
            sq += c1 * c1;
        }
        g += 1.0 - sq / (wd * wd);
    }
    return g / A.n_out;
}

// Value of compact entry j of the node's sorted feature values: nonzeros s.key[0, m) with the zero block (if any) as
// one entry after the s.nneg negatives.
__device__ __forceinline__ float entry_value(const Shared &s, int j, bool zeros) {
    if (!zeros) return s.key[j];
    return j < s.nneg ? s.key[j] : (j == s.nneg ? 0.0f : s.key[j - 1]);
}

// Evaluate feature f on samples[a, b): constant? else the best valid position.  Results in s.fconst / s.fbest_*.
__device__ void evaluate_feature(const FitArgs &A, Shared &s, int f, int a, int b, int W) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        s.m = 0;
        s.nneg = 0;
    }
    __syncthreads();
    // gather (extract_nnz): the column's entries whose sample is in the node, zeros left out
    for (int e = A.col_ptr[f] + tid; e < A.col_ptr[f + 1]; e += kThreads) {
        const int r = A.row_idx[e];
        const float v = A.val[e];
        const int p = s.pos[r];
        if (p != kNone && p >= a && p < b && v != 0.0f) {
            const int k = atomicAdd(&s.m, 1);
            if (k < kForestMaxSamples) {
                s.key[k] = v;
                s.id[k] = uint16_t(r);
            } else {
                s.err = kGatherOverflow;
            }
        }
    }
    __syncthreads();
    const int m = s.m < kForestMaxSamples ? s.m : kForestMaxSamples;
    int P = 1;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += kThreads) {
        s.key[i] = INFINITY;
        s.id[i] = kNone;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {  // bitonic sort of (key, id) by key
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P; i += kThreads) {
                const int ixj = i ^ jj;
                if (ixj > i) {
                    const float x = s.key[i], y = s.key[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (x > y) : (x < y)) {
                        s.key[i] = y;
                        s.key[ixj] = x;
                        const uint16_t t = s.id[i];
                        s.id[i] = s.id[ixj];
                        s.id[ixj] = t;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < m; i += kThreads)
        if (s.key[i] < 0.0f && (i + 1 == m || !(s.key[i + 1] < 0.0f))) s.nneg = i + 1;
    __syncthreads();
    const int n_node = b - a;
    const bool zeros = m < n_node;
    const int N = m + (zeros ? 1 : 0);
    // constant: Xf[end - 1] <= Xf[start] (FEATURE_THRESHOLD acts as 0 in the build this follows)
    if (entry_value(s, N - 1, zeros) <= entry_value(s, 0, zeros)) {
        if (tid == 0) s.fconst = 1;
        __syncthreads();
        return;
    }
    // each thread owns compact entries [c0, c0 + cnt): its positions ("left = entries before j")
    const int C = (N + kThreads - 1) / kThreads;
    const int c0 = tid * C;
    const int cnt = c0 < N ? (N - c0 < C ? N - c0 : C) : 0;
    const int zpos = zeros ? s.nneg : -1;
    int ew[kChunk];
    uint64_t ey[kChunk];
    int wl[kChunk];
    double gl[kChunk], gr[kChunk];
    int local = 0;
#pragma unroll
    for (int c = 0; c < kChunk; ++c) {
        ew[c] = 0;
        ey[c] = 0;
        gl[c] = 0.0;
        gr[c] = 0.0;
        if (c < cnt) {
            const int j = c0 + c;
            if (j != zpos) {
                const int e = zeros && j > zpos ? j - 1 : j;
                const int smp = s.id[e];
                ew[c] = s.w[smp];
                ey[c] = A.ybits[smp];
            }
            local += ew[c];
        }
    }
    int tot_nz;
    int run = block_excl_scan(local, s, tot_nz);
    const int Wz = W - tot_nz;  // weight of the zero block
#pragma unroll
    for (int c = 0; c < kChunk; ++c) {
        const int j = c0 + c;
        wl[c] = run + (zpos >= 0 && j > zpos ? Wz : 0);
        run += ew[c];
    }
    const int Wtot = W;
    for (int k = 0; k < A.n_out; ++k) {
        const int Yk = s.nodeY[k];
        const bool two = (A.two_class >> k) & 1u;
        int yloc = 0;
#pragma unroll
        for (int c = 0; c < kChunk; ++c) yloc += int((ey[c] >> k) & 1u) * ew[c];
        int ytot;
        int yrun = block_excl_scan(yloc, s, ytot);
        const int Yz = Yk - ytot;
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const int j = c0 + c;
            if (c < cnt && j > 0) {
                const int yl = yrun + (zpos >= 0 && j > zpos ? Yz : 0);
                const int wlc = wl[c], wrc = Wtot - wlc;
                // children_impurity: sum_left[k, c], sum_right = sum_total - sum_left, classes in order
                double sql = 0.0, sqr = 0.0;
                const double l0 = double(wlc - yl), r0 = double((Wtot - Yk) - (wlc - yl));
                sql += l0 * l0;
                sqr += r0 * r0;
                if (two) {
                    const double l1 = double(yl), r1 = double(Yk - yl);
                    sql += l1 * l1;
                    sqr += r1 * r1;
                }
                const double wld = double(wlc), wrd = double(wrc);
                gl[c] += 1.0 - sql / (wld * wld);
                gr[c] += 1.0 - sqr / (wrd * wrd);
            }
            yrun += int((ey[c] >> k) & 1u) * ew[c];
        }
    }
    double bp = -INFINITY;
    int bj = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < kChunk; ++c) {
        const int j = c0 + c;
        if (c < cnt && j > 0) {
            if (entry_value(s, j, zeros) > entry_value(s, j - 1, zeros)) {  // next_p stops here
                const double il = gl[c] / A.n_out, ir = gr[c] / A.n_out;
                const double wld = double(wl[c]), wrd = double(Wtot - wl[c]);
                const double proxy = -wrd * ir - wld * il;
                if (proxy > bp) {
                    bp = proxy;
                    bj = j;
                }
            }
        }
    }
    block_argmax(bp, bj, s);
    if (tid == 0) {
        s.fconst = 0;
        s.fbest_proxy = bp;
        s.fbest_j = bj;
        if (bj != 0x7fffffff) {
            const float pv = entry_value(s, bj - 1, zeros), cv = entry_value(s, bj, zeros);
            double thr = double(pv) / 2.0 + double(cv) / 2.0;
            if (thr == double(cv) || thr == INFINITY || thr == -INFINITY) thr = double(pv);
            s.fthr = thr;
            s.fleft = zeros && bj > zpos ? bj - 1 + (n_node - m) : bj;  // samples left of the position
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void forest_fit_kernel(const FitArgs *__restrict__ problems, int32_t n_trees) {
    __shared__ Shared s;
    const int problem = int(blockIdx.x) / n_trees;
    const int t = int(blockIdx.x) - problem * n_trees, tid = threadIdx.x;
    const FitArgs &A = problems[problem];  // uniform over the workgroup: scalar loads, like kernel arguments
    const int n = A.n, F = A.F;
    const int32_t *cnt = A.counts + size_t(t) * n;
    for (int i = tid; i < n; i += kThreads) s.w[i] = uint16_t(cnt[i]);
    for (int f = tid; f < F; f += kThreads) s.feat[f] = uint16_t(f);
    int32_t *stack = A.stack + size_t(t) * A.stack_cap * 6;
    const size_t nb = size_t(t) * A.cap;  // this tree's node slots
    const size_t vstride = size_t(A.n_out) * A.mc;
    if (tid == 0) s.err = kOk;
    __syncthreads();
    // lane 0's sequential state: the splitter's rand_r state, the builder's counters
    uint32_t rs = A.rand_state[t];
    int n_nodes = 0, depth_seen = -1, wtotal = 0;
    if (tid == 0) {  // Splitter.init: the samples of positive weight, in index order
        int j = 0;
        for (int i = 0; i < n; ++i) {
            if (s.w[i] > 0) {
                s.samples[j] = uint16_t(i);
                s.pos[i] = uint16_t(j);
                wtotal += s.w[i];
                ++j;
            } else {
                s.pos[i] = kNone;
            }
        }
        const int32_t root[6] = {0, j, 0, -1, 0, 0};  // start, end, depth, parent, is_left, n_constant_features
        for (int k = 0; k < 6; ++k) stack[k] = root[k];
        s.stack_top = 1;
    }
    __syncthreads();
    while (true) {
        int depth = 0, parent = -1, is_left = 0;
        if (tid == 0) {
            if (s.stack_top > 0 && s.err == kOk) {
                const int32_t *r = stack + size_t(s.stack_top - 1) * 6;
                s.node_start = r[0];
                s.node_end = r[1];
                depth = r[2];
                parent = r[3];
                is_left = r[4];
                s.n_known = r[5];
                s.stack_top -= 1;
            } else {
                s.node_start = -1;
            }
        }
        __syncthreads();
        if (s.node_start < 0) break;
        const int start = s.node_start, end = s.node_end;
        const int n_node = end - start;
        node_sums(A, s, start, end, &s.nodeW, s.nodeY);
        const int W = s.nodeW;
        double imp = 0.0;
        if (tid == 0) {
            imp = gini(A, W, s.nodeY);  // = the parent's children_impurity for this child: the same sums, the same operations
            s.cmd = (n_node < 2 || imp <= kEpsilon) ? 1 : 0;
        }
        __syncthreads();
        const bool leaf0 = s.cmd != 0;
        __syncthreads();
        // ---- node_split_best
        int n_total = 0;
        if (!leaf0) {
            for (int i = tid; i < (F + 31) / 32; i += kThreads) s.nzmask[i] = 0u;
            __syncthreads();
            for (int p = start + tid; p < end; p += kThreads) {
                const int smp = s.samples[p];
                for (int e = A.row_ptr[smp]; e < A.row_ptr[smp + 1]; ++e) {
                    const int c = A.col_idx[e];
                    atomicOr(&s.nzmask[c >> 5], 1u << (c & 31));
                }
            }
            __syncthreads();
            const int n_known = s.n_known;
            int f_i = F, n_found = 0, n_drawn = 0, n_visited = 0, f_j = 0, best_found = 0, best_feature = -1, best_left = 0;
            double best_proxy = -INFINITY, best_thr = 0.0;
            n_total = n_known;
            while (true) {
                if (tid == 0) {
                    int cmd = -1;
                    while (f_i > n_total && (n_visited < A.max_features || n_visited <= n_found + n_drawn)) {
                        ++n_visited;
                        // rand_int(n_drawn_constants, f_i - n_found_constants)
                        f_j = n_drawn + int(our_rand_r(rs) % uint32_t(f_i - n_found - n_drawn));
                        if (f_j < n_known) {
                            const uint16_t x = s.feat[n_drawn];
                            s.feat[n_drawn] = s.feat[f_j];
                            s.feat[f_j] = x;
                            ++n_drawn;
                            continue;
                        }
                        f_j += n_found;
                        const int f = s.feat[f_j];
                        if (!((s.nzmask[f >> 5] >> (f & 31)) & 1u)) {  // all zeros in the node: constant
                            s.feat[f_j] = s.feat[n_total];
                            s.feat[n_total] = uint16_t(f);
                            ++n_found;
                            ++n_total;
                            continue;
                        }
                        cmd = f;
                        break;
                    }
                    s.cmd = cmd;
                }
                __syncthreads();
                const int f = s.cmd;
                if (f < 0) break;
                evaluate_feature(A, s, f, start, end, W);
                if (tid == 0) {
                    if (s.fconst) {
                        s.feat[f_j] = s.feat[n_total];
                        s.feat[n_total] = uint16_t(f);
                        ++n_found;
                        ++n_total;
                    } else {
                        --f_i;
                        const uint16_t x = s.feat[f_i];
                        s.feat[f_i] = s.feat[f_j];
                        s.feat[f_j] = x;
                        if (s.fbest_j != 0x7fffffff && s.fbest_proxy > best_proxy) {
                            best_proxy = s.fbest_proxy;
                            best_found = 1;
                            best_feature = f;
                            best_thr = s.fthr;
                            best_left = s.fleft;
                        }
                    }
                }
                __syncthreads();
            }
            if (tid == 0) {
                s.n_total = n_total;
                s.cmd = best_found ? best_feature : -1;
                s.fthr = best_thr;
                s.fleft = best_left;
            }
            __syncthreads();
            // features[:n_known] = constant_features[:n_known]; constant_features[n_known:n_total] = features[n_known:n_total]
            const int nt = s.n_total;
            for (int i = tid; i < nt; i += kThreads) {
                if (i < n_known) s.feat[i] = s.cfeat[i];
                else s.cfeat[i] = s.feat[i];
            }
            __syncthreads();
        }
        const int split_feature = leaf0 ? -1 : s.cmd;
        const double split_thr = s.fthr;
        const int left_n = s.fleft;
        __syncthreads();
        // ---- partition_samples_final: samples with X[:, f] <= threshold first
        if (split_feature >= 0) {
            const int f = split_feature;
            // (a threshold of exactly 0 is the midpoint of -a and +a: the node then holds no zeros, and the block is empty)
            const uint8_t zero_left = 0.0 <= split_thr ? 1 : 0;
            for (int p = start + tid; p < end; p += kThreads) s.side[p] = zero_left;
            __syncthreads();
            for (int e = A.col_ptr[f] + tid; e < A.col_ptr[f + 1]; e += kThreads) {
                const int p = s.pos[A.row_idx[e]];
                const float v = A.val[e];
                if (p != kNone && p >= start && p < end && v != 0.0f) s.side[p] = double(v) <= split_thr ? 1 : 0;
            }
            __syncthreads();
            const int C = (n_node + kThreads - 1) / kThreads;
            const int c0 = start + tid * C < end ? start + tid * C : end;
            const int c1 = c0 + C < end ? c0 + C : end;
            int nl = 0;
            for (int p = c0; p < c1; ++p) nl += s.side[p];
            int L;
            int offl = block_excl_scan(nl, s, L);
            int offr = (c0 - start) - offl;
            for (int p = c0; p < c1; ++p) {
                if (s.side[p]) s.tmp[start + offl++] = s.samples[p];
                else s.tmp[start + L + offr++] = s.samples[p];
            }
            __syncthreads();
            for (int p = start + tid; p < end; p += kThreads) {
                const uint16_t smp = s.tmp[p];
                s.samples[p] = smp;
                s.pos[smp] = uint16_t(p);
            }
            if (tid == 0 && L != left_n) s.err = kPartitionMismatch;
            __syncthreads();
            node_sums(A, s, start, start + left_n, &s.leftW, s.leftY);
        }
        if (tid == 0 && s.err == kOk) {
            bool leaf = split_feature < 0;
            if (!leaf) {  // impurity_improvement of the chosen split; a split that makes things worse by more than EPSILON is a leaf
                const int Wl = s.leftW, Wr = W - Wl;
                int32_t Yr[kForestMaxOutputs];
                for (int k = 0; k < A.n_out; ++k) Yr[k] = s.nodeY[k] - s.leftY[k];
                const double imp_l = gini(A, Wl, s.leftY), imp_r = gini(A, Wr, Yr);
                const double wd = double(W);
                const double improvement =
                    (wd / double(wtotal)) * (imp - (double(Wr) / wd * imp_r) - (double(Wl) / wd * imp_l));
                leaf = improvement + kEpsilon < 0.0;
            }
            const int id = n_nodes;
            if (id >= A.cap) {
                s.err = kNodeOverflow;
            } else {
                if (parent >= 0) (is_left ? A.left : A.right)[nb + parent] = id;
                A.left[nb + id] = -1;
                A.right[nb + id] = -1;
                A.feature[nb + id] = leaf ? -2 : split_feature;
                A.threshold[nb + id] = leaf ? -2.0 : split_thr;
                A.impurity[nb + id] = imp;
                A.n_node[nb + id] = n_node;
                A.weighted[nb + id] = double(W);
                double *v = A.value + (nb + id) * vstride;
                for (int k = 0; k < A.n_out; ++k) {  // node_value: sum_total[k, c] / weighted_n_node_samples
                    if ((A.two_class >> k) & 1u) {
                        v[k * A.mc] = double(W - s.nodeY[k]) / double(W);
                        v[k * A.mc + 1] = double(s.nodeY[k]) / double(W);
                    } else {
                        v[k * A.mc] = double(W) / double(W);
                        if (A.mc == 2) v[k * A.mc + 1] = 0.0;
                    }
                }
                n_nodes += 1;
                if (depth > depth_seen) depth_seen = depth;
                if (!leaf) {
                    if (s.stack_top + 2 > A.stack_cap) {
                        s.err = kStackOverflow;
                    } else {
                        int32_t *r = stack + size_t(s.stack_top) * 6;
                        const int32_t right[6] = {start + left_n, end, depth + 1, id, 0, n_total};
                        const int32_t lft[6] = {start, start + left_n, depth + 1, id, 1, n_total};
                        for (int k = 0; k < 6; ++k) {
                            r[k] = right[k];
                            r[6 + k] = lft[k];
                        }
                        s.stack_top += 2;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        A.node_count[t] = n_nodes;
        A.max_depth[t] = depth_seen;
        A.status[t] = s.err;
    }
    if (t == 0 && tid < A.n_out) A.ncls[tid] = (A.two_class >> tid) & 1u ? 2 : 1;
}

// One problem of a predict launch: a forest, its rows, and the first of its blocks in the grid.
struct PredictArgs {
    const int32_t *left, *right, *feature;
    const double *threshold, *value;
    const uint8_t *ncls;
    int32_t n_trees, cap, n_out, mc, F, block0;
    const double *x;
    int64_t n_rows;
    double *posit;
};

// One thread per (row, output): walk every tree in order, sum the normalised leaf values in fp64 (forest
// _accumulate_prediction), divide by the number of trees, posit = 1 - proba[:, k, 0].  Block b serves problem
// block_problem[b]; a thread's arithmetic depends on its own forest and row alone.
__global__ __launch_bounds__(256) void forest_predict_kernel(const PredictArgs *__restrict__ problems,
                                                             const int32_t *__restrict__ block_problem) {
    const PredictArgs P = problems[block_problem[blockIdx.x]];
    const int64_t g = int64_t(int(blockIdx.x) - P.block0) * blockDim.x + threadIdx.x;
    if (g >= P.n_rows * P.n_out) return;
    const int64_t row = g / P.n_out;
    const int k = int(g % P.n_out);
    const double *xr = P.x + row * P.F;
    double acc = 0.0;
    for (int t = 0; t < P.n_trees; ++t) {
        const size_t nb = size_t(t) * P.cap;
        int node = 0;
        while (P.left[nb + node] >= 0) {
            const float xv = float(xr[P.feature[nb + node]]);  // predict input is validated to float32 first
            node = double(xv) <= P.threshold[nb + node] ? P.left[nb + node] : P.right[nb + node];
        }
        const double *v = P.value + (nb + node) * size_t(P.n_out) * P.mc + size_t(k) * P.mc;
        double norm = P.ncls[k] == 2 ? v[0] + v[1] : v[0];
        if (norm == 0.0) norm = 1.0;
        acc += v[0] / norm;
    }
    P.posit[g] = 1.0 - acc / double(P.n_trees);
}

int fail(const std::string &msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

// Byte offsets of arrays laid end to end in one allocation, each aligned to 256 bytes.
struct Layout {
    size_t bytes = 0;
    template <typename T>
    size_t add(size_t n) {
        const size_t at = bytes;
        bytes += (n * sizeof(T) + 255) / 256 * 256;
        return at;
    }
};

template <typename T>
void stage(std::vector<unsigned char> &host, size_t off, const T *src, size_t n) {
    if (n) std::memcpy(host.data() + off, src, n * sizeof(T));
}

int check_shared(const std::string &pre, int32_t n_features, int32_t n_outputs, int32_t n_trees, int32_t max_features) {
    if (n_features < 1 || n_features > kForestMaxFeatures)
        return fail(pre + "n_features must be in [1, " + std::to_string(kForestMaxFeatures) + "]");
    if (n_outputs < 1 || n_outputs > kForestMaxOutputs)
        return fail(pre + "n_outputs must be in [1, " + std::to_string(kForestMaxOutputs) + "]");
    if (n_trees < 1 || n_trees > 65535) return fail(pre + "n_trees must be in [1, 65535]");
    if (max_features < 1 || max_features > n_features) return fail(pre + "max_features must be in [1, n_features]");
    return GECCO_CRF_OK;
}

int check_samples(const std::string &pre, int32_t n_samples) {
    if (n_samples < 1 || n_samples > kForestMaxSamples)
        return fail(pre + "n_samples must be in [1, " + std::to_string(kForestMaxSamples) + "]");
    return GECCO_CRF_OK;
}

int check_data(const std::string &pre, int32_t n_features, int32_t n_outputs, int32_t n_trees, const ForestProblem &p) {
    const int32_t n_samples = p.n_samples;
    const int32_t *col_ptr = p.col_ptr, *row_idx = p.row_idx, *sample_counts = p.sample_counts;
    if (!col_ptr || !p.n_classes || !p.y || !sample_counts || !p.rand_state) return fail(pre + "null buffer");
    if (col_ptr[0] != 0) return fail(pre + "col_ptr[0] must be 0");
    for (int32_t f = 0; f < n_features; ++f)
        if (col_ptr[f + 1] < col_ptr[f]) return fail(pre + "col_ptr must be non-decreasing");
    const int64_t nnz = col_ptr[n_features];
    if (nnz > 0 && (!row_idx || !p.values)) return fail(pre + "null buffer");
    for (int32_t f = 0; f < n_features; ++f)
        for (int32_t e = col_ptr[f]; e < col_ptr[f + 1]; ++e) {
            if (row_idx[e] < 0 || row_idx[e] >= n_samples) return fail(pre + "row index out of range");
            if (e > col_ptr[f] && row_idx[e] <= row_idx[e - 1])
                return fail(pre + "row indices must be strictly increasing within a column");
            if (!std::isfinite(p.values[e])) return fail(pre + "values must be finite");
        }
    for (int32_t k = 0; k < n_outputs; ++k)
        if (p.n_classes[k] < 1 || p.n_classes[k] > 2) return fail(pre + "every output must have 1 or 2 classes");
    for (int64_t i = 0; i < int64_t(n_samples) * n_outputs; ++i)
        if (p.y[i] >= p.n_classes[i % n_outputs]) return fail(pre + "class index out of range");
    for (int64_t i = 0; i < int64_t(n_trees) * n_samples; ++i)
        if (sample_counts[i] < 0 || sample_counts[i] > n_samples) return fail(pre + "bootstrap counts must be in [0, n_samples]");
    for (int32_t t = 0; t < n_trees; ++t) {
        int64_t tot = 0;
        for (int32_t i = 0; i < n_samples; ++i) tot += sample_counts[int64_t(t) * n_samples + i];
        if (tot < 1) return fail(pre + "a tree without samples");
        if (tot >= (int64_t(1) << 24)) return fail(pre + "total weight of a tree must stay below 2^24");
    }
    return GECCO_CRF_OK;
}

std::string fit_prefix(bool lone, int32_t k) {
    return lone ? std::string("forest_fit: ") : "forest_fit_batch: problem " + std::to_string(k) + ": ";
}

}  // namespace

int forest_fit_check(int32_t n_samples, int32_t n_features, const int32_t *col_ptr, const int32_t *row_idx, const float *values,
                     int32_t n_outputs, const uint8_t *n_classes, const uint8_t *y, int32_t n_trees, const int32_t *sample_counts,
                     const uint32_t *rand_state, int32_t max_features) {
    const std::string pre = fit_prefix(true, 0);
    const ForestProblem p{n_samples, col_ptr, row_idx, values, n_classes, y, sample_counts, rand_state};
    int rc;
    if ((rc = check_samples(pre, n_samples)) || (rc = check_shared(pre, n_features, n_outputs, n_trees, max_features))) return rc;
    return check_data(pre, n_features, n_outputs, n_trees, p);
}

int forest_fit_batch_check(int32_t n_problems, int32_t n_features, int32_t n_outputs, int32_t n_trees, int32_t max_features,
                           const ForestProblem *problems) {
    if (n_problems < 1 || n_problems > kForestMaxProblems)
        return fail("forest_fit_batch: n_problems must be in [1, " + std::to_string(kForestMaxProblems) + "]");
    if (!problems) return fail("forest_fit_batch: null buffer");
    int rc = check_shared("forest_fit_batch: ", n_features, n_outputs, n_trees, max_features);
    for (int32_t k = 0; k < n_problems && !rc; ++k) {
        const std::string pre = fit_prefix(false, k);
        if (!(rc = check_samples(pre, problems[k].n_samples))) rc = check_data(pre, n_features, n_outputs, n_trees, problems[k]);
    }
    return rc;
}

int forest_fit_batch(int32_t device, int32_t n_problems, int32_t n_features, int32_t n_outputs, int32_t n_trees,
                     int32_t max_features, const ForestProblem *problems, bool lone, std::vector<std::unique_ptr<Forest>> *out) {
    int rc = set_device(device);
    if (rc) return rc;
    const int32_t K = n_problems, F = n_features, T = n_trees;
    // host side, per problem: CSR of the nonzero-valued entries, class bits, the output layout
    struct Host {
        std::vector<int32_t> row_ptr, col_idx;
        std::vector<uint64_t> ybits;
        uint64_t two = 0;
        int32_t mc = 1, nnz = 0;
        size_t col_ptr, row_idx, val, row_ptr_at, col_idx_at, ybits_at, counts, rand_state, stack;  // offsets in the work space
    };
    std::vector<Host> host(static_cast<size_t>(K));
    std::vector<std::unique_ptr<Forest>> own(static_cast<size_t>(K));
    Layout in;  // uploaded: the descriptor table, then every problem's inputs
    const size_t table_at = in.add<FitArgs>(size_t(K));
    for (int32_t k = 0; k < K; ++k) {
        const ForestProblem &p = problems[k];
        Host &h = host[size_t(k)];
        const int32_t n = p.n_samples;
        h.nnz = p.col_ptr[F];
        h.row_ptr.assign(size_t(n) + 1, 0);
        for (int32_t e = 0; e < h.nnz; ++e)
            if (p.values[e] != 0.0f) h.row_ptr[size_t(p.row_idx[e]) + 1] += 1;
        for (int32_t i = 0; i < n; ++i) h.row_ptr[size_t(i) + 1] += h.row_ptr[size_t(i)];
        h.col_idx.resize(size_t(h.row_ptr[size_t(n)]));
        {
            std::vector<int32_t> fill(h.row_ptr.begin(), h.row_ptr.end() - 1);
            for (int32_t f = 0; f < F; ++f)
                for (int32_t e = p.col_ptr[f]; e < p.col_ptr[f + 1]; ++e)
                    if (p.values[e] != 0.0f) h.col_idx[size_t(fill[size_t(p.row_idx[e])]++)] = f;
        }
        h.ybits.assign(size_t(n), 0);
        for (int32_t o = 0; o < n_outputs; ++o)
            if (p.n_classes[o] == 2) {
                h.two |= uint64_t(1) << o;
                h.mc = 2;
            }
        for (int32_t i = 0; i < n; ++i)
            for (int32_t o = 0; o < n_outputs; ++o)
                if (p.y[size_t(i) * n_outputs + o]) h.ybits[size_t(i)] |= uint64_t(1) << o;
        h.col_ptr = in.add<int32_t>(size_t(F) + 1);
        h.row_idx = in.add<int32_t>(size_t(h.nnz));
        h.val = in.add<float>(size_t(h.nnz));
        h.row_ptr_at = in.add<int32_t>(h.row_ptr.size());
        h.col_idx_at = in.add<int32_t>(h.col_idx.size());
        h.ybits_at = in.add<uint64_t>(h.ybits.size());
        h.counts = in.add<int32_t>(size_t(T) * n);
        h.rand_state = in.add<uint32_t>(size_t(T));
    }
    Layout work = in;  // not uploaded: every problem's stacks, then node_count / max_depth / status of all K x T trees
    for (int32_t k = 0; k < K; ++k) host[size_t(k)].stack = work.add<int32_t>(size_t(T) * (size_t(problems[k].n_samples) + 1) * 6);
    const size_t result_at = work.add<int32_t>(size_t(3) * K * T);
    DeviceBlock<char> d;
    if ((rc = d.alloc(work.bytes, "forest alloc"))) return rc;
    std::vector<unsigned char> up(in.bytes);
    std::vector<FitArgs> table(static_cast<size_t>(K));
    for (int32_t k = 0; k < K; ++k) {
        const ForestProblem &p = problems[k];
        const Host &h = host[size_t(k)];
        const int32_t n = p.n_samples;
        auto f = std::make_unique<Forest>();
        f->device = device;
        f->n_trees = T;
        f->n_features = F;
        f->n_outputs = n_outputs;
        f->max_n_classes = h.mc;
        f->cap = 2 * n - 1;
        f->n_classes.assign(p.n_classes, p.n_classes + n_outputs);
        const size_t slots = size_t(T) * f->cap;
        Layout o;  // memory per forest: 40 bytes a node slot, and 8 n_outputs max_n_classes for its value
        const size_t left = o.add<int32_t>(slots), right = o.add<int32_t>(slots), feature = o.add<int32_t>(slots),
                     n_node = o.add<int32_t>(slots), threshold = o.add<double>(slots), impurity = o.add<double>(slots),
                     weighted = o.add<double>(slots), value = o.add<double>(slots * n_outputs * h.mc),
                     ncls = o.add<uint8_t>(size_t(n_outputs));
        if ((rc = f->d_slab.alloc(o.bytes, "forest alloc"))) return rc;
        char *base = f->d_slab.get();
        f->d_left = reinterpret_cast<int32_t *>(base + left);
        f->d_right = reinterpret_cast<int32_t *>(base + right);
        f->d_feature = reinterpret_cast<int32_t *>(base + feature);
        f->d_n_node = reinterpret_cast<int32_t *>(base + n_node);
        f->d_threshold = reinterpret_cast<double *>(base + threshold);
        f->d_impurity = reinterpret_cast<double *>(base + impurity);
        f->d_weighted = reinterpret_cast<double *>(base + weighted);
        f->d_value = reinterpret_cast<double *>(base + value);
        f->d_ncls = reinterpret_cast<uint8_t *>(base + ncls);
        stage(up, h.col_ptr, p.col_ptr, size_t(F) + 1);
        stage(up, h.row_idx, p.row_idx, size_t(h.nnz));
        stage(up, h.val, p.values, size_t(h.nnz));
        stage(up, h.row_ptr_at, h.row_ptr.data(), h.row_ptr.size());
        stage(up, h.col_idx_at, h.col_idx.data(), h.col_idx.size());
        stage(up, h.ybits_at, h.ybits.data(), h.ybits.size());
        stage(up, h.counts, p.sample_counts, size_t(T) * n);
        stage(up, h.rand_state, p.rand_state, size_t(T));
        FitArgs &A = table[size_t(k)];
        A = FitArgs{};
        A.n = n;
        A.F = F;
        A.n_out = n_outputs;
        A.mc = h.mc;
        A.max_features = max_features;
        A.cap = f->cap;
        A.stack_cap = n + 1;
        A.two_class = h.two;
        A.col_ptr = d.at<int32_t>(h.col_ptr);
        A.row_idx = d.at<int32_t>(h.row_idx);
        A.val = d.at<float>(h.val);
        A.row_ptr = d.at<int32_t>(h.row_ptr_at);
        A.col_idx = d.at<int32_t>(h.col_idx_at);
        A.ybits = d.at<uint64_t>(h.ybits_at);
        A.counts = d.at<int32_t>(h.counts);
        A.rand_state = d.at<uint32_t>(h.rand_state);
        A.stack = d.at<int32_t>(h.stack);
        A.left = f->d_left;
        A.right = f->d_right;
        A.feature = f->d_feature;
        A.n_node = f->d_n_node;
        A.threshold = f->d_threshold;
        A.impurity = f->d_impurity;
        A.weighted = f->d_weighted;
        A.value = f->d_value;
        A.node_count = d.at<int32_t>(result_at) + size_t(k) * T;
        A.max_depth = A.node_count + size_t(K) * T;
        A.status = A.max_depth + size_t(K) * T;
        A.ncls = f->d_ncls;
        own[size_t(k)] = std::move(f);
    }
    stage(up, table_at, table.data(), table.size());
    if ((rc = check_hip(hipMemcpy(d.get(), up.data(), up.size(), hipMemcpyHostToDevice), "forest upload"))) return rc;
    forest_fit_kernel<<<unsigned(K) * unsigned(T), kThreads>>>(d.at<FitArgs>(table_at), T);
    if ((rc = check_hip(hipGetLastError(), "forest fit kernel"))) return rc;
    if ((rc = check_hip(hipDeviceSynchronize(), "forest fit"))) return rc;
    const size_t KT = size_t(K) * T;
    std::vector<int32_t> result(3 * KT);
    if ((rc = check_hip(hipMemcpy(result.data(), d.at<int32_t>(result_at), result.size() * 4, hipMemcpyDeviceToHost),
                        "forest download")))
        return rc;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t *nc = result.data() + size_t(k) * T, *md = nc + KT, *status = md + KT;
        own[size_t(k)]->node_count.assign(nc, nc + T);
        own[size_t(k)]->max_depth.assign(md, md + T);
        for (int32_t t = 0; t < T; ++t)
            if (status[t] != kOk) {
                static const char *what[] = {"ok", "node capacity exceeded", "stack capacity exceeded",
                                             "partition disagrees with the chosen split", "gather overflow"};
                const int st = status[t];
                set_error(fit_prefix(lone, k) + "tree " + std::to_string(t) + ": " + (st > 0 && st < 5 ? what[st] : "unknown status"));
                return GECCO_CRF_EUNSUPPORTED;
            }
    }
    *out = std::move(own);
    return GECCO_CRF_OK;
}

int forest_export(const Forest *f, int32_t tree, int32_t *left, int32_t *right, int32_t *feature, double *threshold,
                  double *impurity, int32_t *n_node_samples, double *weighted_n_node_samples, double *value) {
    if (!f || tree < 0 || tree >= f->n_trees) return fail("forest_export: no such tree");
    int rc = set_device(f->device);
    if (rc) return rc;
    const size_t nc = size_t(f->node_count[size_t(tree)]), off = size_t(tree) * f->cap;
    const size_t vs = size_t(f->n_outputs) * f->max_n_classes;
    struct Item {
        void *dst;
        const void *src;
        size_t bytes;
    } items[] = {{left, f->d_left + off, nc * 4},          {right, f->d_right + off, nc * 4},
                 {feature, f->d_feature + off, nc * 4},    {threshold, f->d_threshold + off, nc * 8},
                 {impurity, f->d_impurity + off, nc * 8},  {n_node_samples, f->d_n_node + off, nc * 4},
                 {weighted_n_node_samples, f->d_weighted + off, nc * 8}, {value, f->d_value + off * vs, nc * vs * 8}};
    for (const Item &it : items)
        if (it.dst && it.bytes && (rc = check_hip(hipMemcpy(it.dst, it.src, it.bytes, hipMemcpyDeviceToHost), "forest export")))
            return rc;
    return GECCO_CRF_OK;
}

int forest_predict_batch_check(const Forest *const *f, int32_t n_problems, const int32_t *n_rows, const double *const *x,
                               double *const *posit) {
    if (n_problems < 1 || n_problems > kForestMaxProblems)
        return fail("forest_predict_batch: n_problems must be in [1, " + std::to_string(kForestMaxProblems) + "]");
    if (!f || !n_rows || !x || !posit) return fail("forest_predict_batch: null buffer");
    for (int32_t k = 0; k < n_problems; ++k)
        if (n_rows[k] < 0) return fail("forest_predict_batch: problem " + std::to_string(k) + ": n_rows must be >= 0");
    for (int32_t k = 0; k < n_problems; ++k) {
        if (!f[k]) return fail("forest_predict_batch: problem " + std::to_string(k) + ": null forest");
        if (f[k]->device != f[0]->device) return fail("forest_predict_batch: every forest must be on one device");
        if (n_rows[k] > 0 && (!x[k] || !posit[k])) return fail("forest_predict_batch: problem " + std::to_string(k) + ": null buffer");
    }
    return GECCO_CRF_OK;
}

int forest_predict_batch(const Forest *const *f, int32_t n_problems, const int32_t *n_rows, const double *const *x,
                         double *const *posit) {
    const int32_t K = n_problems;
    std::vector<PredictArgs> table(static_cast<size_t>(K));
    std::vector<int32_t> block_problem;
    std::vector<size_t> x_at(static_cast<size_t>(K)), p_at(static_cast<size_t>(K));
    Layout in, out;
    for (int32_t k = 0; k < K; ++k) x_at[size_t(k)] = in.add<double>(size_t(n_rows[k]) * f[k]->n_features);
    for (int32_t k = 0; k < K; ++k) {
        p_at[size_t(k)] = out.add<double>(size_t(n_rows[k]) * f[k]->n_outputs);
        const size_t cells = size_t(n_rows[k]) * f[k]->n_outputs;
        table[size_t(k)].block0 = int32_t(block_problem.size());
        block_problem.insert(block_problem.end(), (cells + 255) / 256, k);
    }
    if (block_problem.empty()) return GECCO_CRF_OK;  // no rows at all: no device is touched
    // the table and the block map go up in one copy of their own, after the rows
    const size_t small_at = in.bytes, table_at = in.add<PredictArgs>(size_t(K)), map_at = in.add<int32_t>(block_problem.size());
    int rc = set_device(f[0]->device);
    if (rc) return rc;
    DeviceBlock<char> d;
    if ((rc = d.alloc(in.bytes + out.bytes, "forest predict alloc"))) return rc;
    std::vector<unsigned char> up(in.bytes - small_at);
    for (int32_t k = 0; k < K; ++k) {
        const Forest &fk = *f[k];
        PredictArgs &P = table[size_t(k)];
        P.left = fk.d_left;
        P.right = fk.d_right;
        P.feature = fk.d_feature;
        P.threshold = fk.d_threshold;
        P.value = fk.d_value;
        P.ncls = fk.d_ncls;
        P.n_trees = fk.n_trees;
        P.cap = fk.cap;
        P.n_out = fk.n_outputs;
        P.mc = fk.max_n_classes;
        P.F = fk.n_features;
        P.x = d.at<double>(x_at[size_t(k)]);
        P.n_rows = n_rows[k];
        P.posit = d.at<double>(in.bytes + p_at[size_t(k)]);
        // rows go up straight from the caller's buffer: staging them would be one more pass over the largest input
        if (n_rows[k] > 0 && (rc = check_hip(hipMemcpy(d.at<double>(x_at[size_t(k)]), x[k], size_t(n_rows[k]) * fk.n_features * sizeof(double),
                                                       hipMemcpyHostToDevice),
                                             "forest predict upload")))
            return rc;
    }
    stage(up, table_at - small_at, table.data(), table.size());
    stage(up, map_at - small_at, block_problem.data(), block_problem.size());
    if ((rc = check_hip(hipMemcpy(d.at<unsigned char>(small_at), up.data(), up.size(), hipMemcpyHostToDevice),
                        "forest predict upload")))
        return rc;
    forest_predict_kernel<<<unsigned(block_problem.size()), 256>>>(d.at<PredictArgs>(table_at), d.at<int32_t>(map_at));
    if ((rc = check_hip(hipGetLastError(), "forest predict kernel"))) return rc;
    std::vector<unsigned char> down(out.bytes);
    if ((rc = check_hip(hipMemcpy(down.data(), d.at<unsigned char>(in.bytes), down.size(), hipMemcpyDeviceToHost),
                        "forest predict download")))
        return rc;
    for (int32_t k = 0; k < K; ++k)
        if (n_rows[k] > 0) std::memcpy(posit[k], down.data() + p_at[size_t(k)], size_t(n_rows[k]) * f[k]->n_outputs * sizeof(double));
    return GECCO_CRF_OK;
}

}  // namespace gecco
