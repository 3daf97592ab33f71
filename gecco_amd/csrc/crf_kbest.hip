// The K best label paths of every contig on the whole-contig lattice: list Viterbi.  gl_state (crf_general.hip)
// leaves the raw state scores in GenArgs::state, -infinity at a disallowed (gene, label) pair; nothing else of the marginals'
// workspace is read.  Additions and comparisons only; the file is compiled without floating-point contraction all the same.
//
// The recursion.  For every (gene t, label j) the K best prefix scores in order, delta_t[j][0 .. K):
//   delta_0[j] = [state_0[j]],     delta_t[j] = the K best of { (delta_{t-1}[i][r] + trans[i][j]) + state_t[j] },
// the operation order of the existing Viterbi recursions, so a path's score is the left-to-right sum along the path.  Every
// source list is sorted, so a step is an L-way merge that stops after K outputs: a lane keeps the head candidate of every source
// list and how far it has read each, takes the best head, and replaces it by the next entry of that list.
//   The order is total: greater score first; among equal scores the smaller source label i, then the smaller source rank r; at
// the end of the contig the L final lists merge by the same rule (smaller last label, then smaller rank).  In exact arithmetic
// that is "score descending, then the reversed path (y_{T-1}, ..., y_0) ascending".  Rank 0 is the Viterbi path (strict `<`
// update, first arg max).  A candidate whose score is -infinity does not exist: it is never emitted, and a rank that no path
// fills stays empty (score -infinity, back-pointer 0xffff, labels -1).  The order is total and merges preserve it, so rank k of
// a call with K' < K is rank k of the call with K: the lists of the smaller call are prefixes of the larger call's.
//
// gl_kbest_forward<LP>: the frame of crf_contig_walk.hpp (group geometry, columns in LDS, gene loop, group arg max), one lane per
// destination label.  The two generations of lists are the frame's columns, [2][64 rows][K | 1] doubles.  Heads and read positions
// are registers, indexed by unrolled loops only.  Back-pointers: uint16 per (gene, label, rank), (previous label << 8) | previous
// rank.  The final merge runs across the group's lanes (every lane the head of its own list, the rank as the arg max's payload)
// and leaves, per (contig, rank), the last label and its rank in `fin`, the score, and the number of paths.
// gl_kbest_backtrack: one lane per (contig, rank) follows the back-pointers from the last gene to the first and writes
// y[g * K + k], gene-major like the sampler's output: a step's stores are consecutive bytes.
// A contig is one sequential walk; it is not chunked (profiles/EXPERIMENTS.md has the parallel-in-T idea).
#include "crf_contig_walk.hpp"

#include <cmath>

namespace gecco {
namespace {

constexpr int kKBack = kWalkBack;  // lanes per workgroup of the backtrack
constexpr uint16_t kNoPath = 0xffffu;

template <int LP>
__global__ void __launch_bounds__(kWalkLanes) gl_kbest_forward(const double *__restrict__ state, const double *__restrict__ trans,
                                                               const int32_t *__restrict__ contig_ptr, const int L,
                                                               const int n_contigs, const int K, uint16_t *__restrict__ back,
                                                               uint16_t *__restrict__ fin, double *__restrict__ score,
                                                               int32_t *__restrict__ n_paths) {
    extern __shared__ double lists[];  // [2][kWalkLanes][K | 1]
    const double ninf = kWalkNinf;
    const WalkGroup<LP> g(contig_ptr, n_contigs, L);
    const int lane = g.lane, j = g.j, T = g.T;
    double tcol[LP];
    g.load_trans(trans, L, tcol);
    const double *st = g.column(state, L);
    const WalkColumns cols(lists, K);
    const int KS = cols.KS;
    cols.fill(lane, 0, g.state_at(st, L, 0 < T, 0));
    __syncthreads();  // (one wave)
    // one gene: the lane's L-way merge of the previous generation's lists, K outputs
    const auto step = [&](const int t, const double s_t) {
        const bool act = t < T;
        const double *prev = cols.gen(t - 1) + g.row0 * KS;
        double *mine = cols.gen(t) + lane * KS;
        double cand[LP];
        int ptr[LP];
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            cand[i] = prev[i * KS] + tcol[i];
            ptr[i] = 0;
        }
        uint16_t *bk = back + (static_cast<size_t>(g.g0 + (act ? t : 0)) * L + g.jj) * K;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            double best = cand[0];
            int arg = 0, r = ptr[0];
#pragma unroll
            for (int i = 1; i < LP; ++i) {  // ascending i, strict `>`: the smaller source label wins a tie
                const bool take = cand[i] > best;
                best = take ? cand[i] : best;
                arg = take ? i : arg;
                r = take ? ptr[i] : r;
            }
            const int p = r + 1;  // the next entry of the winner's list: equal scores of one source leave in rank order
            const double nd = prev[arg * KS + (p < K ? p : 0)];
            const double next = p < K ? nd : ninf;
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                const bool hit = i == arg;
                cand[i] = hit ? next + tcol[i] : cand[i];
                ptr[i] = hit ? p : ptr[i];
            }
            const double out = best + s_t;
            if (act) {
                mine[k] = out;
                if (g.on) bk[k] = out > ninf ? static_cast<uint16_t>((arg << 8) | r) : kNoPath;
            }
        }
        __syncthreads();
    };
    contig_walk(1, T, [&](int t) { return g.state_at(st, L, t < T, t); }, step);
    // the final merge: every lane the head of its own label's last list, the group's arg max
    const double *fl = cols.gen(T - 1) + lane * KS;
    int p = 0, count = 0;
    for (int k = 0; k < K; ++k) {
        double v = (T > 0 && p < K) ? fl[p < K ? p : 0] : ninf;
        int bj = j, bp = p;
        group_argmax<LP>(v, bj, bp);
        const bool exists = v > ninf;
        p += (exists && bj == j) ? 1 : 0;
        count += exists ? 1 : 0;
        if (g.valid && j == 0) {
            const size_t o = static_cast<size_t>(g.c) * K + k;
            fin[o] = exists ? static_cast<uint16_t>((bj << 8) | bp) : kNoPath;
            score[o] = exists ? v : ninf;
        }
    }
    if (g.valid && j == 0) n_paths[g.c] = count;
}

__global__ void __launch_bounds__(kKBack) gl_kbest_backtrack(const uint16_t *__restrict__ back, const uint16_t *__restrict__ fin,
                                                             const int32_t *__restrict__ contig_ptr, const int L,
                                                             const int n_contigs, const int K, int8_t *__restrict__ y) {
    const size_t gid = static_cast<size_t>(blockIdx.x) * kKBack + threadIdx.x;
    const size_t c = gid / static_cast<size_t>(K);
    const int k = static_cast<int>(gid - c * static_cast<size_t>(K));
    if (c >= static_cast<size_t>(n_contigs)) return;
    const int g0 = contig_ptr[c], T = contig_ptr[c + 1] - g0;
    if (T <= 0) return;
    const size_t KK = static_cast<size_t>(K);
    int8_t *col = y + static_cast<size_t>(g0) * KK + static_cast<size_t>(k);
    const uint16_t f = fin[c * KK + static_cast<size_t>(k)];
    if (f == kNoPath) {
        for (int t = 0; t < T; ++t) col[static_cast<size_t>(t) * KK] = -1;
        return;
    }
    int lab = f >> 8, r = f & 0xff;
    for (int t = T - 1; t >= 0; --t) {
        if (lab >= L || r >= K) lab = r = 0;  // (cannot happen: an emitted entry points at an emitted entry; no address leaves the workspace)
        col[static_cast<size_t>(t) * KK] = static_cast<int8_t>(lab);
        if (t == 0) break;
        const uint16_t b = back[(static_cast<size_t>(g0 + t) * L + lab) * KK + static_cast<size_t>(r)];
        lab = b >> 8;
        r = b & 0xff;
    }
}

template <int LP>
void launch_forward(const GenArgs &a, int32_t K, uint16_t *back, uint16_t *fin, double *score, int32_t *n_paths, hipStream_t stream) {
    hipLaunchKernelGGL(gl_kbest_forward<LP>, dim3(walk_blocks<LP>(a.n_contigs)), dim3(kWalkLanes), walk_lds_bytes(K), stream, a.state,
                       a.trans, a.contig_ptr, a.L, a.n_contigs, K, back, fin, score, n_paths);
}

}  // namespace

size_t kbest_back_bytes(int64_t n_genes, int32_t L, int32_t k) {
    return static_cast<size_t>(n_genes) * static_cast<size_t>(L) * static_cast<size_t>(k) * sizeof(uint16_t);
}
size_t kbest_fin_bytes(int32_t n_contigs, int32_t k) { return static_cast<size_t>(n_contigs) * static_cast<size_t>(k) * sizeof(uint16_t); }

hipError_t launch_gen_kbest(const GenArgs &a, int32_t k, uint16_t *back, uint16_t *fin, int8_t *y, double *score, int32_t *n_paths,
                            hipStream_t stream) {
    if (a.L <= 0 || a.L > kGenMaxL || k < 1 || k > kMaxKBest) return hipErrorNotSupported;
    if (a.n_contigs <= 0) return hipSuccess;
    if (!a.state || !a.trans || !back || !fin || !y || !score || !n_paths) return hipErrorNotSupported;
    dispatch_lp(a.L, [&](auto lp) { launch_forward<lp>(a, k, back, fin, score, n_paths, stream); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lanes = static_cast<size_t>(a.n_contigs) * static_cast<size_t>(k);
    const unsigned blocks = static_cast<unsigned>((lanes + kKBack - 1) / kKBack);
    hipLaunchKernelGGL(gl_kbest_backtrack, dim3(blocks), dim3(kKBack), 0, stream, back, fin, a.contig_ptr, a.L, a.n_contigs, k, y);
    return hipGetLastError();
}

}  // namespace gecco
