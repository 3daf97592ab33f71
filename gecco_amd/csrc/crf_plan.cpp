#include "crf_plan.hpp"

#include <algorithm>
#include <functional>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/gecco_crf.h"
#include "crf_session.hpp"

namespace gecco {

int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return GECCO_CRF_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return GECCO_CRF_ENODEV;
    if (e == hipErrorOutOfMemory) return GECCO_CRF_ENOMEM;
    return GECCO_CRF_EHIP;
}

Model::~Model() {
    for (auto &e : sessions) session_destroy(e.second);  // before the tables their plans point at
    for (DeviceTables *t : dev_tables) {
        if (!t) continue;
        DeviceScope scope(t->device);
        delete t;  // (the blocks free themselves; without a usable device the allocations die with the context)
    }
}

int get_device_tables(const Model &m, int device, const DeviceTables **out) {
    std::lock_guard<std::mutex> lock(m.dev_mutex);
    for (DeviceTables *t : m.dev_tables)
        if (t && t->device == device) {
            *out = t;
            return GECCO_CRF_OK;
        }
    int rc = set_device(device);
    if (rc) return rc;
    auto t = std::make_unique<DeviceTables>();
    t->device = device;
    const size_t A = size_t(m.A), L = size_t(m.L);
    std::vector<double> et(L * L);
    for (size_t i = 0; i < L * L; ++i) et[i] = std::exp(m.trans[i]);
    for (double v : m.state) t->wmax_abs = std::max(t->wmax_abs, std::fabs(v));
    for (double v : m.trans) t->tmax_abs = std::max(t->tmax_abs, std::fabs(v));
    if (!m.trans.empty()) t->tmax = *std::max_element(m.trans.begin(), m.trans.end());
    for (size_t i = 0; i < L * L; ++i)
        if (et[i] != 0.0) t->tmax_abs_live = std::max(t->tmax_abs_live, std::fabs(m.trans[i]));
    rc = t->wtab.upload(m.state.data(), A * L, "upload state weights");
    if (!rc) rc = t->exp_trans.upload(et.data(), L * L, "upload transitions");
    if (!rc) rc = t->trans.upload(m.trans.data(), L * L, "upload transitions");
    if (!rc && m.L == 2) {
        std::vector<double2> w2(A ? A : 1);
        for (int label = 0; label < 2 && !rc; ++label) {
            for (size_t a = 0; a < A; ++a) w2[a] = make_double2(m.state[a * 2 + (1 - label)], m.state[a * 2 + label]);
            rc = t->wtab2[label].upload(w2, "upload state weight pairs");
        }
        // r = mu01 exp(d) in the window kernel (mu_exp_tab): exp(d) = 2^e 2^(j/32) exp(r'), |r'| <= ln2/64; the table holds
        // mu01 2^(j/32), rounded once from extended precision
        for (int label = 0; label < 2 && !rc; ++label) {
            const int o = 1 - label;
            auto T = [&](int i, int j) { return (long double)m.trans[size_t(i) * 2 + j]; };
            const long double lmu = T(o, label) + T(label, o) - 2.0L * T(o, o);
            double tab[32];
            for (int j = 0; j < 32; ++j) tab[j] = double(expl(lmu + (long double)j * 0.693147180559945309417232121458L / 32.0L));
            rc = t->rtab[label].upload(tab, 32, "upload exp table");
        }
        // the factor table of the product-form slot constants, in the same precision (build_slot_table)
        for (int label = 0; label < 2 && !rc; ++label) {
            SlotTable st;
            build_slot_table(m, label, st);
            t->slot_dmax = st.dmax;
            t->slot_prod_max_cnt = st.prod_max_cnt;
            rc = t->ptab[label].upload(reinterpret_cast<const double2 *>(st.pairs.data()), A + 1, "upload slot factor table");
        }
    }
    if (rc) return rc;
    if (m.L == 2) {
        for (int label = 0; label < 2; ++label) {
            DeviceTables::WinConsts &c = t->win[label];
            // exp() of differences only: every constant is a ratio of transition weights
            const int o = 1 - label;
            auto T = [&](int i, int j) { return m.trans[size_t(i) * 2 + j]; };
            c.mu01 = std::exp(T(o, label) + T(label, o) - 2.0 * T(o, o));
            c.rho = std::exp(T(label, label) + T(o, o) - T(o, label) - T(label, o));  // mu11 / mu01
            const double kappa = std::exp(T(label, o) - T(o, o));
            c.kappa_over_mu01 = std::exp(T(o, o) - T(o, label));                       // kappa / mu01
            c.inv_kappa = 1.0 / kappa;
            const double mx = *std::max_element(m.trans.begin(), m.trans.end());
            auto G = [&](int i, int j) { return std::exp(m.trans[size_t(i) * 2 + j] - mx); };
            c.g00 = G(o, o);
            c.g01 = G(o, label);
            c.g10 = G(label, o);
            c.g11 = G(label, label);
            fill_exp_coefficients(c.expc);
            c.ratio_zmax = 1.0e250;
            // the running product starts at mu01: every partial product lies within e^(+-(|ln mu01| + cnt dmax)), which has to
            // stay within e^+-700 (the normal range of a double ends at e^-708 and e^709)
            const double room = 700.0 - std::fabs(T(o, label) + T(label, o) - 2.0 * T(o, o));
            c.prod_cnt = room > 0.0 ? std::min(t->slot_prod_max_cnt, slot_prod_max_cnt(t->slot_dmax * (700.0 / room))) : 0;
        }
        DeviceTables::SeqConsts &q = t->seq;
        q.mx = *std::max_element(m.trans.begin(), m.trans.end());
        q.m00 = std::exp(m.trans[0] - q.mx);
        q.m01 = std::exp(m.trans[1] - q.mx);
        q.m10 = std::exp(m.trans[2] - q.mx);
        q.m11 = std::exp(m.trans[3] - q.mx);
        const double lo = *std::min_element(m.trans.begin(), m.trans.end());
        q.raw_fold = (q.mx - lo) * double(kSeqGenesPerLane) < 600.0 ? 1 : 0;
        q.v_lo = m.trans[1] - m.trans[3];
        q.v_hi = m.trans[0] - m.trans[2];
        q.v_k = m.trans[3] - m.trans[0];
        q.v_exact = 1;
        fill_exp_coefficients(q.expc);
        t->consts_ok = true;
    }
    *out = t.get();
    m.dev_tables.push_back(t.release());
    return GECCO_CRF_OK;
}

int Arena::reserve(size_t bytes, const char *what) {
    if (bytes <= cap && h) return GECCO_CRF_OK;
    release();
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);  // head room: chunks of one batch differ a little
    // (mapped + portable: the kernels of ANY device of a session may read the block where the host wrote it)
    int rc = check_hip(hipHostMalloc(reinterpret_cast<void **>(&h), want, hipHostMallocMapped | hipHostMallocPortable), what);
    if (rc) return rc;
    if ((rc = check_hip(hipMalloc(reinterpret_cast<void **>(&d), want), what))) {
        (void)hipHostFree(h);
        h = nullptr;
        return rc;
    }
    cap = want;
    return GECCO_CRF_OK;
}

void Arena::release() {
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = d = nullptr;
    cap = 0;
}

// The blocks and the side stream free themselves after this body, with the plan's device current; `home` then hands the
// caller's device back.
Plan::~Plan() {
    if (device < 0) return;
    home.enter(device);
    tables.release();
    seq.release();
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
}

// Steps after which the un-normalised DP vectors are rescaled by a power of two.
// The kernel keeps alpha/beta un-normalised in a transformed basis (crf_kernels.hip):
// emissions max-normalised to (0,1], transitions divided by m00.  With
//   bits  = log2(max(M)/min(M)),  cbits = log2(max(M)/m00)      (M = exp(trans))
// the larger component of alpha~ after k steps lies in [2^-(bits(k+1)), 2^(k(1+cbits)+bits)],
// that of beta~ in [2^-(bits(2k+1)), 2^(k(1+cbits)+bits)] with min/max >= 2^-(2 bits), so a
// candidate pair has max(x,y) in [2^-(bits(3k+4)), 2^(2k(1+cbits)+2bits)].  Comparing two
// candidates multiplies two such numbers; both products stay inside fp64's normal range if
//   bits*(3P+4) <= 500   and   2P(1+cbits) + 2 bits <= 500
// for a rescale period P.  GECCO's embedded model: bits = 7.6, cbits <= 0.15 -> P = 20 >=
// W-1, i.e. no rescale inside a 20-gene window (mask = 0).
static bool rescale_mask_for(const Model &m, int W, uint32_t *mask) {
    *mask = 0;
    double lo = m.trans[0], hi = m.trans[0];
    for (double t : m.trans) {
        lo = std::min(lo, t);
        hi = std::max(hi, t);
    }
    if (!std::isfinite(lo) || !std::isfinite(hi)) return false;
    const double ln2 = std::log(2.0);
    const double bits = (hi - lo) / ln2;
    // m00 is trans[other][other]; `other` is 0 or 1 depending on the queried label
    const double cbits = (hi - std::min(m.trans[0], m.trans[3])) / ln2;
    double pf = (500.0 - 2.0 * bits) / (2.0 * (1.0 + cbits));
    if (bits > 0.0) pf = std::min(pf, (500.0 / bits - 4.0) / 3.0);
    pf = std::floor(pf);
    if (pf < 1.0) return false;
    if (pf >= double(W)) return true;
    const int P = int(pf);
    for (int k = P; k < W && k < 32; k += P) *mask |= (1u << k);
    return true;
}

// bits [lo, hi) of a bit array
static inline void set_bit_range(uint64_t *bits, int64_t lo, int64_t hi) {
    if (lo >= hi) return;
    const int64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
    const uint64_t m0 = ~0ull << (lo & 63), m1 = ~0ull >> (63 - ((hi - 1) & 63));
    if (w0 == w1) {
        bits[w0] |= m0 & m1;
        return;
    }
    bits[w0] |= m0;
    for (int64_t w = w0 + 1; w < w1; ++w) bits[w] = ~0ull;
    bits[w1] |= m1;
}

// The tile table of a window kernel whose workgroups own `tile_out` output slots each: per tile the contigs in reach and
// whether its slots map to genes by a constant shift.  irr_prefix[k + 1] - irr_prefix[k] = 1 where contig k is padded or a
// skipped contig lies between it and contig k + 1.
static void fill_tile_desc(const Plan &p, const std::vector<int32_t> &irr_prefix, int32_t tile_out, int32_t ntiles, int4 *out) {
    const int32_t W = p.W;
    // contigs in reach of a workgroup: both ends of the reach only move forward from tile to tile
    int first = 0, last = 0;
    for (int32_t b = 0; b < ntiles; ++b) {
        const int64_t q0 = int64_t(b) * tile_out - (W - 1);
        const int64_t q_lo = std::max<int64_t>(q0, 0);
        const int64_t q_hi = std::min<int64_t>(q0 + tile_out + 2 * (W - 1) - 1, p.S - 1);
        while (first + 1 < p.K && p.c_slot[first + 1] <= q_lo) ++first;  // largest k with c_slot[k] <= q_lo
        if (last < first) last = first;
        while (last + 1 < p.K && p.c_slot[last + 1] <= q_hi) ++last;
        // regular: no padded contig in reach and no skipped contig between the contigs in reach
        // (a gap after the last contig is harmless)
        const bool padded_or_gap =
            (irr_prefix[last] - irr_prefix[first]) != 0 || (p.c_slot[last + 1] - p.c_slot[last] != p.c_n[last]);
        const int shift = p.c_gene[first] - p.c_slot[first];
        out[b] = make_int4(shift, first, last, padded_or_gap ? 0 : 1);
    }
}

int plan_build(const Model &m, int device, const int32_t *contig_ptr, int32_t n_contigs, int32_t W, int32_t step,
               int32_t pad, Plan &p, hipStream_t upload_stream, bool sync) {
    // same checks, same order as gecco/_meta.py:127-130
    if (W <= 0) {
        set_error("Window size must be strictly positive");
        return GECCO_CRF_EINVAL;
    }
    if (step <= 0 || step > W) {
        set_error("Window step must be strictly positive and under `window_size`");
        return GECCO_CRF_EINVAL;
    }
    if (n_contigs < 0 || (n_contigs > 0 && !contig_ptr)) {
        set_error("bad contig_ptr");
        return GECCO_CRF_EINVAL;
    }
    if (p.device >= 0 && p.device != device) {
        set_error("a plan cannot move to another device");
        return GECCO_CRF_EINVAL;
    }
    p.gen_small = false;
    p.all_ntiles = -1;
    p.gen_tab[0].chunk = p.gen_tab[1].chunk = 0;  // (chunk tables of the previous contigs)
    p.gen_wave_tmax = p.gen_wave_tmax_f = INT32_MIN;
    p.pipe = Plan::Pipe{};  // (score differences and CSR pointers of the previous layout)
    p.csr_begin = p.csr_end = -1;  // (the owner sets them after the build, for the batch at hand)
    p.model = &m;
    p.device = device;
    p.W = W;
    p.step = step;
    p.pad = pad ? 1 : 0;
    p.n_contigs = n_contigs;
    // a slice of a larger batch is accepted: gene offsets are taken relative to its first contig
    const int64_t g_base = n_contigs ? contig_ptr[0] : 0;
    {
        const int64_t ng = n_contigs ? int64_t(contig_ptr[n_contigs]) - g_base : 0;
        if (ng < 0) {
            set_error("contig_ptr must be non-decreasing");
            return GECCO_CRF_EINVAL;
        }
        p.n_genes = int32_t(ng);
    }
    p.contig_ptr.resize(n_contigs ? size_t(n_contigs) + 1 : 0);
    p.c_slot.clear();
    p.c_gene.clear();
    p.c_n.clear();
    p.skipped.clear();
    p.seq_ready = false;
    p.n_max = 0;
    int64_t S = 0;
    p.n_windows = 0;
    if (n_contigs) p.contig_ptr[0] = 0;
    for (int32_t c = 0; c < n_contigs; ++c) {
        const int32_t g0 = int32_t(contig_ptr[c] - g_base), n = contig_ptr[c + 1] - contig_ptr[c];
        p.contig_ptr[size_t(c) + 1] = g0 + n;
        p.n_max = std::max(p.n_max, n);
        if (n < 0) {
            set_error("contig_ptr must be non-decreasing");
            return GECCO_CRF_EINVAL;
        }
        if (n == 0) continue;  // cannot occur in the reference (groupby never yields empty groups)
        int32_t np = n;
        if (n < W) {
            if (!p.pad) {  // crf/__init__.py:228-234: contig skipped, genes keep "no prediction"
                p.skipped.push_back(make_int2(g0, g0 + n));
                continue;
            }
            np = W;  // :226-227
        }
        p.c_slot.push_back(int32_t(S));
        p.c_gene.push_back(g0);
        p.c_n.push_back(n);
        S += np;
        p.n_windows += np - W + 1;  // :239 (ignores step, like the reference)
        if (S > INT32_MAX - 4096) {
            set_error("batch too large: more than 2^31 padded gene slots");
            return GECCO_CRF_EUNSUPPORTED;
        }
    }
    p.K = int32_t(p.c_gene.size());
    p.S = int32_t(S);
    p.c_slot.push_back(p.S);

    if (m.L < 1 || m.L > kGenMaxL) {
        set_error("models with more than 32 labels are not supported");
        return GECCO_CRF_EUNSUPPORTED;
    }
    {
        const char *env = std::getenv("GECCO_CRF_FORCE_GENERAL");
        // (valued and masked state scores exist in gl_state alone; region posteriors, sampled paths and the K best paths read the
        // any-L workspace)
        p.general = m.L != 2 || (env && env[0] == '1') || p.valued || p.masked || p.lattice;
    }
    p.fast_ok = (!p.general && W <= kWinMaxW && rescale_mask_for(m, W, &p.rescale_mask));
    {
        static const bool env_reference = [] {
            const char *env = std::getenv("GECCO_CRF_REFERENCE_BITS");
            return env && env[0] == '1';
        }();
        // (the environment switch is for windowed marginals of 2-label models: a Viterbi-only or whole-contig layout, or another
        // label count, keeps its kernels; an explicit request -- reference_bits -- for an unsupported shape is an error)
        p.reference_now = !p.valued && !p.masked && (p.reference_bits || (env_reference && p.windowed_use && m.L == 2 && reference_bits_ok(m.L, W)));
        if (p.reference_now) {
            if (!reference_bits_ok(m.L, W)) {
                set_error("reference-bits mode serves 2-label models and windows of at most 32 genes");
                return GECCO_CRF_EUNSUPPORTED;
            }
            // (the fast kernels' by-products -- score differences for the decoder, p in host memory -- are theirs alone: the
            // decoder sums its state scores itself, p goes through device memory)
            p.general = false;
            p.fast_ok = false;
        }
    }
    {
        const char *env = std::getenv("GECCO_CRF_FORCE_GENERIC");
        p.force_generic = env && env[0] == '1';
    }
    if (p.force_generic) p.fast_ok = false;
    {
        const char *env = std::getenv("GECCO_CRF_TILES_PER_WG");
        p.tiles_per_wg = (env && env[0] >= '1' && env[0] <= '3' && !env[1]) ? env[0] - '0' : kWinTilesPerWg;
        // A batch that leaves most wave slots of the chip empty runs ONE tile per workgroup: the two tiles of a workgroup are a
        // chain, and with a wave or two per SIMD nothing else hides a tile's latency (C2, 0.2 M genes: window kernel 10.0 -> 7.9 us).
        // A batch of one workgroup keeps two (crf_windowed_small_l2).
        if (!env && !p.general && W == 20 && p.S > 2 * (kWinThreads - (W - 1)) && p.S <= kWinTiles1MaxSlots) p.tiles_per_wg = 1;
        // windows other than GECCO's 20 take the dynamic-W instantiation, whose two-tile form spills scalar registers: one tile
        // (tools/window_size_sweep.py, 1 M genes, two / one tile: W = 5 19.9 / 17.1 us, W = 10 22.9 / 19.2, W = 32 76 / 69)
        if (!env && !p.general && W != 20) p.tiles_per_wg = 1;
    }
    // window-start flags per slot (_meta.py:131: starts at 0, step, 2*step, ... <= n' - W)
    // one zero word in front (slots -64 .. -1: the lead-in of the first workgroup) and kStartBitsTail behind (the reach of
    // the last one): the window kernels index the array with any slot of their reach, unclamped
    constexpr size_t kStartBitsTail = 24;
    p.start_bits.assign(1 + size_t(p.S) / 64 + 2 + kStartBitsTail, 0);
    uint64_t *const start_bits = p.start_bits.data() + 1;  // word of slot 0
    // irregular[k]: contig k is padded, or a skipped contig lies between it and contig k+1
    std::vector<int32_t> &irr_prefix = p.irr_prefix;
    irr_prefix.assign(size_t(p.K) + 1, 0);
    for (int32_t k = 0; k < p.K; ++k) {
        const int32_t s0 = p.c_slot[k], np = p.c_slot[k + 1] - s0;
        if (step == 1) {
            set_bit_range(start_bits, s0, int64_t(s0) + np - W + 1);
        } else {
            for (int32_t pos = 0; pos + W <= np; pos += step) {
                const int64_t q = int64_t(s0) + pos;
                start_bits[size_t(q >> 6)] |= 1ull << (q & 63);
            }
        }
        const bool padded = np != p.c_n[k];
        const bool gap_after = k + 1 < p.K && p.c_gene[k + 1] != p.c_gene[k] + p.c_n[k];
        irr_prefix[k + 1] = irr_prefix[k] + ((padded || gap_after) ? 1 : 0);
    }
    // slot space = gene space everywhere: no contig padded, none skipped (empty contigs take no slots and no genes)
    p.all_regular = p.skipped.empty() && p.S == p.n_genes && irr_prefix[size_t(p.K)] == 0;
    if (p.general && m.L >= 3 && gen_small_ok(m.L, W, m.trans.data()) && !std::getenv("GECCO_CRF_GENERAL_GROUPS")) {
        // a handful of labels: one lane per window start (GECCO_CRF_GENERAL_GROUPS=1: the lane-group kernel, tests / A/B)
        p.kernel_name = m.L > 8 ? "gl_windowed_mfma" : "gl_windowed_small";  // (9 to 32 labels: sixteen windows per wave on the matrix cores)
        p.gen_small = true;
        p.tile_out = gen_small_tile_out(W);
    } else {
        p.kernel_name = p.reference_now ? "crf_windowed_reference_l2" : p.general ? "gl_windowed" : windowed_kernel_name(W, m.L, p.fast_ok);
        p.tile_out = windowed_tile_out(W, m.L, p.tiles_per_wg);
    }
    p.ntiles = p.S > 0 ? (p.S + p.tile_out - 1) / p.tile_out : 0;
    p.tile_desc.resize(p.ntiles);
    fill_tile_desc(p, irr_prefix, p.tile_out, p.ntiles, p.tile_desc.data());
    if (device < 0) return GECCO_CRF_OK;

    int rc = set_device(device);
    if (rc) return rc;
    if ((rc = get_device_tables(m, device, &p.tables_model))) return rc;
    // one pinned block -> one device block, one copy
    Carver blk;
    auto take = [&](size_t bytes) { return blk.take(bytes ? bytes : 1); };  // (an empty table keeps a place of its own)
    const size_t o_slot = take(p.c_slot.size() * 4), o_gene = take(p.c_gene.size() * 4), o_n = take(p.c_n.size() * 4),
                 o_tile = take(p.tile_desc.size() * sizeof(int4)), o_bits = take(p.start_bits.size() * 8),
                 o_skip = take(p.skipped.size() * sizeof(int2)), o_cptr = take(p.contig_ptr.size() * 4);
    const size_t off = blk.off;
    if ((rc = p.tables.reserve(off, "plan tables"))) return rc;
    char *h = p.tables.h, *d = p.tables.d;
    if (p.tables_in_host_memory) {
        void *dv = nullptr;
        if ((rc = check_hip(hipHostGetDevicePointer(&dv, h, 0), "hipHostGetDevicePointer"))) return rc;
        d = static_cast<char *>(dv);
    }
    auto put = [&](size_t o, const void *src, size_t bytes) {
        if (bytes) std::memcpy(h + o, src, bytes);
    };
    put(o_slot, p.c_slot.data(), p.c_slot.size() * 4);
    put(o_gene, p.c_gene.data(), p.c_gene.size() * 4);
    put(o_n, p.c_n.data(), p.c_n.size() * 4);
    put(o_tile, p.tile_desc.data(), p.tile_desc.size() * sizeof(int4));
    put(o_bits, p.start_bits.data(), p.start_bits.size() * 8);
    put(o_skip, p.skipped.data(), p.skipped.size() * sizeof(int2));
    put(o_cptr, p.contig_ptr.data(), p.contig_ptr.size() * 4);
    p.d_c_slot = reinterpret_cast<int32_t *>(d + o_slot);
    p.d_c_gene = reinterpret_cast<int32_t *>(d + o_gene);
    p.d_c_n = reinterpret_cast<int32_t *>(d + o_n);
    p.d_tile_desc = reinterpret_cast<int4 *>(d + o_tile);
    p.d_start_bits = reinterpret_cast<uint64_t *>(d + o_bits) + 1;  // (the word of slot 0)
    p.d_skipped = reinterpret_cast<int2 *>(d + o_skip);
    p.d_contig_ptr = reinterpret_cast<int32_t *>(d + o_cptr);
    if (p.tables_in_host_memory) return GECCO_CRF_OK;
    if (p.tables_by_kernel && !sync) {
        void *dv = nullptr;
        if ((rc = check_hip(hipHostGetDevicePointer(&dv, h, 0), "hipHostGetDevicePointer"))) return rc;
        return check_hip(launch_copy_block(dv, d, off, upload_stream), "plan tables launch");
    }
    if ((rc = check_hip(hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, upload_stream), "upload plan tables"))) return rc;
    if (sync && (rc = check_hip(hipStreamSynchronize(upload_stream), "upload plan tables"))) return rc;
    return GECCO_CRF_OK;
}

// ---- any number of labels (crf_general.hip) ------------------------------------------------
namespace {
// A contig longer than this sends the whole batch through the chunked whole-contig kernels (crf_general.hip):
// below it, one group of lanes per contig walking it sequentially is the cheaper arrangement.
constexpr int32_t kGenLongContig = 2048;

// chunk_min_len >= 0: only contigs LONGER than that get chunks (the second table set); -1: every contig
int fill_gen_args(Plan &p, const DeviceCsr &csr, GenArgs &a, bool whole_contig = false,
                  hipStream_t stream = nullptr, int32_t chunk_min_len = -1) {
    const Model &m = *p.model;
    const size_t n = size_t(p.n_genes), L = size_t(m.L);
    // Whole-contig recursions go through the chunked kernels for EVERY batch (round 3): a contig-sequential group of lanes
    // is a dependent chain as long as the contig, and a batch of 200-gene contigs has three to seven chunks' worth of
    // parallelism inside every contig (1 000 contigs x 200 genes, L = 3: Viterbi 0.40 -> 1.5 G genes/s, marginals 0.17 ->
    // 1.1 G).  Chunks of 32 genes for batches of short contigs, 64 when a contig is longer than kGenLongContig (the walk
    // over a contig's chunks is the serial part).  GECCO_CRF_GENERAL_CHUNKED=0: the contig-sequential kernels (tests).
    bool chunked = whole_contig;
    if (whole_contig)
        if (const char *env = std::getenv("GECCO_CRF_GENERAL_CHUNKED")) chunked = env[0] == '1';  // tests: force either path
    size_t nch = 0;
    if (chunked) {
        // the chunk tables depend on the plan's contigs and the chunk length only: built and uploaded once
        bool has_long = false;
        for (int32_t c = 0; c < p.n_contigs && !has_long; ++c) has_long = p.contig_ptr[c + 1] - p.contig_ptr[c] > kGenLongContig;
        int32_t C = has_long ? gen_chunk_genes() : gen_chunk_genes() / 2;
        if (const char *env = std::getenv("GECCO_CRF_GENERAL_CHUNK")) {
            const int v = std::atoi(env);
            if (v >= 4 && v <= 4096) C = v;
        }
        std::lock_guard<std::mutex> lock(p.ws_mutex);
        Plan::GenTab &tab = p.gen_tab[chunk_min_len >= 0 ? 1 : 0];
        if (!tab.d.get() || tab.chunk != C || tab.min_len != chunk_min_len) {
            std::vector<int32_t> ch_g0, ch_contig, cc_ptr;
            cc_ptr.push_back(0);
            for (int32_t c = 0; c < p.n_contigs; ++c) {
                if (p.contig_ptr[c + 1] - p.contig_ptr[c] > chunk_min_len) {
                    for (int32_t g = p.contig_ptr[c]; g < p.contig_ptr[c + 1]; g += C) {
                        ch_g0.push_back(g);
                        ch_contig.push_back(c);
                    }
                }
                cc_ptr.push_back(int32_t(ch_g0.size()));
            }
            ch_g0.push_back(p.n_genes);  // (a chunk ends where the next one starts or where its contig does: gl_chunk_end)
            const size_t n_ch = ch_contig.size();
            Carver img_at;
            img_at.take(ch_g0.size() * 4);
            const size_t o1 = img_at.take(n_ch * 4 + 4), o2 = img_at.take(cc_ptr.size() * 4), total = img_at.off;
            tab.chunk = 0;
            int rc = tab.d.alloc(total, "hipMalloc chunk tables");
            if (rc) return rc;
            std::vector<char> img(total, 0);
            std::memcpy(img.data(), ch_g0.data(), ch_g0.size() * 4);
            std::memcpy(img.data() + o1, ch_contig.data(), n_ch * 4);
            std::memcpy(img.data() + o2, cc_ptr.data(), cc_ptr.size() * 4);
            if ((rc = check_hip(hipMemcpy(tab.d.get(), img.data(), total, hipMemcpyHostToDevice), "upload chunk tables"))) return rc;
            tab.chunk = C;
            tab.min_len = chunk_min_len;
            tab.nch = n_ch;
            tab.off1 = o1;
            tab.off2 = o2;
        }
        nch = tab.nch;
    }
    // in front of everything, at a fixed place: the chunked Viterbi's counters (4 x u32) and contig flags, zero at rest (the
    // re-decode clears the flags it reads); zeroed when the block is allocated
    Carver ws;
    ws.take(size_t(p.n_contigs) + 16);
    const size_t b_fix = ws.off;
    const size_t b_vec = n * L * 8 + 8, b_one = n * 8 + 8;
    const size_t o_state = ws.take(b_vec), o_E = ws.take(b_vec), o_alpha = ws.take(b_vec), o_smax = ws.take(b_one), o_scale = ws.take(b_one),
                 o_back = ws.take(n * L + 8);
    size_t o_chM = 0, o_chV = 0, o_chB = 0, o_chEx = 0, o_chZ = 0, o_chMap = 0, o_chY = 0;
    if (chunked) {
        const size_t b_chv = nch * L * 8 + 8;
        o_chM = ws.take(nch * L * L * 8 + 8);
        o_chV = ws.take(b_chv);
        o_chB = ws.take(b_chv);
        o_chEx = ws.take(b_chv);
        o_chZ = ws.take(nch * 8 + 8);
        ws.take(nch * 8 + 8);  // (chZ is two such arrays)
        o_chMap = ws.take(nch * L + 8);
        o_chY = ws.take(nch * L + 8);
    }
    {
        std::lock_guard<std::mutex> lock(p.ws_mutex);
        const size_t cap0 = p.gen_ws.capacity();
        int rc = p.gen_ws.reserve(ws.off, "hipMalloc general-L workspace");
        if (rc) return rc;
        if (p.gen_ws.capacity() != cap0 && (rc = check_hip(hipMemsetAsync(p.gen_ws.get(), 0, b_fix, stream), "memset contig flags"))) return rc;
    }
    char *w = p.gen_ws.get();
    a = GenArgs{};
    a.vit_stats = reinterpret_cast<uint32_t *>(w);
    a.fix_flag = reinterpret_cast<uint8_t *>(w + 16);
    // the margin's bound on a partial sum of state scores is nnz * max|v| * max|w| with values.  Nothing else
    // on this route reads the state weights' size: gen_small_ok / all_small_ok (gl_windowed_small, gl_windowed_mfma, gl_all_small)
    // and rows_rescale_period below guard the spread of the TRANSITIONS over un-normalised steps, and every sum-product kernel
    // takes the states as exp(state - max state) in (0, 1], whatever the states' size
    a.v_wmax = csr.attr_value ? p.tables_model->wmax_abs * csr.vmax_abs : p.tables_model->wmax_abs;
    a.v_tmax = p.tables_model->tmax_abs;
    a.gene_ptr = csr.gene_ptr;
    a.attr_id = csr.attr_id;
    a.wtab = p.tables_model->wtab.get();
    a.exp_trans = p.tables_model->exp_trans.get();
    a.trans = p.tables_model->trans.get();
    a.contig_ptr = p.d_contig_ptr;
    a.L = m.L;
    a.A = m.A;
    a.n_genes = p.n_genes;
    a.n_contigs = p.n_contigs;
    a.rows_rescale_period = 4.0 * p.tables_model->tmax_abs < 600.0 ? 4 : 1;
    a.state = reinterpret_cast<double *>(w + o_state);
    a.E = reinterpret_cast<double *>(w + o_E);
    a.alpha = reinterpret_cast<double *>(w + o_alpha);
    a.smax = reinterpret_cast<double *>(w + o_smax);
    a.scale = reinterpret_cast<double *>(w + o_scale);
    a.back = reinterpret_cast<uint8_t *>(w + o_back);
    if (chunked && nch) {
        const Plan::GenTab &tab = p.gen_tab[chunk_min_len >= 0 ? 1 : 0];
        a.ch_g0 = tab.d.at<const int32_t>(0);
        a.ch_contig = tab.d.at<const int32_t>(tab.off1);
        a.cc_ptr = tab.d.at<const int32_t>(tab.off2);
        a.n_chunks = int32_t(nch);
        a.chM = reinterpret_cast<double *>(w + o_chM);
        a.chV = reinterpret_cast<double *>(w + o_chV);
        a.chB = reinterpret_cast<double *>(w + o_chB);
        a.chEx = reinterpret_cast<int32_t *>(w + o_chEx);
        a.chZ = reinterpret_cast<double *>(w + o_chZ);
        a.chMap = reinterpret_cast<uint8_t *>(w + o_chMap);
        a.chY = reinterpret_cast<int8_t *>(w + o_chY);
    }
    return GECCO_CRF_OK;
}

// Whole-contig recursions of 9 to 32 labels: which contigs go to the wave-per-contig kernel (crf_general.hip).  The waves take as
// long as the longest contig they are given (t_step us per gene: a lone wave issues an instruction every four cycles); the
// chunked kernels pay L x the arithmetic for every gene they are given (t_gene us), a walk over the chunks of their longest
// contig (t_walk us per gene) and a chain of launches (t_launches us).  So the batch is SPLIT: the k longest contigs -- the
// tail of a metagenome's length distribution -- go through the chunked kernels on the plan's side stream, NEXT TO the waves
// of the others, with k minimising max(t_waves(longest of the others), t_chunked(the k longest)).
// Returns -1: chunked kernels for everything; 0: waves for everything; > 0: waves for contigs up to this length.
// `env`: wave | chunked | split (k = 1) forces; `automatic`: whether the model's label count is one the choice is made for;
// `cache`: the choice for this layout (INT32_MIN: not made yet).
int32_t choose_wave_split(const Plan &p, const char *env, bool automatic, double t_step, double t_gene, double t_walk, double t_launches,
                          int32_t &cache) {
    const int forced = !env ? -1 : env[0] == 'w' ? 1 : env[0] == 'c' ? 0 : env[0] == 's' ? 2 : -1;
    if (forced == 1) return 0;
    if (forced == 0 || (forced < 0 && !automatic)) return -1;
    if (forced < 0 && cache != INT32_MIN) return cache;  // (the sort below is the host's only loop over the contigs)
    int32_t wave_tmax = -1;
    std::vector<int32_t> len(size_t(p.n_contigs));
    for (int32_t c = 0; c < p.n_contigs; ++c) len[size_t(c)] = p.contig_ptr[c + 1] - p.contig_ptr[c];
    std::sort(len.begin(), len.end(), std::greater<int32_t>());
    const double all_chunked = double(p.n_genes) * t_gene + double(len[0]) * t_walk + t_launches;
    double best = all_chunked;
    int64_t tail = 0;
    for (int32_t k = 0; k < p.n_contigs; ++k) {  // the k longest contigs chunked NEXT TO the waves of the others
        const double t_tail = k ? double(tail) * t_gene + double(len[0]) * t_walk + t_launches : 0.0;
        const double t = std::max(double(len[size_t(k)]) * t_step, t_tail);
        if (t < best || (forced == 2 && k == 1)) {
            best = t;
            wave_tmax = k ? len[size_t(k)] : 0;  // (contigs as long as the k-th longest stay with the waves)
            if (forced == 2 && k == 1) break;
        }
        tail += len[size_t(k)];
        if (double(tail) * t_gene + t_launches > best) break;  // (cannot get better from here)
    }
    if (wave_tmax > 0 && len[0] <= wave_tmax) wave_tmax = 0;  // (nothing is longer: no tail)
    if (forced < 0) cache = wave_tmax;
    return wave_tmax;
}

// The any-L sum-product kernels take the transitions as exp(trans), uploaded as std::exp gives them (get_device_tables).  A
// scaled step forms s <= L e^max with L <= 32, finite while max < 709.78 - ln 32 = 706.3; with max < -745 every exp(trans) is
// 0 and the pass would return zeros, with max > 709.78 infinities and NaN, either with a clean status.  700 is the figure
// the 2-label route keeps its own products inside (`room`, slot_prod_max_cnt).  A finite model outside it is refused, not
// shifted: no in-range model changes a bit.  Viterbi reads the raw weights and is not refused.  DESIGN.md §4.9f.
constexpr double kRunsMaxTrans = 150.0;  // plan_run_run_posteriors
int check_exp_trans_range(const Plan &p) {
    const double mx = p.tables_model->tmax;
    if (!(mx > 700.0) && !(mx < -700.0)) return GECCO_CRF_OK;
    char msg[320];
    std::snprintf(msg, sizeof(msg),
                  "the largest transition weight (%g) is outside [-700, 700], the range in which the any-label sum-product kernels "
                  "can take exp(transition weight): subtracting a constant from every transition weight leaves the model unchanged",
                  mx);
    set_error(msg);
    return GECCO_CRF_EINVAL;
}

// fork the chunked kernels of a batch's long tail onto the plan's side stream (behind what `stream` holds so far); join_tail
// makes `stream` wait for them
int fork_tail(Plan &p, hipStream_t stream) {
    int rc;
    if (!p.side_stream.get()) {
        if ((rc = p.side_stream.create())) return rc;
        if ((rc = check_hip(hipEventCreateWithFlags(&p.ev_fork, hipEventDisableTiming), "hipEventCreate"))) return rc;
        if ((rc = check_hip(hipEventCreateWithFlags(&p.ev_join, hipEventDisableTiming), "hipEventCreate"))) return rc;
    }
    if ((rc = check_hip(hipEventRecord(p.ev_fork, stream), "hipEventRecord"))) return rc;
    return check_hip(hipStreamWaitEvent(p.side_stream.get(), p.ev_fork, 0), "hipStreamWaitEvent");
}
int join_tail(Plan &p, hipStream_t stream) {
    int rc = check_hip(hipEventRecord(p.ev_join, p.side_stream.get()), "hipEventRecord");
    if (rc) return rc;
    return check_hip(hipStreamWaitEvent(stream, p.ev_join, 0), "hipStreamWaitEvent");
}

// One whole-contig recursion of the any-L kernels -- forward-backward marginals or Viterbi -- as run_gen_whole sees it: the
// switch that forces its arrangement, when the choice is automatic, the cost model of choose_wave_split, its launchers.
struct GenRecursion {
    // GECCO_CRF_GENERAL_*=wave|chunked|split for 9 <= L <= 32 (tests, A/B).  A reader, not the variable's name: the getenv call
    // keeps its literal, which is how tests/test_native_cpu.py finds every switch the library reads
    const char *(*forced)();
    int auto_above;                     // the choice is made for models of more labels than this
    double (*t_step)(int L), (*t_gene)(int L), (*t_walk)(int L), (*t_launches)(int L);  // us; choose_wave_split
    int32_t Plan::*cache;               // the split chosen for the plan's layout
    hipError_t (*chunked)(const GenArgs &, hipStream_t), (*wave)(const GenArgs &, hipStream_t);
    void (*clear)(GenArgs &);           // the workspace fields the recursion does not use
    const char *what;
    bool sum_product;                   // the kernels read exp(trans): check_exp_trans_range
};
// 17 to 32 labels: the split of the Viterbi recursion for the forward-backward recursion (gl_marginals_wave; a step of it is
// ~0.5 us; the chunked kernels -- transfer matrices on the matrix cores -- run at 2.6 / 2.2 ns per gene at L = 32 / 24).
// Measured on 1 000 contigs / 0.22 M genes, longest 1 519 (all chunked -> all waves -> split): L = 32 0.60 -> 0.77 -> 0.44 ms.
// GECCO_CRF_GENERAL_MARGINALS=wave|chunked|split forces for 9 <= L <= 32 (tests, A/B).
const GenRecursion kGenMarginals = {
    [] { return (const char *)std::getenv("GECCO_CRF_GENERAL_MARGINALS"); },
    16,
    [](int L) { return L > 16 ? 0.5 : 0.38; },
    [](int L) { return L >= 28 ? 2.6e-3 : L > 16 ? 2.2e-3 : 1.0e-3; },
    [](int) { return 0.1; },
    [](int) { return 200.0; },
    &Plan::gen_wave_tmax_f,
    launch_gen_marginals,
    launch_gen_marginals_wave,
    [](GenArgs &g) { g.state = nullptr; },
    "marginals launch",
    true,
};
// 13 to 32 labels: a wave per contig (gl_viterbi_wave) where the batch has its parallelism in its contigs.  The wave
// kernel takes as long as the longest contig it is given (~0.36 / 0.25 us per gene above / up to 16 labels: a lone wave
// issues an instruction every four cycles); the chunked kernels pay L x the arithmetic for every gene they are given
// plus a chain of six launches and the walk over their longest contig's chunks.  So the batch is SPLIT: the k longest
// contigs -- the tail of a metagenome's length distribution -- go through the chunked kernels on the plan's side
// stream, NEXT TO the waves of the others, with k minimising  max(t_wave(longest of the others), t_chunked(the k longest)).
// Measured on 1 000 contigs / 0.22 M genes, longest 1 519, next 762 (all chunked -> all waves -> split):
// L = 32 1.42 -> 0.55 -> 0.32 ms, L = 24 0.96 -> 0.55 -> 0.32 ms, L = 16 0.28 -> 0.37 -> 0.22 ms.
// GECCO_CRF_GENERAL_VITERBI=wave|chunked forces either for 9 <= L <= 32 (tests, A/B); =split forces the split at k = 1.
const GenRecursion kGenViterbi = {
    [] { return (const char *)std::getenv("GECCO_CRF_GENERAL_VITERBI"); },
    12,
    [](int L) { return L > 16 ? 0.36 : 0.25; },
    [](int L) { return L >= 28 ? 6.3e-3 : L > 16 ? 4.3e-3 : 1.3e-3; },
    [](int L) { return L > 16 ? 0.07 : 0.04; },
    [](int L) { return L > 16 ? 150.0 : 80.0; },
    &Plan::gen_wave_tmax,
    launch_gen_viterbi,
    launch_gen_viterbi_wave,
    [](GenArgs &g) { g.E = g.smax = nullptr; },
    "viterbi launch",
    false,
};

// The whole-contig recursion `r` of an any-L plan: state scores, then the chunked kernels, a wave per contig, or both side by
// side (choose_wave_split).  Outputs the recursion does not write are null.  `used`: the argument block of the launches, for a
// kernel that reads the workspace behind them.
int run_gen_whole(Plan &p, const GenRecursion &r, const DeviceCsr &csr, double *d_marg, double *d_lognorm,
                  int8_t *d_y, double *d_score, hipStream_t stream, GenArgs *used = nullptr) {
    const int L = p.model->L;
    if (r.sum_product)
        if (const int bad = check_exp_trans_range(p)) return bad;
    int32_t wave_tmax = -1;  // -1: no wave kernel; 0: every contig; > 0: contigs up to this length
    if (L > 8 && p.n_contigs > 0)
        wave_tmax = choose_wave_split(p, r.forced(), L > r.auto_above, r.t_step(L), r.t_gene(L), r.t_walk(L), r.t_launches(L), p.*r.cache);
    const bool wave = wave_tmax >= 0, tail_chunked = wave_tmax > 0;
    GenArgs g;
    int rc = fill_gen_args(p, csr, g, !wave || tail_chunked, stream, tail_chunked ? wave_tmax : -1);
    if (rc) return rc;
    g.marg = d_marg;
    g.lognorm = d_lognorm;
    g.y = d_y;
    g.score = d_score;
    r.clear(g);
    g.wave_tmax = tail_chunked ? wave_tmax : 0;
    if (used) *used = g;
    if ((rc = check_hip(launch_gen_state(g, stream, csr.attr_value, csr.allowed), "state score launch"))) return rc;
    if (!wave) return check_hip(r.chunked(g, stream), r.what);
    if (!tail_chunked || g.n_chunks <= 0) return check_hip(r.wave(g, stream), r.what);
    // the long tail (chunked kernels: short in work, long in dependent launches) NEXT TO the waves of the other contigs:
    // forked onto the plan's side stream behind the state scores, joined before anything later on the caller's stream.
    // The two write disjoint genes, contigs and back-pointer regions: a contig's back-pointers, in either kernel's layout, stay
    // inside its own T * L bytes (gl_viterbi_wave: quads of rows 1 .. T - 1 from the first dword boundary).  (A chunkless
    // contig's path score is the waves'.)
    if ((rc = fork_tail(p, stream))) return rc;
    if ((rc = check_hip(r.chunked(g, p.side_stream.get()), r.what))) return rc;
    if ((rc = check_hip(r.wave(g, stream), r.what))) return rc;
    return join_tail(p, stream);
}

int fill_seq_args(Plan &p, SeqArgs &a, hipStream_t stream);

// What every run entry point checks before it launches, in the order the checks have always had: a device behind the plan and
// the label (entry points without one pass 0), and a batch that brings values, and masks, exactly when the layout was built for
// them ...
int check_plan(const Plan &p, const DeviceCsr &csr, int32_t label) {
    if (p.device < 0) {
        set_error("host-only plan: no HIP device bound (there is no CPU fallback)");
        return GECCO_CRF_ENODEV;
    }
    if (label < 0 || label >= p.model->L) {
        set_error("label out of range");
        return GECCO_CRF_EINVAL;
    }
    if ((csr.attr_value != nullptr) != p.valued) {
        set_error(p.valued ? "the plan was built for attribute values: the batch has none"
                           : "attribute values given to a plan that was not built for them");
        return GECCO_CRF_EINVAL;
    }
    if ((csr.allowed != nullptr) != p.masked) {
        set_error(p.masked ? "the plan was built for allowed-label masks: the batch has none"
                           : "allowed-label masks given to a plan that was not built for them");
        return GECCO_CRF_EINVAL;
    }
    return GECCO_CRF_OK;
}
// ... for the whole-contig entry points the workspace (what pipelined decode calls left there is lost) ...
int begin_whole_contig(Plan &p, const DeviceCsr &csr, int32_t label, SeqArgs &a, hipStream_t stream) {
    p.pipe.pending = false;
    const int rc = check_plan(p, csr, label);
    return rc ? rc : fill_seq_args(p, a, stream);
}
// ... then a batch with nothing to do, which ends the call without an error, and the caller's buffers.  True: the call ends
// here, with `rc`.
bool ends_here(bool empty, bool null_buffer, int &rc) {
    rc = GECCO_CRF_OK;
    if (empty) return true;
    if (!null_buffer) return false;
    set_error("null device buffer");
    rc = GECCO_CRF_EINVAL;
    return true;
}

// The whole-contig marginals of a plan laid out with `lattice`, for a query (`what`) that then reads what the pass left in the
// workspace: the recursion as plan_run_marginals_full runs it -- the same launches, the same bits -- with one difference under
// keep_state: gl_state also leaves the raw state scores.  `g`: the argument block of the launches, for the query's kernel (a
// batch's chunked tail has been joined to `stream` by then).
const GenRecursion kGenMarginalsKeepState = [] {
    GenRecursion r = kGenMarginals;
    r.clear = [](GenArgs &) {};
    return r;
}();
int run_lattice(Plan &p, const DeviceCsr &csr, const char *what, bool keep_state, double *d_marg, double *d_lognorm, hipStream_t stream,
                GenArgs &g) {
    SeqArgs a;
    const int rc = begin_whole_contig(p, csr, 0, a, stream);
    if (rc) return rc;
    if (!p.lattice || !p.general) {
        set_error(std::string("the plan was not built for ") + what);
        return GECCO_CRF_EINVAL;
    }
    return run_gen_whole(p, keep_state ? kGenMarginalsKeepState : kGenMarginals, csr, d_marg, d_lognorm, nullptr, nullptr, stream, &g);
}

// The state scores alone, for a query on a plan laid out with `lattice` whose kernels read nothing else: gl_state with the raw
// scores kept and neither E nor smax.  No exp(trans) is read, and no transition range applies.  `g`: the launch's argument block.
int run_state_only(Plan &p, const DeviceCsr &csr, const char *what, hipStream_t stream, GenArgs &g) {
    SeqArgs a;
    int rc = begin_whole_contig(p, csr, 0, a, stream);
    if (rc) return rc;
    if (!p.lattice || !p.general) {
        set_error(std::string("the plan was not built for ") + what);
        return GECCO_CRF_EINVAL;
    }
    if ((rc = fill_gen_args(p, csr, g, false, stream))) return rc;
    g.E = g.smax = nullptr;
    return check_hip(launch_gen_state(g, stream, csr.attr_value, csr.allowed), "state score launch");
}

// where the window kernels accumulate (atomic maxima: `zero` first, numpy.zeros of crf/__init__.py:251) or store p; the genes of
// skipped contigs keep "no prediction"
int start_p_out(const Plan &p, double *d_p_out, bool zero, hipStream_t stream) {
    int rc;
    if (zero && (rc = check_hip(hipMemsetAsync(d_p_out, 0, size_t(p.n_genes) * 8, stream), "memset p"))) return rc;
    if (p.skipped.empty()) return GECCO_CRF_OK;
    return check_hip(launch_fill_nan(d_p_out, p.d_skipped, int(p.skipped.size()), stream), "fill_nan launch");
}

// The windowed marginals of an any-L plan (crf_general_windowed.hip), one label (label >= 0: d_p [n]) or every label
// (label = -1: d_p [n][L], d_p_any [n] or null, `background`): the state scores, the outputs' preparation and the tier, which
// the caller has chosen -- `small`: the tile kernels on `d_tiles`, else one group of lanes per window start.
int run_windowed_general(Plan &p, const DeviceCsr &csr, int32_t label, int32_t background, double *d_p, double *d_p_any,
                         bool small, const int4 *d_tiles, int32_t ntiles, hipStream_t stream) {
    if (!small && p.W > kGenMaxW) {
        set_error("window too long for the any-L kernel (alpha of a whole window is LDS-resident: W <= 48)");
        return GECCO_CRF_EUNSUPPORTED;
    }
    GenArgs g;
    int rc = check_exp_trans_range(p);
    if (rc || (rc = fill_gen_args(p, csr, g))) return rc;
    g.state = nullptr;  // marginals only need exp(state - max)
    if ((rc = check_hip(launch_gen_state(g, stream, csr.attr_value, csr.allowed), "state score launch"))) return rc;
    GenWinArgs a{};
    a.E = g.E;
    a.exp_trans = g.exp_trans;
    a.trans = g.trans;
    a.c_slot = p.d_c_slot;
    a.c_gene = p.d_c_gene;
    a.c_n = p.d_c_n;
    a.start_bits = p.d_start_bits;
    a.p_out = d_p;
    a.p_any = d_p_any;
    a.L = g.L;
    a.K = p.K;
    a.S = p.S;
    a.W = p.W;
    a.label = label;
    a.background = background;
    // the lane-group tier takes maxima in place: +0.0 everywhere first (numpy.zeros of crf/__init__.py:251); the tile kernels
    // store every gene of slot space once.  Then "no prediction" for the genes of skipped contigs, which lie outside slot
    // space and are written by neither
    const int cols = label < 0 ? a.L : 1;
    if (!small) {
        if ((rc = check_hip(hipMemsetAsync(d_p, 0, size_t(p.n_genes) * size_t(cols) * 8, stream), "memset p"))) return rc;
        if (d_p_any && (rc = check_hip(hipMemsetAsync(d_p_any, 0, size_t(p.n_genes) * 8, stream), "memset p"))) return rc;
    }
    if (!p.skipped.empty() &&
        (rc = check_hip(launch_all_fill_nan(d_p, d_p_any, cols, p.d_skipped, int(p.skipped.size()), stream), "fill_nan launch")))
        return rc;
    if (small) return check_hip(launch_gen_windowed_small(a, p.model->trans.data(), d_tiles, ntiles, stream), "windowed launch");
    return check_hip(launch_gen_windowed(a, stream), "windowed launch");
}
}  // namespace

// the launch also carries the Viterbi workgroups of `seq`, which belongs to the PREVIOUS batch (crf_decode_pipelined: nothing
// is exchanged inside the launch)
struct PipelinedLaunch {
    const SeqArgs *seq;
    bool *took = nullptr;  // set when the one launch was made (otherwise the caller launches the Viterbi side itself)
};
static int run_windowed_impl(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                             double2 *d_state_out, double *d_dstate_out, hipStream_t stream, const PipelinedLaunch *piped = nullptr);

int plan_run_windowed(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                      hipStream_t stream) {
    return run_windowed_impl(p, csr, label, d_p_out, nullptr, nullptr, stream);
}

static int run_windowed_impl(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                             double2 *d_state_out, double *d_dstate_out, hipStream_t stream, const PipelinedLaunch *piped) {
    int rc = check_plan(p, csr, label);
    if (rc || ends_here(p.n_genes == 0, !csr.gene_ptr || !d_p_out, rc)) return rc;
    if ((rc = use_device(p.device))) return rc;
    const Model &m = *p.model;
    // (the tier of the single-label entry was chosen when the plan was built: gen_small, on the plan's own tile table)
    if (p.general) return run_windowed_general(p, csr, label, -1, d_p_out, nullptr, p.gen_small, p.d_tile_desc, p.ntiles, stream);
    WinArgs a{};
    a.gene_ptr = csr.gene_ptr;
    a.attr_id = csr.attr_id;
    a.wtab = p.tables_model->wtab.get();
    a.wtab2 = p.tables_model->wtab2[label].get();
    a.exp_trans = p.tables_model->exp_trans.get();
    a.rtab = p.tables_model->rtab[label].get();
    a.ptab = p.tables_model->ptab[label].get();
    a.c_slot = p.d_c_slot;
    a.c_gene = p.d_c_gene;
    a.c_n = p.d_c_n;
    a.tile_desc = p.d_tile_desc;
    a.start_bits = p.d_start_bits;
    a.p_out = d_p_out;
    a.state_out = d_state_out;
    a.dstate_out = d_dstate_out;
    a.K = p.K;
    a.S = p.S;
    a.ntiles = p.ntiles;
    a.W = p.W;
    a.step = p.step;
    a.L = m.L;
    a.label = label;
    a.n_genes = p.n_genes;
    a.A = m.A;
    a.tiles_per_wg = p.tiles_per_wg;
    a.all_regular = p.all_regular ? 1 : 0;
    a.rescale_mask = p.rescale_mask;
    {
        const DeviceTables::WinConsts &c = p.tables_model->win[label];  // (model constants, computed once per device: get_device_tables)
        a.mu01 = c.mu01;
        a.rho = c.rho;
        a.kappa_over_mu01 = c.kappa_over_mu01;
        a.inv_kappa = c.inv_kappa;
        a.g00 = c.g00;
        a.g01 = c.g01;
        a.g10 = c.g10;
        a.g11 = c.g11;
        std::memcpy(a.expc, c.expc, sizeof(a.expc));
        a.ratio_zmax = c.ratio_zmax;
        a.prod_cnt = c.prod_cnt;
    }
    a.csr_begin = int32_t(p.csr_begin);  // (row pointers are 32-bit)
    a.csr_end = int32_t(p.csr_end);
    a.generic = (p.fast_ok || p.reference_now) ? 0 : 1;
    if (p.reference_now || !p.fast_ok) {  // (the reference-bits and the generic kernel work in a scratch block)
        const size_t bytes = p.reference_now ? reference_scratch_bytes(p.n_genes) : size_t(p.S) * size_t(p.W) * 16 + 16;
        std::lock_guard<std::mutex> lock(p.ws_mutex);
        if ((rc = p.win_scratch.reserve(bytes, p.reference_now ? "hipMalloc reference scratch" : "hipMalloc window scratch")))
            return rc;
    }
    // (the register-resident and the reference-bits kernel store every gene of slot space once, by the tile that owns its slot:
    // nothing to zero)
    if ((rc = start_p_out(p, d_p_out, a.generic, stream))) return rc;
    if (p.reference_now) {
        double et[4];
        for (int i = 0; i < 4; ++i) et[i] = std::exp(m.trans[size_t(i)]);  // (the host's libm, as the reference's CRFsuite calls it)
        return check_hip(launch_windowed_reference(a, p.tables_model->wtab2[1].get(), et, p.win_scratch.get(), stream), "reference-bits launch");
    }
    if (a.generic) a.scratch = p.win_scratch.get();
    if (piped && !a.generic && decode_pipelined_ok(a, *piped->seq)) {
        *piped->took = true;
        return check_hip(launch_decode_pipelined(a, *piped->seq, stream), "pipelined decode launch");
    }
    return check_hip(launch_windowed(a, stream), "windowed launch");
}

// ---- every label's windowed marginals (crf_general_windowed.hip) --------------------------------
namespace {
// the lane-per-window tier serves this plan (GECCO_CRF_GENERAL_GROUPS=1: the lane-group tier, as for the single-label kernels)
bool all_small_tier(const Plan &p) {
    return all_small_ok(p.model->L, p.W, p.model->trans.data()) && !std::getenv("GECCO_CRF_GENERAL_GROUPS");
}
// The tile table of the lane-per-window tier: the plan's own when it was laid out for the same geometry (gen_small), else
// built here by plan_build's own routine (fill_tile_desc).
int all_tiles(Plan &p, const int4 **d_tiles, int32_t *ntiles) {
    const int32_t tile_out = gen_small_tile_out(p.W);
    if (p.gen_small && p.tile_out == tile_out) {
        *d_tiles = p.d_tile_desc;
        *ntiles = p.ntiles;
        return GECCO_CRF_OK;
    }
    std::lock_guard<std::mutex> lock(p.ws_mutex);
    if (p.all_ntiles < 0) {
        const int32_t nt = p.S > 0 ? (p.S + tile_out - 1) / tile_out : 0;
        // (the plan's own irr_prefix is scratch that the whole-contig tables reuse: derived again from the layout)
        std::vector<int32_t> irr(size_t(p.K) + 1, 0);
        for (int32_t k = 0; k < p.K; ++k) {
            const bool padded = p.c_slot[k + 1] - p.c_slot[k] != p.c_n[k];
            const bool gap_after = k + 1 < p.K && p.c_gene[k + 1] != p.c_gene[k] + p.c_n[k];
            irr[size_t(k) + 1] = irr[size_t(k)] + ((padded || gap_after) ? 1 : 0);
        }
        std::vector<int4> td(size_t(nt) + 1);
        fill_tile_desc(p, irr, tile_out, nt, td.data());
        int rc = p.all_tiles.reserve(td.size() * sizeof(int4), "hipMalloc tile table");
        if (rc) return rc;
        if ((rc = check_hip(hipMemcpy(p.all_tiles.get(), td.data(), td.size() * sizeof(int4), hipMemcpyHostToDevice), "upload tile table")))
            return rc;
        p.all_ntiles = nt;
    }
    *d_tiles = p.all_tiles.get();
    *ntiles = p.all_ntiles;
    return GECCO_CRF_OK;
}
}  // namespace

const char *plan_all_kernel_name(const Plan &p) { return p.model && all_small_tier(p) ? "gl_all_small" : "gl_all_groups"; }

int plan_run_windowed_all(Plan &p, const DeviceCsr &csr, int32_t background, double *d_p_all,
                          double *d_p_any, hipStream_t stream) {
    int rc = check_plan(p, csr, 0);
    if (rc) return rc;
    if (background < -1 || background >= p.model->L) {
        set_error("background label out of range");
        return GECCO_CRF_EINVAL;
    }
    if ((background < 0) != (d_p_any == nullptr)) {
        set_error(background < 0 ? "p_any needs a background label" : "null p_any buffer with a background label");
        return GECCO_CRF_EINVAL;
    }
    if (ends_here(p.n_genes == 0, !csr.gene_ptr || !d_p_all, rc)) return rc;
    if ((rc = use_device(p.device))) return rc;
    // (the tier of this entry is chosen per call, on a tile table of that geometry: all_tiles)
    const bool small = all_small_tier(p);
    const int4 *d_tiles = nullptr;
    int32_t ntiles = 0;
    if (small && (rc = all_tiles(p, &d_tiles, &ntiles))) return rc;
    return run_windowed_general(p, csr, -1, background, d_p_all, d_p_any, small, d_tiles, ntiles, stream);
}

// ---- whole-contig scans (rows F, V) ------------------------------------------------------
namespace {
struct SeqLayout {
    size_t lanes, blocks, bytes;
    size_t off_state, off_alpha, off_tmp, off_vlane, off_vblock, off_vmaps, off_vlanemap, off_vblockmap, off_flane,
        off_fblock, off_flanesuf, off_fblocksuf, off_cand, off_stats;
};
SeqLayout seq_layout(size_t n) {
    SeqLayout l{};
    l.lanes = (n + kSeqGenesPerLane - 1) / kSeqGenesPerLane;
    l.blocks = (l.lanes + 255) / 256;
    const size_t lanes_pad = l.blocks * 256;
    Carver ws;
    l.off_stats = ws.take(64);  // (first: the decoder's counters keep their place when the batch size changes)
    l.off_state = ws.take((n + kSeqGenesPerLane) * 16);
    l.off_alpha = ws.take(n * 16);
    l.off_tmp = ws.take(n * 16);
    l.off_vlane = ws.take(lanes_pad * sizeof(VE));
    l.off_vblock = ws.take(l.blocks * sizeof(VE));
    l.off_vmaps = ws.take(lanes_pad * 4);
    l.off_vlanemap = ws.take(lanes_pad * 4);
    l.off_vblockmap = ws.take(l.blocks * 4);
    l.off_flane = ws.take(lanes_pad * sizeof(FE));
    l.off_fblock = ws.take(l.blocks * sizeof(FE));
    l.off_flanesuf = ws.take(lanes_pad * sizeof(FE));
    l.off_fblocksuf = ws.take(l.blocks * sizeof(FE));
    l.off_cand = ws.take((lanes_pad + 4 * l.blocks + 16) * sizeof(SeqArgs::VdCand));
    l.bytes = ws.off + 256;
    return l;
}
// (the per-contig "decode again" flags of the long-contig Viterbi path live behind the scan workspace)

}  // namespace

int plan_ensure_seq(Plan &p, hipStream_t stream, bool sync) {
    std::lock_guard<std::mutex> lock(p.ws_mutex);
    if (p.seq_ready) return GECCO_CRF_OK;
    if (p.device < 0) {
        set_error("host-only plan: no HIP device bound (there is no CPU fallback)");
        return GECCO_CRF_ENODEV;
    }
    int rc = use_device(p.device);
    if (rc) return rc;
    const size_t n = size_t(p.n_genes);
    // short contigs (none longer than a scan block): whole contigs are packed into workgroups of <= 2048 genes
    p.seq_short = true;
    for (int32_t c = 0; c < p.n_contigs && p.seq_short; ++c)
        if (p.contig_ptr[c + 1] - p.contig_ptr[c] > kSeqBlockGenes) p.seq_short = false;
    std::vector<int32_t> &cblk = p.irr_prefix;  // scratch
    cblk.clear();
    if (p.seq_short && n) {
        int32_t start = 0;
        cblk.push_back(0);
        for (int32_t c = 0; c < p.n_contigs; ++c) {
            const int32_t g1 = p.contig_ptr[c + 1];
            if (g1 - start > kSeqBlockGenes) {  // contig c does not fit any more: close the workgroup before it
                start = p.contig_ptr[c];
                cblk.push_back(start);
            }
        }
        cblk.push_back(int32_t(n));
    }
    p.n_cblocks = cblk.empty() ? 0 : int32_t(cblk.size()) - 1;
    // non-empty contigs: their indices, and how many of them precede every workgroup (log Z is written per contig)
    std::vector<int32_t> ne, rank;
    p.n_empty_contigs = 0;
    if (p.n_cblocks) {
        size_t b = 0;
        rank.assign(size_t(p.n_cblocks), 0);
        for (int32_t c = 0; c < p.n_contigs; ++c) {
            if (p.contig_ptr[c + 1] == p.contig_ptr[c]) {
                ++p.n_empty_contigs;
                continue;
            }
            while (b < size_t(p.n_cblocks) && cblk[b] <= p.contig_ptr[c]) {  // workgroups starting at or before this contig
                if (cblk[b] == p.contig_ptr[c]) rank[b] = int32_t(ne.size());
                ++b;
            }
            ne.push_back(c);
        }
    }
    const size_t n_lane_bits = size_t(p.n_cblocks) * 256;  // short contigs: per lane of every workgroup, which of its 8 genes start / end a contig
    // uploaded: the workgroup tables, the lane bits and a copy of the contig table; NOT uploaded: the byte per gene that
    // says "first / last gene of its contig" -- a launch behind the copy derives it from the contig table on the device
    // (two thirds of the block's bytes: 0.5 of 0.77 MB per half-million-gene chunk of the batch driver)
    const size_t n_flat_bits = ((n + kSeqBlockGenes - 1) / kSeqBlockGenes) * 256;
    Carver blk;
    const size_t o_blk = blk.take((cblk.size() + 1) * 4), o_rank = blk.take((rank.size() + 1) * 4), o_ne = blk.take((ne.size() + 1) * 4),
                 o_lb = blk.take(n_lane_bits * 2 + 2), o_fb = blk.take(n_flat_bits * 2 + 2), o_cp = blk.take((size_t(p.n_contigs) + 1) * 4),
                 bytes = blk.off, o_flags = blk.take(n + 16), all_bytes = blk.off;
    if ((rc = p.seq.reserve(all_bytes, "contig flags"))) return rc;
    if (p.n_contigs) std::memcpy(p.seq.h + o_cp, p.contig_ptr.data(), (size_t(p.n_contigs) + 1) * 4);
    if (n_flat_bits) {
        // the flat layout (long contigs): lane l of the batch owns genes 8 l .. 8 l + 7
        uint16_t *fb = reinterpret_cast<uint16_t *>(p.seq.h + o_fb);
        std::memset(fb, 0, n_flat_bits * 2);
        for (int32_t c = 0; c < p.n_contigs; ++c) {
            const int32_t g0 = p.contig_ptr[c], g1 = p.contig_ptr[c + 1];
            if (g1 <= g0) continue;
            fb[size_t(g0 / kSeqGenesPerLane)] |= uint16_t(1u << (g0 % kSeqGenesPerLane));
            fb[size_t((g1 - 1) / kSeqGenesPerLane)] |= uint16_t(0x100u << ((g1 - 1) % kSeqGenesPerLane));
        }
        size_t l = n;  // positions past the last gene: one-gene contigs
        for (; l < n_flat_bits * kSeqGenesPerLane && l % kSeqGenesPerLane; ++l)
            fb[l / kSeqGenesPerLane] |= uint16_t(0x101u << (l % kSeqGenesPerLane));
        for (; l < n_flat_bits * kSeqGenesPerLane; l += kSeqGenesPerLane) fb[l / kSeqGenesPerLane] = 0xffff;
    }
    if (n_lane_bits) {
        // bit k of the low byte: gene k of the lane is the first of its contig; of the high byte: the last
        uint16_t *lb = reinterpret_cast<uint16_t *>(p.seq.h + o_lb);
        std::memset(lb, 0, n_lane_bits * 2);
        size_t b = 0;
        for (int32_t c = 0; c < p.n_contigs; ++c) {
            const int32_t g0 = p.contig_ptr[c], g1 = p.contig_ptr[c + 1];
            if (g1 <= g0) continue;
            while (cblk[b + 1] <= g0) ++b;  // the workgroup that holds the (whole) contig
            const int32_t l0 = g0 - cblk[b], l1 = g1 - 1 - cblk[b];
            lb[b * 256 + size_t(l0 / kSeqGenesPerLane)] |= uint16_t(1u << (l0 % kSeqGenesPerLane));
            lb[b * 256 + size_t(l1 / kSeqGenesPerLane)] |= uint16_t(0x100u << (l1 % kSeqGenesPerLane));
        }
        // positions past a workgroup's last gene: one-gene contigs (the kernels give them a score difference that decides
        // nothing), so that the hot loops run over all 8 positions of every lane without testing
        for (int32_t blk = 0; blk < p.n_cblocks; ++blk) {
            const int32_t nb = cblk[size_t(blk) + 1] - cblk[size_t(blk)];
            int32_t l = nb;
            for (; l < kSeqBlockGenes && l % kSeqGenesPerLane; ++l)
                lb[size_t(blk) * 256 + size_t(l / kSeqGenesPerLane)] |= uint16_t(0x101u << (l % kSeqGenesPerLane));
            for (; l < kSeqBlockGenes; l += kSeqGenesPerLane) lb[size_t(blk) * 256 + size_t(l / kSeqGenesPerLane)] = 0xffff;
        }
    }
    if (!cblk.empty()) std::memcpy(p.seq.h + o_blk, cblk.data(), cblk.size() * 4);
    if (!rank.empty()) std::memcpy(p.seq.h + o_rank, rank.data(), rank.size() * 4);
    if (!ne.empty()) std::memcpy(p.seq.h + o_ne, ne.data(), ne.size() * 4);
    char *base = p.seq.d;
    if (p.seq_in_host_memory) {
        // a small batch: the decoder reads its tables (a few hundred bytes) from the pinned block itself and the host writes the
        // flag bytes -- nothing is copied, nothing is launched in front of the decoder
        uint8_t *fl = reinterpret_cast<uint8_t *>(p.seq.h + o_flags);
        std::memset(fl, 0, n + 16);
        for (int32_t c = 0; c < p.n_contigs; ++c) {
            const int32_t g0 = p.contig_ptr[c], g1 = p.contig_ptr[c + 1];
            if (g1 <= g0) continue;
            fl[g0] |= 1u;
            fl[g1 - 1] |= 2u;
        }
        void *dv = nullptr;
        if ((rc = check_hip(hipHostGetDevicePointer(&dv, p.seq.h, 0), "hipHostGetDevicePointer"))) return rc;
        base = static_cast<char *>(dv);
    }
    p.d_seq_flags = reinterpret_cast<uint8_t *>(base + o_flags);
    p.d_seq_cblk = reinterpret_cast<int32_t *>(base + o_blk);
    p.d_seq_cblk_rank = reinterpret_cast<int32_t *>(base + o_rank);
    p.d_seq_ne_contig = reinterpret_cast<int32_t *>(base + o_ne);
    p.d_seq_lane_bits = reinterpret_cast<const uint16_t *>(base + o_lb);
    p.d_seq_flat_bits = reinterpret_cast<const uint16_t *>(base + o_fb);
    if (p.seq_in_host_memory) {
        p.seq_ready = true;
        return GECCO_CRF_OK;
    }
    // launches that read the tables must be ordered behind this copy: `sync` (any stream may follow), or the
    // caller keeps to `stream` (the batch driver)
    if (p.tables_by_kernel && !sync) {  // (batch driver: fetched by a launch, the copy engine keeps to the chunks' arrays)
        void *dv = nullptr;
        if ((rc = check_hip(hipHostGetDevicePointer(&dv, p.seq.h, 0), "hipHostGetDevicePointer"))) return rc;
        if ((rc = check_hip(launch_copy_block(dv, p.seq.d, bytes, stream), "contig tables launch"))) return rc;
    } else if ((rc = check_hip(hipMemcpyAsync(p.seq.d, p.seq.h, bytes, hipMemcpyHostToDevice, stream), "upload contig flags"))) {
        return rc;
    }
    if ((rc = check_hip(launch_contig_flags(reinterpret_cast<const int32_t *>(p.seq.d + o_cp), p.n_contigs, p.n_genes, p.d_seq_flags, stream),
                        "contig flags launch")))
        return rc;
    if (sync && (rc = check_hip(hipStreamSynchronize(stream), "upload contig flags"))) return rc;
    p.seq_ready = true;
    return GECCO_CRF_OK;
}

namespace {
int ensure_seq(Plan &p, hipStream_t stream) {
    int rc = plan_ensure_seq(p, stream, !p.async_tables);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(p.ws_mutex);
    const SeqLayout l = seq_layout(size_t(p.n_genes));
    const bool fresh = !p.seq_ws.get() || l.bytes + align256(size_t(p.n_contigs) + 24) > p.seq_ws.capacity();
    rc = p.seq_ws.reserve(l.bytes + align256(size_t(p.n_contigs) + 24), "hipMalloc scan workspace");
    // (the decoder's counters accumulate over launches: they start from zero in a new block)
    if (!rc && fresh) rc = check_hip(hipMemsetAsync(p.seq_ws.get() + l.off_stats, 0, 64, stream), "memset decoder counters");
    // the exactness test's bound, candidate counter and contig flags (behind the layout): zero before the first decode on
    // this layout; every decode leaves them zero again (vd_exact_fix)
    const size_t sig = l.bytes * 1000003u + size_t(p.n_contigs) + 1;
    if (!rc && (fresh || sig != p.vbound_sig)) {
        rc = check_hip(hipMemsetAsync(p.seq_ws.get() + l.bytes, 0, 16 + size_t(p.n_contigs), stream), "memset contig flags");
        if (!rc) p.vbound_sig = sig;
    }
    return rc;
}

// (callers have checked that the plan has a device: check_plan, can_hand_over)
int fill_seq_args(Plan &p, SeqArgs &a, hipStream_t stream) {
    int rc = use_device(p.device);
    if (rc) return rc;
    if (p.general) return GECCO_CRF_OK;  // the any-L path has its own workspace
    if ((rc = ensure_seq(p, stream))) return rc;
    const Model &m = *p.model;
    const SeqLayout l = seq_layout(size_t(p.n_genes));
    char *w = p.seq_ws.get();
    a = SeqArgs{};
    a.state = reinterpret_cast<double2 *>(w + l.off_state);
    a.alpha = reinterpret_cast<double2 *>(w + l.off_alpha);
    a.contigTmp = reinterpret_cast<double2 *>(w + l.off_tmp);
    a.vLane = reinterpret_cast<VE *>(w + l.off_vlane);
    a.vBlock = reinterpret_cast<VE *>(w + l.off_vblock);
    a.vMaps = reinterpret_cast<uint32_t *>(w + l.off_vmaps);
    a.vLaneMap = reinterpret_cast<uint32_t *>(w + l.off_vlanemap);
    a.vBlockMap = reinterpret_cast<uint32_t *>(w + l.off_vblockmap);
    a.fLane = reinterpret_cast<FE *>(w + l.off_flane);
    a.fBlock = reinterpret_cast<FE *>(w + l.off_fblock);
    a.fLaneSuf = reinterpret_cast<FE *>(w + l.off_flanesuf);
    a.fBlockSuf = reinterpret_cast<FE *>(w + l.off_fblocksuf);
    a.vCand = reinterpret_cast<SeqArgs::VdCand *>(w + l.off_cand);
    a.vd_stats = reinterpret_cast<uint32_t *>(w + l.off_stats);
    a.vBound = reinterpret_cast<unsigned long long *>(w + l.bytes);  // (16 bytes in front of the flags: one memset clears both)
    a.fix_flag = reinterpret_cast<uint8_t *>(w + l.bytes + 16);
    a.v_wmax2 = 2.0 * p.tables_model->wmax_abs;
    a.v_tmax = p.tables_model->tmax_abs;
    a.v_nmax = p.n_max;
    a.flags = p.d_seq_flags;
    a.lane_bits = p.d_seq_lane_bits;
    a.flat_bits = p.d_seq_flat_bits;
    a.cblk = p.d_seq_cblk;
    a.n_cblocks = p.n_cblocks;
    a.cblk_rank = p.d_seq_cblk_rank;
    a.ne_contig = p.d_seq_ne_contig;
    a.contig_ptr = p.d_contig_ptr;
    a.short_contigs = p.seq_short ? 1 : 0;
    a.n_contigs = p.n_contigs;
    a.n_genes = p.n_genes;
    const DeviceTables::SeqConsts &q = p.tables_model->seq;  // (model constants, computed once per device)
    a.mx = q.mx;
    a.t00 = m.trans[0];
    a.t01 = m.trans[1];
    a.t10 = m.trans[2];
    a.t11 = m.trans[3];
    a.m00 = q.m00;
    a.m01 = q.m01;
    a.m10 = q.m10;
    a.m11 = q.m11;
    a.dstate = reinterpret_cast<const double *>(a.state);  // same workspace, one of the two forms per call
    a.raw_fold = q.raw_fold;
    a.v_lo = q.v_lo;
    a.v_hi = q.v_hi;
    a.v_k = q.v_k;
    a.v_exact = q.v_exact;
    std::memcpy(a.expc, q.expc, sizeof(a.expc));
    return GECCO_CRF_OK;
}
}  // namespace

// Labels of a 2-label model whose transitions satisfy lo <= hi come from the difference form (8 B/gene, 24-B scan
// elements), the one decoder with a margin test and CRFsuite's own recursion behind it.  A path score, where
// one is requested, comes from the max-plus scan (v_fold -> v_replay -> v_scores) run in front of it without its labels.
// GECCO_CRF_VITERBI=matrix forces the matrix form for the labels too.
static bool viterbi_delta_ok(const SeqArgs &a) {
    const char *env = std::getenv("GECCO_CRF_VITERBI");
    if (env && env[0] == 'm') return false;
    return a.v_lo <= a.v_hi && std::isfinite(a.v_lo) && std::isfinite(a.v_hi);
}

namespace {
// what a caller of run_viterbi_l2 has already left in the plan's workspace
enum class SeqLeft { nothing, state, dstate };  // ... the state scores (a.state), their differences (a.dstate)

inline void bind_seq_io(const Plan &p, SeqArgs &a, const DeviceCsr &csr, int8_t *d_y, double *d_score) {
    a.y = d_y;
    a.score = d_score;
    a.csr_gene_ptr = csr.gene_ptr;
    a.csr_attr_id = csr.attr_id;
    a.csr_wtab01 = p.tables_model->wtab2[1].get();
    a.csr_n_attrs = p.model->A;
}

// buffer `parity` of the two in which pipelined decode calls hand score differences over (the workspace's state block)
inline double *parity_buffer(const Plan &p, const SeqArgs &a, int parity) {
    return const_cast<double *>(reinterpret_cast<const double *>(a.state)) + size_t(parity) * (size_t(p.n_genes) + 8);
}

// handing the score differences over needs the register-resident 2-label kernel and every gene in slot space
inline bool can_hand_over(const Plan &p) { return !p.general && p.fast_ok && p.skipped.empty() && p.device >= 0; }

// which of the two the window tiles should leave for run_viterbi_l2 (`delta`: viterbi_delta_ok)
inline SeqLeft tiles_hand_over(bool delta, const double *d_score) { return delta && !d_score ? SeqLeft::dstate : SeqLeft::state; }

// Whole-contig Viterbi of a 2-label plan; `a` filled and bound (bind_seq_io), `delta`: viterbi_delta_ok(a), read once per call
// by the caller (score differences left behind imply it).  A path score, or labels under anti-sticky
// transitions, come from the max-plus scan over the state scores -- with `y` nulled when the difference form gives the labels
// (viterbi_delta_ok) --; the labels from the decoder over the score differences.
int run_viterbi_l2(Plan &p, const SeqArgs &a, SeqLeft left, bool delta, hipStream_t stream) {
    int rc;
    if (left != SeqLeft::dstate) {
        if (!delta || a.score) {
            if (left == SeqLeft::nothing &&
                (rc = check_hip(launch_seq_state(a.csr_gene_ptr, a.csr_attr_id, a.csr_wtab01, a.csr_n_attrs, p.n_genes,
                                                 const_cast<double2 *>(a.state), stream), "state score launch")))
                return rc;
            SeqArgs m = a;
            if (delta) m.y = nullptr;  // the scores only: the labels are the difference form's, below
            if ((rc = check_hip(launch_seq_viterbi(m, p.d_contig_ptr, stream), "viterbi launch")) || !delta) return rc;
        }
        if ((rc = check_hip(launch_seq_state_delta(a.csr_gene_ptr, a.csr_attr_id, a.csr_wtab01, a.csr_n_attrs, p.n_genes,
                                                   const_cast<double *>(a.dstate), stream), "state score launch")))
            return rc;
    }
    return check_hip(launch_seq_viterbi_delta(a, stream), "viterbi launch");
}
}  // namespace

int plan_run_marginals_full(Plan &p, const DeviceCsr &csr, double *d_marg,
                            double *d_lognorm, hipStream_t stream) {
    SeqArgs a;
    int rc = begin_whole_contig(p, csr, 0, a, stream);
    if (rc || ends_here(p.n_contigs == 0, p.n_genes > 0 && (!csr.gene_ptr || !d_marg), rc)) return rc;
    if (p.general) return run_gen_whole(p, kGenMarginals, csr, d_marg, d_lognorm, nullptr, nullptr, stream);
    a.marg = d_marg;
    a.lognorm = d_lognorm;
    // 8-byte inputs, alpha in registers: one fused kernel when workgroups own whole contigs, the workgroups' products
    // + the fused kernel (look-back / look-ahead over them) for contigs of any length
    a.smax = reinterpret_cast<const double *>(a.alpha);
    // short contigs: log Z is written by the kernel at every contig's last gene; contigs without genes get their 0 here
    if (p.seq_short && d_lognorm && p.n_empty_contigs &&
        (rc = check_hip(hipMemsetAsync(d_lognorm, 0, size_t(p.n_contigs) * 8, stream), "memset lognorm")))
        return rc;
    return check_hip(launch_seq_marginals_short(a, csr.gene_ptr, csr.attr_id, p.tables_model->wtab2[1].get(), p.model->A, p.d_contig_ptr,
                                                stream), "marginals launch");
}

int plan_run_span_probabilities(Plan &p, const DeviceCsr &csr, const SpanQuery *d_spans, int32_t n_spans, double *d_logp,
                                double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (n_spans < 0) {
        set_error("negative number of spans");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0, (p.n_genes > 0 && (!csr.gene_ptr || !d_marg)) || (n_spans > 0 && (!d_spans || !d_logp)), rc))
        return rc;
    GenArgs g;  // (with the raw state scores, which the span kernel shifts by its own maxima)
    if ((rc = run_lattice(p, csr, "region posteriors", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_spans(g, d_spans, n_spans, d_logp, stream), "span launch");
}

int plan_run_span_conditionals(Plan &p, const DeviceCsr &csr, const ConditionalArgs &q, double *d_logp, double *d_marg,
                               double *d_lognorm, hipStream_t stream) {
    if (q.n_spans < 0 || q.reach < 0 || q.n_rows < 0 || q.n_fwd < 0 || q.n_occ < 0) {
        set_error("a negative number of spans or rows, or a negative reach");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0,
                  (p.n_genes > 0 && (!csr.gene_ptr || !d_marg)) ||
                      (q.n_spans > 0 && (!q.spans || !d_logp || !q.row_ptr || !q.fwd_ptr || !q.fwd || !q.walk || !q.cond || !q.item ||
                                         (q.occ_ptr && !q.attr))), rc))
        return rc;
    GenArgs g;  // (with the raw state scores, which the span kernel and the walks shift by their own maxima)
    if ((rc = run_lattice(p, csr, "conditional marginals", true, d_marg, d_lognorm, stream, g))) return rc;
    if ((rc = check_hip(launch_gen_spans(g, q.spans, q.n_spans, d_logp, stream), "span launch"))) return rc;
    ConditionalArgs a = q;
    a.logp = d_logp;
    a.attr_value = csr.attr_value;
    return check_hip(launch_gen_conditionals(g, a, stream), "conditionals launch");
}

int plan_run_run_posteriors(Plan &p, const DeviceCsr &csr, const RunPosteriorArgs &q, double *d_marg, double *d_lognorm,
                            hipStream_t stream) {
    if (q.n_anchors < 0 || q.n_runs < 0 || q.reach < 0 || q.reach > kMaxRunReach) {
        set_error("a negative number of anchors or runs, or reach outside 0 .. 65536");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg ||
                      (q.n_anchors > 0 && (!q.anchors || !q.log_anchor || !q.log_start || !q.log_start_beyond || !q.log_end ||
                                           !q.log_end_beyond)) ||
                      (q.n_runs > 0 && (!q.runs || !q.log_run)), rc))
        return rc;
    // The walks read the pass's stored alpha, and E marg / alpha, of single labels.  The pass forms (alpha . M) E before it
    // normalises, and a wave pass keeps alpha with the step's factor: with max|trans| = s a label B nats behind at a gene is
    // flushed to an exact 0 there once s + B passes 708, and the runs that need it came back -infinity instead of about -B
    // (at s = 600: every label more than 108 behind).  150 is rows_rescale_period's figure; under it a label is kept down
    // to 550 nats behind.  A transition whose exp is 0 does not exist for the pass and does not count.  DESIGN.md 4.9f.
    if ((rc = check_exp_trans_range(p))) return rc;
    if (p.tables_model->tmax_abs_live > kRunsMaxTrans) {
        char msg[320];
        std::snprintf(msg, sizeof(msg),
                      "run posteriors: the largest |transition weight| (%g) is above %g, the range in which the stored forward vectors "
                      "keep the labels the walks read: subtracting a constant from every transition weight leaves the model unchanged",
                      p.tables_model->tmax_abs_live, kRunsMaxTrans);
        set_error(msg);
        return GECCO_CRF_EINVAL;
    }
    GenArgs g;  // (with the raw state scores, which the walks shift by their own maxima)
    if ((rc = run_lattice(p, csr, "run posteriors", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_runs(g, q, stream), "run-posterior launch");
}

int plan_run_sample_paths(Plan &p, const DeviceCsr &csr, int32_t n_samples, uint64_t seed, const RunQuery *d_queries, int32_t n_runs,
                          int8_t *d_y, int32_t *d_runs, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (n_samples < 1 || n_samples > kMaxSamples || n_runs < 0) {
        set_error("n_samples outside 1 .. 2^20, or a negative number of runs");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0, !csr.gene_ptr || !d_marg || !d_y || (n_runs > 0 && (!d_queries || !d_runs)), rc))
        return rc;
    GenArgs g;
    if ((rc = run_lattice(p, csr, "sampled paths", false, d_marg, d_lognorm, stream, g))) return rc;
    if ((rc = check_hip(launch_gen_sample_paths(g, n_samples, seed, d_y, stream), "sample launch"))) return rc;
    return check_hip(launch_gen_sample_runs(g, d_y, d_queries, n_runs, n_samples, d_runs, stream), "run launch");
}

int plan_run_viterbi_kbest(Plan &p, const DeviceCsr &csr, int32_t k, uint16_t *d_back, uint16_t *d_fin, int8_t *d_y, double *d_score,
                           int32_t *d_n_paths, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (k < 1 || k > kMaxKBest) {
        set_error("k outside 1 .. 32");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg || !d_back || !d_fin || !d_y || !d_score || !d_n_paths, rc))
        return rc;
    GenArgs g;  // (the pass gives log Z; the list recursion reads the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "the K best paths", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_kbest(g, k, d_back, d_fin, d_y, d_score, d_n_paths, stream), "k-best launch");
}

// the label set of a run-counter query: not empty, and no label at or above the model's
static bool set_mask_ok(const Plan &p, uint32_t set_mask) {
    const int32_t L = p.model ? p.model->L : 32;  // (a plan that was never built is check_plan's to refuse)
    if (set_mask != 0 && (L >= 32 || !(set_mask >> L))) return true;
    set_error("set_mask is empty, or holds a label at or above num_labels");
    return false;
}

int plan_run_viterbi_min_run(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t min_run, uint8_t *d_back, int8_t *d_y,
                             double *d_score, double *d_lognorm_min_run, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (min_run < 1 || min_run > kMaxMinRun) {
        set_error("min_run outside 1 .. 32");
        return GECCO_CRF_EINVAL;
    }
    if (!set_mask_ok(p, set_mask)) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0, !csr.gene_ptr || !d_marg || !d_back || !d_y || !d_score, rc)) return rc;
    GenArgs g;  // (the pass gives log Z; the run-counter recursion reads the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "minimum-run decoding", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_min_run(g, set_mask, min_run, d_back, d_y, d_score, d_lognorm_min_run, stream), "min-run launch");
}

int plan_run_marginals_min_run(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t min_run, double *d_fwd, double *d_marg_min_run,
                               double *d_inside, double *d_lognorm_min_run, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (min_run < 1 || min_run > kMaxMinRun) {
        set_error("min_run outside 1 .. 32");
        return GECCO_CRF_EINVAL;
    }
    if (!set_mask_ok(p, set_mask)) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg || !d_fwd || !d_lognorm_min_run || (!d_marg_min_run && !d_inside), rc))
        return rc;
    GenArgs g;  // (the pass gives log Z; the run-counter recursions read the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "minimum-run marginals", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_min_run_marginals(g, set_mask, min_run, d_fwd, d_marg_min_run, d_inside, d_lognorm_min_run, stream),
                     "min-run marginals launch");
}

// the length model of a run-length query: M inside the kernels' range, no NaN and no +infinity among its scores
static bool run_length_scores_ok(const RunLengthScores &sc) {
    bool ok = sc.M >= 1 && sc.M <= kMaxRunLength && sc.tau < INFINITY;
    for (int32_t d = 0; ok && d < sc.M; ++d) ok = sc.g[d] < INFINITY;
    if (!ok) set_error("max_length outside 1 .. 32, or a length score that is NaN or +infinity");
    return ok;
}

int plan_run_viterbi_run_length(Plan &p, const DeviceCsr &csr, uint32_t set_mask, const RunLengthScores &sc, uint8_t *d_back, int8_t *d_y,
                                double *d_score, double *d_lognorm_run_length, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (!run_length_scores_ok(sc) || !set_mask_ok(p, set_mask)) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0, !csr.gene_ptr || !d_marg || !d_back || !d_y || !d_score, rc)) return rc;
    GenArgs g;  // (the pass gives log Z; the run-counter recursion reads the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "run-length decoding", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_run_length(g, set_mask, sc, d_back, d_y, d_score, d_lognorm_run_length, stream), "run-length launch");
}

int plan_run_marginals_run_length(Plan &p, const DeviceCsr &csr, uint32_t set_mask, const RunLengthScores &sc, double *d_fwd,
                                  double *d_marg_run_length, double *d_inside, double *d_counts, double *d_lognorm_run_length,
                                  double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (!run_length_scores_ok(sc) || !set_mask_ok(p, set_mask)) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg || !d_fwd || !d_lognorm_run_length || (!d_marg_run_length && !d_inside && !d_counts), rc))
        return rc;
    GenArgs g;  // (the pass gives log Z; the run-counter recursions read the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "run-length marginals", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_run_length_marginals(g, set_mask, sc, d_fwd, d_marg_run_length, d_inside, d_counts,
                                                     d_lognorm_run_length, stream),
                     "run-length marginals launch");
}

int plan_run_run_counts(Plan &p, const DeviceCsr &csr, uint32_t set_mask, int32_t max_runs, uint8_t *d_back, double *d_log_mass,
                        double *d_score, int8_t *d_y, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (max_runs < 1 || max_runs > kMaxRunCounts) {
        set_error("max_runs outside 1 .. 32");
        return GECCO_CRF_EINVAL;
    }
    if (!set_mask_ok(p, set_mask)) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg || (!d_log_mass && !d_score) || (d_score && (!d_back || !d_y)), rc))
        return rc;
    GenArgs g;  // (the pass gives log Z; the run-counter recursion reads the raw state scores and nothing else)
    if ((rc = run_lattice(p, csr, "run counts", true, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_run_counts(g, set_mask, max_runs, d_back, d_log_mass, d_score, d_y, stream), "run-count launch");
}

int plan_run_max_marginals(Plan &p, const DeviceCsr &csr, const MaxMargArgs &q, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (q.n_sets < 0 || q.n_sets > kMaxMargSets || q.n_spans < 0 || (q.n_sets == 0 && (q.inside || q.outside))) {
        set_error("the number of label sets is outside 0 .. 32 (1 .. 32 with inside or outside), or a negative number of spans");
        return GECCO_CRF_EINVAL;
    }
    for (int32_t s = 0; s < q.n_sets; ++s)
        if (!set_mask_ok(p, q.set_mask[s])) return GECCO_CRF_EINVAL;
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !q.fwd || !q.bwd || !q.best || (d_lognorm && !d_marg) ||
                      (q.n_spans > 0 && (!q.spans || (!q.span_best && !q.span_broken))), rc))
        return rc;
    GenArgs g;
    if (d_lognorm) {  // (the pass gives log Z; the max walks read the raw state scores and nothing else)
        if ((rc = run_lattice(p, csr, "max-marginals", true, d_marg, d_lognorm, stream, g))) return rc;
    } else if ((rc = run_state_only(p, csr, "max-marginals", stream, g))) {  // (no exp(trans) is read: no transition range applies)
        return rc;
    }
    return check_hip(launch_gen_max_marginals(g, q, stream), "max-marginal launch");
}

int plan_run_ring(Plan &p, const DeviceCsr &csr, const RingArgs &q, hipStream_t stream) {
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !q.lognorm_ring || (q.marg && !q.fwd) || (!q.y != !q.score) || (q.y && (!q.back || !q.start)), rc))
        return rc;
    GenArgs g;
    if ((rc = run_state_only(p, csr, "circular contigs", stream, g))) return rc;
    return check_hip(launch_gen_ring(g, q, stream), "ring launch");
}

int plan_run_edge_posteriors(Plan &p, const DeviceCsr &csr, const EdgeQuery &q, double *d_marg, double *d_lognorm, hipStream_t stream) {
    if (q.n_sets < 0 || q.n_sets > kMaxEdgeSets || (q.n_sets == 0 && (q.enter || q.leave))) {
        set_error("the number of label sets is outside 1 .. 32 (0 without enter and leave)");
        return GECCO_CRF_EINVAL;
    }
    int rc;
    if (ends_here(p.n_contigs == 0 || p.n_genes == 0,
                  !csr.gene_ptr || !d_marg || !q.runs || !q.run_ptr || (q.transitions && !q.npart) || (q.entropy && !q.hpart), rc))
        return rc;
    // (the run table is the caller's: it has to be the one of this layout's contigs, or a run would leave its contig)
    int64_t n_runs = 0;
    for (int32_t c = 0; c < p.n_contigs; ++c) n_runs += edge_run_count(p.contig_ptr[c + 1] - p.contig_ptr[c]);
    if (q.n_runs != n_runs) {
        set_error("edge posteriors: the run table does not belong to the plan's contigs");
        return GECCO_CRF_EINVAL;
    }
    GenArgs g;  // (the raw state scores are not needed: the edges read E, alpha and the marginals)
    if ((rc = run_lattice(p, csr, "edge posteriors", false, d_marg, d_lognorm, stream, g))) return rc;
    return check_hip(launch_gen_edges(g, q, stream), "edge launch");
}

int plan_run_viterbi(Plan &p, const DeviceCsr &csr, int8_t *d_y, double *d_score,
                     hipStream_t stream) {
    SeqArgs a;
    int rc = begin_whole_contig(p, csr, 0, a, stream);
    if (rc || ends_here(p.n_contigs == 0, p.n_genes > 0 && (!csr.gene_ptr || !d_y), rc)) return rc;
    if (p.general) return run_gen_whole(p, kGenViterbi, csr, nullptr, nullptr, d_y, d_score, stream);
    bind_seq_io(p, a, csr, d_y, d_score);
    return run_viterbi_l2(p, a, SeqLeft::nothing, viterbi_delta_ok(a), stream);
}

int plan_run_decode(Plan &p, const DeviceCsr &csr, int32_t label, double *d_p_out,
                    int8_t *d_y, double *d_score, hipStream_t stream) {
    if (!can_hand_over(p)) {
        // (pipe.pending is only ever set on a plan that can hand over, so it is clear here; plan_run_viterbi clears it all the same)
        int rc = plan_run_windowed(p, csr, label, d_p_out, stream);
        if (rc) return rc;
        return plan_run_viterbi(p, csr, d_y, d_score, stream);
    }
    SeqArgs a;
    int rc = begin_whole_contig(p, csr, label, a, stream);
    if (rc || ends_here(p.n_contigs == 0 || p.n_genes == 0, !csr.gene_ptr || !d_p_out || !d_y, rc)) return rc;
    bind_seq_io(p, a, csr, d_y, d_score);
    // the window tiles leave the state scores, or their differences, where the Viterbi side reads them
    const bool delta = viterbi_delta_ok(a);
    SeqLeft left = tiles_hand_over(delta, d_score);
    // (the ratio-form tiles add up factors and score differences, not the two scores: those come from run_viterbi_l2's own launch)
    if (left == SeqLeft::state && p.fast_ok && !p.reference_now && windowed_ratio_form(p.W, p.rescale_mask)) left = SeqLeft::nothing;
    if ((rc = run_windowed_impl(p, csr, label, d_p_out, left == SeqLeft::state ? const_cast<double2 *>(a.state) : nullptr,
                                left == SeqLeft::dstate ? const_cast<double *>(a.dstate) : nullptr, stream)))
        return rc;
    return run_viterbi_l2(p, a, left, delta, stream);
}

int plan_run_decode_pipelined(Plan *cur, const DeviceCsr &csr, int32_t label, double *d_p_out,
                              Plan *prev, int8_t *d_prev_y, hipStream_t stream) {
    int rc;
    // ---- the previous batch: labels from the score differences its window tiles left behind (or from its CSR arrays)
    SeqArgs pa{};
    bool prev_delta = false;
    const bool prev_work = prev && prev->n_genes > 0 && prev->n_contigs > 0;
    if (prev_work) {
        if (!d_prev_y) {
            set_error("null device buffer");
            return GECCO_CRF_EINVAL;
        }
        if (prev->pipe.pending && !prev->general) {
            if ((rc = fill_seq_args(*prev, pa, stream))) return rc;
            pa.dstate = parity_buffer(*prev, pa, prev->pipe.parity);
            bind_seq_io(*prev, pa, prev->pipe.csr, d_prev_y, nullptr);
            prev_delta = true;
        }
    }
    if (prev_work && !prev_delta) {
        // no score differences left behind (any-L model, contigs outside slot space, or another call used the workspace since):
        // the state scores are summed again from the CSR arrays -- BEFORE this batch's tiles write into the workspace
        const Plan::Pipe keep = prev->pipe;
        if (!keep.csr.gene_ptr) {
            set_error("pipelined decode: the previous plan has not been scored by a pipelined call (or has been rebuilt since)");
            return GECCO_CRF_EINVAL;
        }
        if ((rc = plan_run_viterbi(*prev, keep.csr, d_prev_y, nullptr, stream))) return rc;
        prev->pipe = keep;
    }
    // ---- this batch: marginals, and score differences for the next call where the kernels hand them over
    bool took = false;
    if (cur) {
        Plan &p = *cur;
        const int parity = p.pipe.parity ^ 1;  // (cur == prev: the Viterbi side reads the other buffer)
        double *d_dstate = nullptr;
        if (can_hand_over(p) && p.n_genes > 0) {
            SeqArgs ca;
            if (prev_delta && prev == cur) {
                ca = pa;  // (a plan that follows itself: the block has just been filled for the Viterbi side)
            } else if ((rc = fill_seq_args(p, ca, stream))) {
                return rc;
            }
            if (viterbi_delta_ok(ca)) d_dstate = parity_buffer(p, ca, parity);
        }
        const bool delta = d_dstate != nullptr;
        PipelinedLaunch fl{};
        fl.seq = &pa;
        fl.took = &took;
        if ((rc = run_windowed_impl(p, csr, label, d_p_out, nullptr, d_dstate, stream,
                                    (delta && prev_delta) ? &fl : nullptr)))
            return rc;
        p.pipe.pending = delta;
        p.pipe.parity = delta ? parity : p.pipe.parity;
        p.pipe.csr = csr;
    }
    if (prev_delta && !took && (rc = run_viterbi_l2(*prev, pa, SeqLeft::dstate, true, stream))) return rc;
    if (prev && prev != cur) prev->pipe.pending = false;
    return GECCO_CRF_OK;
}

int plan_viterbi_stats(Plan &p, int64_t out[4], bool reset) {
    for (int i = 0; i < 4; ++i) out[i] = 0;
    std::lock_guard<std::mutex> lock(p.ws_mutex);
    // (any-L plans: the counters of the chunked Viterbi, in front of the general-L workspace)
    char *base = p.general ? p.gen_ws.get() : p.seq_ws.get();
    if (p.device < 0 || !base) return GECCO_CRF_OK;  // nothing has been decoded yet
    int rc = use_device(p.device);
    if (rc) return rc;
    if ((rc = check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize"))) return rc;
    uint32_t v[4] = {0, 0, 0, 0};
    char *at = p.general ? base : base + seq_layout(size_t(p.n_genes)).off_stats;
    if ((rc = check_hip(hipMemcpy(v, at, sizeof(v), hipMemcpyDeviceToHost), "read decoder counters"))) return rc;
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    if (reset) rc = check_hip(hipMemset(at, 0, sizeof(v)), "clear decoder counters");
    return rc;
}

int plan_run_segment(Plan &p, const double *d_p, const uint8_t *d_annotated, const SegParams &params, int32_t *d_seg,
                     int32_t max_seg, int32_t *d_seg_off, int32_t *d_total, hipStream_t stream, double *d_gather, int32_t gather_cap) {
    if (!d_total || max_seg < 0 || (max_seg > 0 && !d_seg)) {
        set_error("plan_run_segment: bad arguments");
        return GECCO_CRF_EINVAL;
    }
    if (params.criterion != 0 && params.criterion != 1) {
        set_error("Unknown cluster filtering criterion");  // refine.py:165
        return GECCO_CRF_EINVAL;
    }
    if (params.criterion == 1 && p.n_genes > 0 && (!params.bio_ptr || !params.bio_id)) {
        set_error("the antismash criterion needs the genes' marker domains");
        return GECCO_CRF_EINVAL;
    }
    // the contig flags of the whole-contig tables when the plan has them; otherwise the segmenter derives them from the
    // contig table on the device (a memset and a launch over the contigs instead of an upload of a byte per gene)
    int rc = GECCO_CRF_OK;
    if (p.n_genes > 0 && (!d_p || !d_annotated)) {
        set_error("null device buffer");
        return GECCO_CRF_EINVAL;
    }
    {
        std::lock_guard<std::mutex> lock(p.ws_mutex);
        if ((rc = p.seg_ws.reserve(segment_workspace_bytes(p.n_genes, p.n_contigs), "hipMalloc segment workspace")))
            return rc;
    }
    return check_hip(launch_segment(d_p, d_annotated, p.seq_ready ? p.d_seq_flags : nullptr, p.d_contig_ptr, p.n_genes, p.n_contigs, params, d_seg, max_seg,
                                    d_seg_off, d_total, p.seg_ws.get(), stream, d_gather, gather_cap),
                     "segment launch");
}

}  // namespace gecco
