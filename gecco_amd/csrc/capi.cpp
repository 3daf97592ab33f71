// extern "C" surface declared in include/gecco_crf.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_exact_exp.hpp"
#include "crf_fisher.hpp"
#include "crf_forest.hpp"
#include "crf_model.hpp"
#include "crf_overlap.hpp"
#include "crf_plan.hpp"
#include "crf_session.hpp"
#include "crf_tables.hpp"
#include "crf_train.hpp"

using namespace gecco;

struct gecco_crf_model {
    Model m;
};
struct gecco_crf_plan {
    Plan p;
};
struct gecco_crf_packed {
    Packed p;
};
struct gecco_crf_cluster_rows {
    ClusterRows r;
};
struct gecco_crf_session {
    Session *s = nullptr;
    ~gecco_crf_session() { session_destroy(s); }
};

// No C++ exception may cross the C boundary (ctypes would std::terminate the interpreter).
#define GECCO_GUARD_BEGIN try {
#define GECCO_GUARD_END                                                     \
    }                                                                       \
    catch (const std::bad_alloc &) {                                        \
        set_error("out of host memory");                                    \
        return GECCO_CRF_ENOMEM;                                            \
    }                                                                       \
    catch (const std::exception &e) {                                       \
        set_error(std::string("internal error: ") + e.what());              \
        return GECCO_CRF_EHIP;                                              \
    }                                                                       \
    catch (...) {                                                           \
        set_error("internal error");                                        \
        return GECCO_CRF_EHIP;                                              \
    }

#define GECCO_API extern "C" __attribute__((visibility("default")))

namespace {
int fail(const char *msg) {
    set_error(msg);
    return GECCO_CRF_EINVAL;
}
int fail(const std::string &msg) { return fail(msg.c_str()); }

// The argument checks that the one-shots share, each message written once.  They come before any device work, so that an
// argument error surfaces even on a box without a GPU.
int check_window(int32_t window, int32_t step) {
    if (window <= 0) return fail("Window size must be strictly positive");
    if (step <= 0 || step > window) return fail("Window step must be strictly positive and under `window_size`");
    return GECCO_CRF_OK;
}
int check_label(const gecco_crf_model *m, int32_t label) {
    return label < 0 || label >= m->m.L ? fail("label out of range") : GECCO_CRF_OK;
}
int check_background(const gecco_crf_model *m, int32_t background, const double *p_any) {
    if (background < -1 || background >= m->m.L) return fail("background label out of range");
    if ((background < 0) != (p_any == nullptr))
        return fail(background < 0 ? "p_any needs a background label" : "null p_any buffer with a background label");
    return GECCO_CRF_OK;
}
}  // namespace

GECCO_API const char *gecco_crf_last_error(void) { return last_error(); }
GECCO_API int gecco_crf_version(void) { return 340; }

GECCO_API int gecco_crf_model_load(const uint8_t *lcrf, size_t n_bytes, gecco_crf_model **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_model> h(new gecco_crf_model());
    int rc = parse_lcrf(lcrf, n_bytes, h->m);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_model_from_tables(const double *state, const double *trans, int32_t num_attrs,
                                          int32_t num_labels, gecco_crf_model **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_model> h(new gecco_crf_model());
    int rc = model_from_tables(state, trans, num_attrs, num_labels, h->m);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}

GECCO_API void gecco_crf_model_free(gecco_crf_model *m) { delete m; }
GECCO_API int32_t gecco_crf_model_num_labels(const gecco_crf_model *m) { return m ? m->m.L : 0; }
GECCO_API int32_t gecco_crf_model_num_attrs(const gecco_crf_model *m) { return m ? m->m.A : 0; }
GECCO_API int32_t gecco_crf_model_num_features(const gecco_crf_model *m) { return m ? m->m.n_features : 0; }
GECCO_API const char *gecco_crf_model_label_name(const gecco_crf_model *m, int32_t id) {
    return (m && id >= 0 && id < m->m.L) ? m->m.labels[id].c_str() : nullptr;
}
GECCO_API const char *gecco_crf_model_attr_name(const gecco_crf_model *m, int32_t id) {
    return (m && id >= 0 && id < m->m.A) ? m->m.attrs[id].c_str() : nullptr;
}
GECCO_API int32_t gecco_crf_model_label_id(const gecco_crf_model *m, const char *name) {
    if (!m || !name) return -1;
    auto it = m->m.label_index.find(name);
    return it == m->m.label_index.end() ? -1 : it->second;
}
GECCO_API int32_t gecco_crf_model_attr_id(const gecco_crf_model *m, const char *name) {
    if (!m || !name) return -1;
    auto it = m->m.attr_index.find(name);
    return it == m->m.attr_index.end() ? -1 : it->second;
}
GECCO_API int gecco_crf_model_map_attrs(const gecco_crf_model *m, const char *const *names, int32_t n, int32_t *ids) {
    if (!m || (n > 0 && (!names || !ids))) return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    std::string key;
    for (int32_t i = 0; i < n; ++i) {
        if (!names[i]) {
            ids[i] = -1;
            continue;
        }
        key.assign(names[i]);
        auto it = m->m.attr_index.find(key);
        ids[i] = it == m->m.attr_index.end() ? -1 : it->second;
    }
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_model_state_weights(const gecco_crf_model *m, double *w, uint8_t *present) {
    if (!m) return GECCO_CRF_EINVAL;
    if (w) std::memcpy(w, m->m.state.data(), m->m.state.size() * sizeof(double));
    if (present) std::memcpy(present, m->m.state_mask.data(), m->m.state_mask.size());
    return GECCO_CRF_OK;
}
GECCO_API int gecco_crf_model_slot_table(const gecco_crf_model *m, int32_t label, double *pairs, double *dmax, int32_t *prod_max_cnt) {
    if (!m || m->m.L != 2 || label < 0 || label > 1) return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    gecco::SlotTable st;
    gecco::build_slot_table(m->m, label, st);
    if (pairs) std::memcpy(pairs, st.pairs.data(), st.pairs.size() * sizeof(double));
    if (dmax) *dmax = st.dmax;
    if (prod_max_cnt) *prod_max_cnt = st.prod_max_cnt;
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API int32_t gecco_crf_slot_prod_max_cnt(double dmax) { return gecco::slot_prod_max_cnt(dmax); }
GECCO_API int gecco_crf_model_trans_weights(const gecco_crf_model *m, double *w, uint8_t *present) {
    if (!m) return GECCO_CRF_EINVAL;
    if (w) std::memcpy(w, m->m.trans.data(), m->m.trans.size() * sizeof(double));
    if (present) std::memcpy(present, m->m.trans_mask.data(), m->m.trans_mask.size());
    return GECCO_CRF_OK;
}

GECCO_API int gecco_crf_device_count(int32_t *n) {
    if (!n) return GECCO_CRF_EINVAL;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
    return GECCO_CRF_OK;
}

// ---- plans -----------------------------------------------------------------------------
GECCO_API int gecco_crf_plan_create(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                    int32_t n_contigs, int32_t window, int32_t step, int32_t pad,
                                    gecco_crf_plan **out) {
    if (!m || !out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    if (device >= 0) {
        int rc = check_device(device);
        if (rc) return rc;
    }
    if (n_contigs > 0 && contig_ptr && contig_ptr[0] != 0) {
        set_error("contig_ptr[0] must be 0");
        return GECCO_CRF_EINVAL;
    }
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_plan> h(new gecco_crf_plan());
    int rc = plan_build(m->m, device, contig_ptr, n_contigs, window, step, pad, h->p);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API void gecco_crf_plan_free(gecco_crf_plan *p) {
    DeviceScope guard;
    delete p;
}
GECCO_API int32_t gecco_crf_plan_num_genes(const gecco_crf_plan *p) { return p ? p->p.n_genes : 0; }
GECCO_API int64_t gecco_crf_plan_num_windows(const gecco_crf_plan *p) { return p ? p->p.n_windows : 0; }
GECCO_API int32_t gecco_crf_plan_num_tiles(const gecco_crf_plan *p) { return p ? p->p.ntiles : 0; }
GECCO_API int32_t gecco_crf_plan_tile_out(const gecco_crf_plan *p) { return p ? p->p.tile_out : 0; }
GECCO_API const char *gecco_crf_plan_kernel_name(const gecco_crf_plan *p) { return p ? p->p.kernel_name.c_str() : ""; }

GECCO_API int gecco_crf_plan_run_windowed(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                          int32_t label, double *d_p_out, void *stream) {
    if (!p) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_windowed(p->p, {d_gene_ptr, d_attr_id}, label, d_p_out, static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_run_windowed_all(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                              int32_t background, double *d_p_all, double *d_p_any, void *stream) {
    if (!p) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_windowed_all(p->p, {d_gene_ptr, d_attr_id}, background, d_p_all, d_p_any, static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}
GECCO_API const char *gecco_crf_plan_all_kernel_name(const gecco_crf_plan *p) { return p ? plan_all_kernel_name(p->p) : ""; }

// `call` repeated on stream `s`: `warmup` times untimed, then `iters` times between two events
template <class Call>
static int time_calls(hipStream_t s, int32_t warmup, int32_t iters, float *ms_per_launch, Call call) {
    int rc;
    for (int i = 0; i < warmup; ++i)
        if ((rc = call())) return rc;
    hipEvent_t e0, e1;
    if ((rc = check_hip(hipEventCreate(&e0), "hipEventCreate"))) return rc;
    if ((rc = check_hip(hipEventCreate(&e1), "hipEventCreate"))) return rc;
    rc = check_hip(hipEventRecord(e0, s), "hipEventRecord");
    for (int i = 0; i < iters && !rc; ++i) rc = call();
    if (!rc) rc = check_hip(hipEventRecord(e1, s), "hipEventRecord");
    if (!rc) rc = check_hip(hipEventSynchronize(e1), "hipEventSynchronize");
    float ms = 0.f;
    if (!rc) rc = check_hip(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = ms / float(iters);
    return rc;
}

GECCO_API int gecco_crf_plan_time_windowed(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                           int32_t label, double *d_p_out, void *stream, int32_t warmup,
                                           int32_t iters, float *ms_per_launch) {
    if (!p || !ms_per_launch || iters <= 0) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_calls(s, warmup, iters, ms_per_launch, [&] { return plan_run_windowed(p->p, {d_gene_ptr, d_attr_id}, label, d_p_out, s); });
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_time_windowed_all(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                               int32_t background, double *d_p_all, double *d_p_any, void *stream,
                                               int32_t warmup, int32_t iters, float *ms_per_launch) {
    if (!p || !ms_per_launch || iters <= 0) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_calls(s, warmup, iters, ms_per_launch,
                      [&] { return plan_run_windowed_all(p->p, {d_gene_ptr, d_attr_id}, background, d_p_all, d_p_any, s); });
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_time_decode_pipelined(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                                   int32_t label, double *d_p_out, int8_t *d_y, void *stream, int32_t warmup,
                                                   int32_t iters, float *ms_per_launch) {
    if (!p || !ms_per_launch || iters <= 0) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    // the plan follows itself: call 0 primes (tiles only), every later call is one launch of tiles + Viterbi workgroups
    if ((rc = plan_run_decode_pipelined(&p->p, {d_gene_ptr, d_attr_id}, label, d_p_out, nullptr, nullptr, s))) return rc;
    rc = time_calls(s, warmup, iters, ms_per_launch,
                    [&] { return plan_run_decode_pipelined(&p->p, {d_gene_ptr, d_attr_id}, label, d_p_out, &p->p, d_y, s); });
    if (!rc) rc = plan_run_decode_pipelined(nullptr, {}, label, nullptr, &p->p, d_y, s);  // (flush)
    return rc;
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_viterbi_stats(gecco_crf_plan *p, int64_t out[4], int32_t reset) {
    if (!p || !out) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_viterbi_stats(p->p, out, reset != 0);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_run_decode(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                        int32_t label, double *d_p_out, int8_t *d_y, double *d_score, void *stream) {
    if (!p) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_decode(p->p, {d_gene_ptr, d_attr_id}, label, d_p_out, d_y, d_score, static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_plan_run_decode_pipelined(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id, int32_t label,
                                                  double *d_p_out, gecco_crf_plan *prev, int8_t *d_prev_y, void *stream) {
    if (!p && !prev) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_decode_pipelined(p ? &p->p : nullptr, {d_gene_ptr, d_attr_id}, label, d_p_out, prev ? &prev->p : nullptr, d_prev_y,
                                     static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_plan_run_marginals_full(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                                double *d_marg, double *d_lognorm, void *stream) {
    if (!p) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_marginals_full(p->p, {d_gene_ptr, d_attr_id}, d_marg, d_lognorm, static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_plan_run_viterbi(gecco_crf_plan *p, const int32_t *d_gene_ptr, const int32_t *d_attr_id,
                                         int8_t *d_y, double *d_score, void *stream) {
    if (!p) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_viterbi(p->p, {d_gene_ptr, d_attr_id}, d_y, d_score, static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}

// ---- pinned host memory -----------------------------------------------------------------------
GECCO_API int gecco_crf_host_alloc(size_t n_bytes, void **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    int32_t n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (pinned memory needs the HIP runtime)");
        return GECCO_CRF_ENODEV;
    }
    return check_hip(hipHostMalloc(out, n_bytes ? n_bytes : 1, hipHostMallocPortable), "hipHostMalloc");
}
GECCO_API void gecco_crf_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

// ---- batch driver -------------------------------------------------------------------------------
GECCO_API int gecco_crf_session_create(const gecco_crf_model *m, const int32_t *devices, int32_t n_devices,
                                       gecco_crf_session **out) {
    if (!m || !out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_session> h(new gecco_crf_session());
    int rc = session_create(m->m, devices, n_devices, &h->s);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API void gecco_crf_session_free(gecco_crf_session *s) {
    DeviceScope guard;
    delete s;
}
GECCO_API int gecco_crf_session_set_chunk_genes(gecco_crf_session *s, int32_t genes) {
    if (!s || genes <= 0) return GECCO_CRF_EINVAL;
    session_set_chunk_genes(*s->s, genes);
    return GECCO_CRF_OK;
}
GECCO_API int gecco_crf_session_set_direct_genes(gecco_crf_session *s, int32_t genes) {
    if (!s || genes < -1) return GECCO_CRF_EINVAL;  // (-1: back to the defaults, as the header documents)
    session_set_direct_genes(*s->s, genes);
    return GECCO_CRF_OK;
}
GECCO_API int gecco_crf_session_set_reference_bits(gecco_crf_session *s, int32_t on) {
    if (!s) return GECCO_CRF_EINVAL;
    session_set_reference_bits(*s->s, on != 0);
    return GECCO_CRF_OK;
}
GECCO_API int gecco_crf_exp_correctly_rounded(const double *x, int64_t n, double *out) {
    if (n < 0 || (n > 0 && (!x || !out))) return GECCO_CRF_EINVAL;
    for (int64_t i = 0; i < n; ++i) out[i] = gecco::ddx::exp_correctly_rounded(x[i]);
    return GECCO_CRF_OK;
}
GECCO_API int gecco_crf_session_stats(const gecco_crf_session *s, int32_t *n_chunks, int64_t *h2d_bytes, int64_t *d2h_bytes,
                                      double *host_plan_seconds, double *wall_seconds) {
    if (!s) return GECCO_CRF_EINVAL;
    const SessionStats st = session_stats(*s->s);
    if (n_chunks) *n_chunks = st.n_chunks;
    if (h2d_bytes) *h2d_bytes = st.h2d_bytes;
    if (d2h_bytes) *d2h_bytes = st.d2h_bytes;
    if (host_plan_seconds) *host_plan_seconds = st.host_plan_seconds;
    if (wall_seconds) *wall_seconds = st.wall_seconds;
    return GECCO_CRF_OK;
}

GECCO_API int gecco_crf_session_stats_ex(const gecco_crf_session *s, gecco_crf_session_stats_t *out) {
    if (!s || !out) return GECCO_CRF_EINVAL;
    const SessionStats st = session_stats(*s->s);
    out->n_chunks = st.n_chunks;
    out->n_devices = st.n_devices;
    out->direct = st.direct;
    out->host_threads = st.host_threads;
    out->h2d_bytes = st.h2d_bytes;
    out->d2h_bytes = st.d2h_bytes;
    out->host_plan_seconds = st.host_plan_seconds;
    out->host_issue_seconds = st.host_issue_seconds;
    out->wall_seconds = st.wall_seconds;
    return GECCO_CRF_OK;
}

namespace {
int run_guarded(Session &s, const BatchRequest &r) {
    GECCO_GUARD_BEGIN
    return session_run(s, r);
    GECCO_GUARD_END
}
BatchRequest csr_request(const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id) {
    BatchRequest r;
    r.contig_ptr = contig_ptr;
    r.n_contigs = n_contigs;
    r.gene_ptr = gene_ptr;
    r.attr_id = attr_id;
    return r;
}
}  // namespace

GECCO_API int gecco_crf_session_windowed(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                         const int32_t *gene_ptr, const int32_t *attr_id, int32_t window, int32_t step,
                                         int32_t label, int32_t pad, double *p_out) {
    if (!s || !p_out) return GECCO_CRF_EINVAL;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    return run_guarded(*s->s, r);
}
GECCO_API int gecco_crf_session_windowed_degrees(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                                 const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                                 int32_t window, int32_t step, int32_t label, int32_t pad, double *p_out) {
    if (!s || !p_out || !degree) return GECCO_CRF_EINVAL;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.degree = degree;
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    return run_guarded(*s->s, r);
}
GECCO_API int gecco_crf_session_decode(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                       const int32_t *gene_ptr, const int32_t *attr_id, int32_t window, int32_t step,
                                       int32_t label, int32_t pad, double *p_out, int8_t *y_out) {
    if (!s || !p_out || !y_out) return GECCO_CRF_EINVAL;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    r.y_out = y_out;
    return run_guarded(*s->s, r);
}
namespace {
SegParams seg_params(const gecco_crf_refine_params &q) {
    SegParams sp;
    sp.threshold = q.threshold;
    sp.average_threshold = q.average_threshold;
    sp.criterion = q.criterion;
    sp.n_cds = q.n_cds;
    sp.n_biopfams = q.n_biopfams;
    sp.edge_distance = q.edge_distance;
    sp.trim = q.trim ? 1 : 0;
    sp.carry = q.carry_state ? 1 : 0;
    sp.bio_ptr = q.marker_ptr;
    sp.bio_id = q.marker_id;
    return sp;
}
gecco_crf_refine_params gecco_params(double threshold, int32_t n_cds, int32_t edge_distance, int32_t trim, int32_t carry_state) {
    gecco_crf_refine_params q{};
    q.threshold = threshold;
    q.average_threshold = 0.6;
    q.criterion = 0;
    q.n_cds = n_cds;
    q.n_biopfams = 5;
    q.edge_distance = edge_distance;
    q.trim = trim;
    q.carry_state = carry_state;
    return q;
}
}  // namespace

GECCO_API int gecco_crf_session_decode_wire(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                            const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                            const uint16_t *attr_id16, int32_t window, int32_t step, int32_t label, int32_t pad,
                                            double *p_out, int8_t *y_out) {
    if (!s || !p_out) return GECCO_CRF_EINVAL;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.degree = degree;
    r.attr_id16 = attr_id16;
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    r.y_out = y_out;
    return run_guarded(*s->s, r);
}
GECCO_API int gecco_crf_session_clusters_ex(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                            const int32_t *gene_ptr, const int32_t *attr_id, const uint8_t *annotated,
                                            int32_t window, int32_t step, int32_t label, int32_t pad,
                                            const gecco_crf_refine_params *params, double *p_out, int32_t *seg_out,
                                            int32_t max_seg, int32_t *n_seg, double *seg_p_out, int64_t max_seg_genes,
                                            int64_t *seg_off_out) {
    return gecco_crf_session_clusters_degrees(s, contig_ptr, n_contigs, gene_ptr, nullptr, attr_id, annotated, window, step, label, pad,
                                              params, p_out, seg_out, max_seg, n_seg, seg_p_out, max_seg_genes, seg_off_out);
}
GECCO_API int gecco_crf_session_clusters_degrees(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                                 const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                                 const uint8_t *annotated, int32_t window, int32_t step, int32_t label, int32_t pad,
                                                 const gecco_crf_refine_params *params, double *p_out, int32_t *seg_out,
                                                 int32_t max_seg, int32_t *n_seg, double *seg_p_out, int64_t max_seg_genes,
                                                 int64_t *seg_off_out) {
    return gecco_crf_session_clusters_wire(s, contig_ptr, n_contigs, gene_ptr, degree, attr_id, nullptr, annotated, window, step, label,
                                           pad, params, p_out, seg_out, max_seg, n_seg, seg_p_out, max_seg_genes, seg_off_out);
}
GECCO_API int gecco_crf_session_clusters_wire(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                              const int32_t *gene_ptr, const uint8_t *degree, const int32_t *attr_id,
                                              const uint16_t *attr_id16, const uint8_t *annotated, int32_t window, int32_t step,
                                              int32_t label, int32_t pad, const gecco_crf_refine_params *params, double *p_out,
                                              int32_t *seg_out, int32_t max_seg, int32_t *n_seg, double *seg_p_out,
                                              int64_t max_seg_genes, int64_t *seg_off_out) {
    if (!s || !params) return GECCO_CRF_EINVAL;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.degree = degree;
    r.attr_id16 = attr_id16;
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    r.want_segments = true;
    r.annotated = annotated;
    r.seg = seg_params(*params);
    r.seg_out = seg_out;
    r.max_seg = max_seg;
    r.n_seg = n_seg;
    r.seg_p_out = seg_p_out;
    r.max_seg_genes = max_seg_genes;
    r.seg_off_out = seg_off_out;
    return run_guarded(*s->s, r);
}

GECCO_API int gecco_crf_session_clusters(gecco_crf_session *s, const int32_t *contig_ptr, int32_t n_contigs,
                                         const int32_t *gene_ptr, const int32_t *attr_id, const uint8_t *annotated,
                                         int32_t window, int32_t step, int32_t label, int32_t pad, double threshold,
                                         int32_t n_cds, int32_t edge_distance, int32_t trim, double *p_out, int32_t *seg_out,
                                         int32_t max_seg, int32_t *n_seg, double *seg_p_out, int64_t max_seg_genes,
                                         int64_t *seg_off_out) {
    const gecco_crf_refine_params q = gecco_params(threshold, n_cds, edge_distance, trim, 0);
    return gecco_crf_session_clusters_ex(s, contig_ptr, n_contigs, gene_ptr, attr_id, annotated, window, step, label, pad, &q, p_out,
                                         seg_out, max_seg, n_seg, seg_p_out, max_seg_genes, seg_off_out);
}

// ---- one-shot host entry points: thin wrappers over the model's own per-device session ------------
namespace {
int default_session(const gecco_crf_model *m, int32_t device, Session **out) {
    int rc = check_device(device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(m->m.dev_mutex);
    for (auto &e : m->m.sessions)
        if (e.first == device) {
            *out = e.second;
            return GECCO_CRF_OK;
        }
    Session *s = nullptr;
    if ((rc = session_create(m->m, &device, 1, &s))) return rc;
    m->m.sessions.emplace_back(device, s);
    *out = s;
    return GECCO_CRF_OK;
}
}  // namespace

GECCO_API int gecco_crf_windowed_marginals(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                           int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                           int32_t window, int32_t step, int32_t label, int32_t pad, double *p_out) {
    if (!m) return GECCO_CRF_EINVAL;
    int rc;
    if ((rc = check_window(window, step)) || (rc = check_label(m, label))) return rc;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    Session *s = nullptr;
    if ((rc = default_session(m, device, &s))) return rc;
    if (n_contigs > 0 && contig_ptr && contig_ptr[n_contigs] > 0 && !p_out) {
        set_error("null buffer");
        return GECCO_CRF_EINVAL;
    }
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.window = window;
    r.step = step;
    r.label = label;
    r.pad = pad;
    r.p_out = p_out;
    return session_run(*s, r);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_marginals_full(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                       int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                       double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    Session *s = nullptr;
    int rc = default_session(m, device, &s);
    if (rc) return rc;
    if (!marg && !lognorm) return GECCO_CRF_OK;
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.marg_out = marg;
    r.lognorm_out = lognorm;
    return session_run(*s, r);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_viterbi(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                const int32_t *gene_ptr, const int32_t *attr_id, int8_t *y_out, double *score) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    Session *s = nullptr;
    int rc = default_session(m, device, &s);
    if (rc) return rc;
    if (!y_out) {
        if (n_contigs > 0 && contig_ptr && contig_ptr[n_contigs] > 0) {
            set_error("null buffer");
            return GECCO_CRF_EINVAL;
        }
        return GECCO_CRF_OK;
    }
    BatchRequest r = csr_request(contig_ptr, n_contigs, gene_ptr, attr_id);
    r.y_out = y_out;
    r.score_out = score;
    return session_run(*s, r);
    GECCO_GUARD_END
}

// ---- one-shots on one plan over the whole batch: every label's windowed marginals (ABI 2.11.0), the entries with a value
// per attribute entry (ABI 2.13.0) and those with a mask of allowed labels per gene (ABI 2.15.0) ------------------------------
namespace {
// A batch resident on the device for one call: one plan over all of it, and one block with the rebased row pointers, the
// attribute ids, their values (a valued batch: csr.attr_value; null means unvalued), the masks of allowed labels (a masked batch:
// csr.allowed) and the outputs.
struct ResidentBatch {
    Plan plan;
    DeviceBlock<char> d;  // (after the plan: freed before it, with the plan's device still current)
    int64_t n = 0;  // genes
    DeviceCsr csr;
    size_t out_off[3] = {0, 0, 0};
    template <class T>
    T *out(int i) const {
        return d.at<T>(out_off[i]);
    }
};

// the caller's buffer for a per-gene output: needed as soon as the batch has a gene
int check_output(const int32_t *contig_ptr, int32_t n_contigs, const void *out) {
    return n_contigs > 0 && contig_ptr && contig_ptr[n_contigs] > contig_ptr[0] && !out ? fail("null buffer") : GECCO_CRF_OK;
}

int check_contig_ptr(const int32_t *contig_ptr, int32_t n_contigs) {
    return n_contigs < 0 || (n_contigs > 0 && !contig_ptr) ? fail("bad contig_ptr") : GECCO_CRF_OK;
}
uint32_t bits_beyond(int32_t L) { return L >= 32 ? 0u : ~0u << L; }  // the mask bits at or above L

// The checks of query q of a lattice call (`kind`: "span", "run"; a message starts with "span 3: "): its contig, whose length comes
// back for the entry's own range check, and its label set.  A call may bring ten thousand queries: the text is put together for
// a refusal only.
std::string query_name(const char *kind, int32_t q) { return std::string(kind) + " " + std::to_string(q) + ": "; }
int check_query_contig(const char *kind, int32_t q, int32_t c, int32_t n_contigs, const int32_t *contig_ptr, int64_t *len) {
    if (c < 0 || c >= n_contigs)
        return fail(query_name(kind, q) + "contig " + std::to_string(c) + " out of range (the batch has " + std::to_string(n_contigs) + ")");
    *len = int64_t(contig_ptr[c + 1]) - contig_ptr[c];
    return GECCO_CRF_OK;
}
int check_label_set(const char *kind, int32_t q, uint32_t mask, int32_t L) {
    if (mask == 0) return fail(query_name(kind, q) + "the label set is empty (a mask of 0)");
    if (mask & bits_beyond(L))
        return fail(query_name(kind, q) + "the set holds a label at or above num_labels = " + std::to_string(L) + " (mask " +
                    std::to_string(mask) + ")");
    return GECCO_CRF_OK;
}

// The host checks of the CSR arrays (before any device work), the plan, and the upload.  `valued`: the plan takes the any-L
// kernels at every label count and attr_value holds a finite value per attribute entry; otherwise attr_value is not read.
// `masked` (the *_constrained entries): `allowed` holds one mask per gene, indexed like the rows of gene_ptr (gene g of the caller's
// arrays), each with a bit below L and none at or above it; otherwise `allowed` is not read.
// Output i gets a part of the block, at b.out(i): per_gene[i] bytes for every gene (i = 0, 1), per_contig for every contig
// (i = 2).  Returns with b.n == 0 for a batch without genes (nothing to run).  empty_masks_ok: a mask of 0 is taken (the entry's
// kernels read the state scores alone, where such a gene is -infinity at every label: its contig has no path).
int batch_open(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
               const int32_t *attr_id, const double *attr_value, bool valued, const uint32_t *allowed, bool masked, int32_t window,
               int32_t step, int32_t pad, bool windowed, const size_t per_gene[2], size_t per_contig, ResidentBatch &b,
               bool empty_masks_ok = false) {
    int rc = check_contig_ptr(contig_ptr, n_contigs);
    if (rc) return rc;
    const int64_t n = n_contigs > 0 ? int64_t(contig_ptr[n_contigs]) - contig_ptr[0] : 0;
    if (n > 0 && !gene_ptr) return fail("null buffer");
    const int32_t *gp = n > 0 ? gene_ptr + contig_ptr[0] : nullptr;
    const int64_t a0 = n > 0 ? gp[0] : 0, nnz = n > 0 ? int64_t(gp[n]) - a0 : 0;
    if (nnz < 0 || (nnz > 0 && !attr_id)) return fail("bad gene_ptr");
    if (valued && nnz > 0 && !attr_value)
        return fail("null attr_value with attribute entries (the unvalued entry takes attributes without values)");
    double vmax = 0.0;
    for (int64_t k = 0; valued && k < nnz; ++k) {
        const double v = attr_value[a0 + k];
        if (!std::isfinite(v)) {
            set_error("attribute value " + std::to_string(a0 + k) + " is not finite (NaN or infinite)");
            return GECCO_CRF_EINVAL;
        }
        vmax = std::max(vmax, std::fabs(v));
    }
    if (masked && n > 0) {
        if (!allowed) return fail("null allowed with genes (one mask of allowed labels per gene)");
        const int32_t L = m->m.L;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t g = int64_t(contig_ptr[0]) + i;
            if (allowed[g] == 0 && !empty_masks_ok) return fail("constrained: gene " + std::to_string(g) + " allows no label (a mask of 0)");
            if (allowed[g] & bits_beyond(L))
                return fail("constrained: gene " + std::to_string(g) + " allows a label at or above num_labels = " + std::to_string(L) +
                            " (mask " + std::to_string(allowed[g]) + ")");
        }
    }
    if ((rc = check_device(device))) return rc;
    b.plan.valued = valued;
    b.plan.masked = masked;
    b.plan.windowed_use = windowed;
    if ((rc = plan_build(m->m, device, contig_ptr, n_contigs, window, step, pad, b.plan))) return rc;
    if (b.plan.n_genes == 0) return GECCO_CRF_OK;
    const size_t b_gp = size_t(n + 1) * 4, n_at = size_t(nnz ? nnz : 1);
    Carver blk;
    const size_t o_gp = blk.take(b_gp), o_at = blk.take(n_at * 4), o_val = valued ? blk.take(n_at * 8) : 0;
    const size_t o_mask = masked ? blk.take(size_t(n) * 4) : 0;
    b.out_off[0] = blk.take(per_gene[0] * size_t(n) + 8);
    b.out_off[1] = blk.take(per_gene[1] * size_t(n) + 8);
    b.out_off[2] = blk.take(per_contig * size_t(n_contigs) + 8);
    if ((rc = b.d.alloc(blk.off, "hipMalloc batch"))) return rc;
    // (gene_ptr may carry any base offset: the kernels index attr_id with its values, so the row pointers are rebased on the
    // host, and ids and values go up from that base)
    std::vector<int32_t> rows(size_t(n) + 1);
    for (int64_t i = 0; i <= n; ++i) rows[size_t(i)] = int32_t(gp[i] - a0);
    rc = check_hip(hipMemcpy(b.d.get() + o_gp, rows.data(), b_gp, hipMemcpyHostToDevice), "upload gene_ptr");
    if (!rc && nnz) rc = check_hip(hipMemcpy(b.d.get() + o_at, attr_id + a0, size_t(nnz) * 4, hipMemcpyHostToDevice), "upload attr_id");
    if (!rc && nnz && valued)
        rc = check_hip(hipMemcpy(b.d.get() + o_val, attr_value + a0, size_t(nnz) * 8, hipMemcpyHostToDevice), "upload attr_value");
    if (!rc && masked)
        rc = check_hip(hipMemcpy(b.d.get() + o_mask, allowed + contig_ptr[0], size_t(n) * 4, hipMemcpyHostToDevice), "upload allowed");
    if (rc) return rc;
    b.n = n;
    b.csr.gene_ptr = reinterpret_cast<const int32_t *>(b.d.get() + o_gp);
    b.csr.attr_id = reinterpret_cast<const int32_t *>(b.d.get() + o_at);
    if (valued) {
        b.csr.attr_value = reinterpret_cast<const double *>(b.d.get() + o_val);
        b.csr.vmax_abs = vmax;
    }
    if (masked) b.csr.allowed = reinterpret_cast<const uint32_t *>(b.d.get() + o_mask);
    return GECCO_CRF_OK;
}

// after the run call: waits for the device ...
int batch_wait(int rc, const char *what) { return rc ? rc : check_hip(hipStreamSynchronize(nullptr), what); }
// ... and brings an output back (one the caller did not ask for is skipped)
int batch_fetch(int rc, void *dst, const void *src, size_t bytes, const char *what) {
    if (rc || !dst || !bytes) return rc;
    return check_hip(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), what);
}

int windowed_all(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                 const int32_t *attr_id, const double *attr_value, bool valued, const uint32_t *allowed, bool masked, int32_t window,
                 int32_t step, int32_t background, int32_t pad, double *p_all, double *p_any) {
    if (!m) return GECCO_CRF_EINVAL;
    int rc;
    if ((rc = check_window(window, step)) || (rc = check_background(m, background, p_any))) return rc;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    if ((rc = check_output(contig_ptr, n_contigs, p_all))) return rc;
    ResidentBatch b;
    const size_t L = size_t(m->m.L), per_gene[2] = {L * 8, 8};
    rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, valued, allowed, masked, window, step, pad, true,
                    per_gene, 0, b);
    if (rc || b.n == 0) return rc;
    rc = plan_run_windowed_all(b.plan, b.csr, background, b.out<double>(0), p_any ? b.out<double>(1) : nullptr, nullptr);
    rc = batch_wait(rc, "windowed marginals");
    rc = batch_fetch(rc, p_all, b.out<double>(0), size_t(b.n) * L * 8, "download p_all");
    return batch_fetch(rc, p_any, b.out<double>(1), size_t(b.n) * 8, "download p_any");
    GECCO_GUARD_END
}
}  // namespace

GECCO_API int gecco_crf_windowed_marginals_all(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                               int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                               int32_t window, int32_t step, int32_t background, int32_t pad, double *p_all,
                                               double *p_any) {
    return windowed_all(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, nullptr, false, nullptr, false, window, step, background,
                        pad, p_all, p_any);
}

GECCO_API int gecco_crf_windowed_marginals_all_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                      int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                      const double *attr_value, int32_t window, int32_t step,
                                                      int32_t background, int32_t pad, double *p_all, double *p_any) {
    return windowed_all(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, true, nullptr, false, window, step, background,
                        pad, p_all, p_any);
}

namespace {
// The three other one-shots of the family, with values (`valued`), masks (`masked`) or both.
int windowed_one(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                 const int32_t *attr_id, const double *attr_value, bool valued, const uint32_t *allowed, bool masked, int32_t window,
                 int32_t step, int32_t label, int32_t pad, double *p_out) {
    if (!m) return GECCO_CRF_EINVAL;
    int rc;
    if ((rc = check_window(window, step)) || (rc = check_label(m, label))) return rc;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    if ((rc = check_output(contig_ptr, n_contigs, p_out))) return rc;
    ResidentBatch b;
    const size_t per_gene[2] = {8, 0};
    rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, valued, allowed, masked, window, step, pad, true,
                    per_gene, 0, b);
    if (rc || b.n == 0) return rc;
    rc = batch_wait(plan_run_windowed(b.plan, b.csr, label, b.out<double>(0), nullptr), "windowed marginals");
    return batch_fetch(rc, p_out, b.out<double>(0), size_t(b.n) * 8, "download p");
    GECCO_GUARD_END
}

int marginals_full_one(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                       const int32_t *attr_id, const double *attr_value, bool valued, const uint32_t *allowed, bool masked,
                       double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    if (!marg && !lognorm) return GECCO_CRF_OK;
    ResidentBatch b;
    const size_t L = size_t(m->m.L), per_gene[2] = {L * 8, 0};
    int rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, valued, allowed, masked, 1, 1, 1, false, per_gene,
                        8, b);
    if (rc || b.n == 0) {
        for (int32_t c = 0; !rc && lognorm && c < n_contigs; ++c) lognorm[c] = 0.0;  // (contigs without genes: log Z = 0)
        return rc;
    }
    // (the device always writes both; the caller's missing buffer is simply not fetched)
    rc = batch_wait(plan_run_marginals_full(b.plan, b.csr, b.out<double>(0), b.out<double>(2), nullptr), "marginals");
    rc = batch_fetch(rc, marg, b.out<double>(0), size_t(b.n) * L * 8, "download marginals");
    return batch_fetch(rc, lognorm, b.out<double>(2), size_t(n_contigs) * 8, "download lognorm");
    GECCO_GUARD_END
}

int viterbi_one(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                const int32_t *attr_id, const double *attr_value, bool valued, const uint32_t *allowed, bool masked, int8_t *y_out,
                double *score) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    if (!y_out) return check_output(contig_ptr, n_contigs, y_out);  // (no genes: nothing to label)
    ResidentBatch b;
    const size_t per_gene[2] = {1, 0};
    int rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, valued, allowed, masked, 1, 1, 1, false, per_gene,
                        8, b);
    if (rc || b.n == 0) {
        for (int32_t c = 0; !rc && score && c < n_contigs; ++c) score[c] = 0.0;
        return rc;
    }
    rc = batch_wait(plan_run_viterbi(b.plan, b.csr, b.out<int8_t>(0), b.out<double>(2), nullptr), "viterbi");
    rc = batch_fetch(rc, y_out, b.out<int8_t>(0), size_t(b.n), "download labels");
    return batch_fetch(rc, score, b.out<double>(2), size_t(n_contigs) * 8, "download score");
    GECCO_GUARD_END
}
}  // namespace

GECCO_API int gecco_crf_windowed_marginals_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                  int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                  const double *attr_value, int32_t window, int32_t step, int32_t label,
                                                  int32_t pad, double *p_out) {
    return windowed_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, true, nullptr, false, window, step, label, pad,
                        p_out);
}

GECCO_API int gecco_crf_marginals_full_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                              int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                              const double *attr_value, double *marg, double *lognorm) {
    return marginals_full_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, true, nullptr, false, marg, lognorm);
}

GECCO_API int gecco_crf_viterbi_valued(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                       const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                       int8_t *y_out, double *score) {
    return viterbi_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, true, nullptr, false, y_out, score);
}

// ---- allowed-label sets at inference (ABI 2.15.0): the *_valued arguments plus one mask per gene; attr_value may be NULL (no
// values), so one family serves masked calls with and without values
GECCO_API int gecco_crf_windowed_marginals_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                       int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                       const double *attr_value, const uint32_t *allowed, int32_t window,
                                                       int32_t step, int32_t label, int32_t pad, double *p_out) {
    return windowed_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed, true, window,
                        step, label, pad, p_out);
}

GECCO_API int gecco_crf_windowed_marginals_all_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                           int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                           const double *attr_value, const uint32_t *allowed, int32_t window,
                                                           int32_t step, int32_t background, int32_t pad, double *p_all,
                                                           double *p_any) {
    return windowed_all(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed, true, window,
                        step, background, pad, p_all, p_any);
}

GECCO_API int gecco_crf_marginals_full_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr,
                                                   int32_t n_contigs, const int32_t *gene_ptr, const int32_t *attr_id,
                                                   const double *attr_value, const uint32_t *allowed, double *marg,
                                                   double *lognorm) {
    return marginals_full_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed, true, marg,
                              lognorm);
}

GECCO_API int gecco_crf_viterbi_constrained(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                            const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                            const uint32_t *allowed, int8_t *y_out, double *score) {
    return viterbi_one(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed, true, y_out,
                       score);
}

namespace {
// gecco_crf_marginals_full for LatticeCall::finish.  That entry takes batches that start at gene 0: a slice is rebased for it, rows
// and attribute entries alike.
int marginals_full_of_slice(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                            const int32_t *gene_ptr, const int32_t *attr_id, double *marg, double *lognorm) {
    if (contig_ptr[0] == 0) return gecco_crf_marginals_full(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, marg, lognorm);
    const int32_t g0 = contig_ptr[0], a0 = gene_ptr[g0];
    std::vector<int32_t> contigs(size_t(n_contigs) + 1), rows(size_t(contig_ptr[n_contigs] - g0) + 1);
    for (size_t c = 0; c < contigs.size(); ++c) contigs[c] = contig_ptr[c] - g0;
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = gene_ptr[size_t(g0) + i] - a0;
    return gecco_crf_marginals_full(m, device, contigs.data(), n_contigs, rows.data(), attr_id ? attr_id + a0 : nullptr, marg, lognorm);
}

// One call of a lattice query -- region posteriors, sampled paths, the K best paths, edge posteriors, minimum-run decoding, run counts.  The batch goes to the device on a plan laid
// out with `lattice`: the marginals at out(0), per_gene1 bytes a gene at out(1), log Z and then per_contig_more bytes a contig at
// out(2).  `run(b)` is the entry's part: its plan_run_* call and the fetch of its own outputs; of a batch without genes (b.n == 0:
// nothing is on the device, and log Z = 0 is written by then) it only fills what else the entry returns.  marg / lognorm (either
// may be null) are the bytes of the marginals entry of the same kind.  That entry runs the any-L kernels too, with one exception:
// a 2-label model without values and masks has kernels of its own there (own_l2), which are asked in a second pass once the batch
// has left the device.
template <class Run>
int lattice_call(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                 const int32_t *attr_id, const double *attr_value, const uint32_t *allowed, size_t per_gene1, size_t per_contig_more,
                 double *marg, double *lognorm, Run run) {
    const size_t L = size_t(m->m.L);
    const bool own_l2 = L == 2 && !attr_value && !allowed && (marg || lognorm);
    {
        ResidentBatch b;
        b.plan.lattice = true;
        const size_t per_gene[2] = {L * 8, per_gene1};
        int rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed,
                            allowed != nullptr, 1, 1, 1, false, per_gene, 8 + per_contig_more, b);
        for (int32_t c = 0; !rc && b.n == 0 && lognorm && c < n_contigs; ++c) lognorm[c] = 0.0;
        if (!rc) rc = run(b);
        if (rc || b.n == 0) return rc;
        if (!own_l2) {
            rc = batch_fetch(rc, marg, b.out<double>(0), size_t(b.n) * L * 8, "download marginals");
            return batch_fetch(rc, lognorm, b.out<double>(2), size_t(n_contigs) * 8, "download lognorm");
        }
    }
    return marginals_full_of_slice(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, marg, lognorm);
}
// the checks of a query's place in its contig of `len` genes: a half-open range [b, e), or one item t (`word`: what the entry calls it)
int check_query_range(const char *kind, int32_t q, int32_t c, int32_t b, int32_t e, int64_t len) {
    if (b < 0 || b >= e || e > len)
        return fail(query_name(kind, q) + "[" + std::to_string(b) + ", " + std::to_string(e) + ") is not a non-empty range inside contig " +
                    std::to_string(c) + " of " + std::to_string(len) + " genes");
    return GECCO_CRF_OK;
}
int check_query_item(const char *kind, const char *word, int32_t q, int32_t c, int32_t t, int64_t len) {
    if (t < 0 || t >= len)
        return fail(query_name(kind, q) + word + " " + std::to_string(t) + " lies outside contig " + std::to_string(c) + " of " +
                    std::to_string(len) + " genes");
    return GECCO_CRF_OK;
}
// a lattice entry without queries is the whole-contig marginals' own call, of the batch's kind
int marginals_full_of_kind(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *gene_ptr,
                           const int32_t *attr_id, const double *attr_value, const uint32_t *allowed, double *marg, double *lognorm) {
    if (allowed) return gecco_crf_marginals_full_constrained(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, marg, lognorm);
    if (attr_value) return gecco_crf_marginals_full_valued(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, marg, lognorm);
    return gecco_crf_marginals_full(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, marg, lognorm);
}
// the device block of an entry's queries: `total` bytes, the `bytes` of `host` at its head
int upload_queries(DeviceBlock<char> &q, const void *host, size_t bytes, size_t total, const char *what_alloc, const char *what_copy) {
    const int rc = q.alloc(total, what_alloc);
    return rc ? rc : check_hip(hipMemcpy(q.get(), host, bytes, hipMemcpyHostToDevice), what_copy);
}
// the n_spans queries of the span entries, each checked ("span 3: ..."), as the kernels take them
int checked_spans(const gecco_crf_model *m, const int32_t *contig_ptr, int32_t n_contigs, const int32_t *span_contig,
                  const int32_t *span_begin, const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans,
                  std::vector<SpanQuery> &spans) {
    spans.resize(static_cast<size_t>(n_spans));
    for (int32_t q = 0; q < n_spans; ++q) {
        const int32_t c = span_contig[q], b = span_begin[q], e = span_end[q];
        int64_t len;
        int rc;
        if ((rc = check_query_contig("span", q, c, n_contigs, contig_ptr, &len))) return rc;
        if ((rc = check_query_range("span", q, c, b, e, len))) return rc;
        if ((rc = check_label_set("span", q, span_mask[q], m->m.L))) return rc;
        spans[size_t(q)] = SpanQuery{c, b, e, span_mask[q]};
    }
    return GECCO_CRF_OK;
}
// The rows of the conditionals entry: query q's are the genes max(begin - reach, 0) .. min(end + reach, T) of its contig.  Fills
// the library's own row_ptr [n_spans + 1], fwd_ptr [n_spans + 1] (cumulative span lengths) and, with the caller's occ_ptr,
// occ [n_rows + 1] (cumulative attribute-occurrence counts of the rows' genes), and holds the caller's two arrays to them
// ("span 3: ..."): a caller whose buffers were sized from other numbers is refused before anything is written.
int check_conditional_rows(const std::vector<SpanQuery> &spans, int32_t reach, const int32_t *contig_ptr, const int32_t *gene_ptr,
                           const int64_t *row_ptr, const int64_t *occ_ptr, std::vector<int64_t> &rows, std::vector<int64_t> &fwd,
                           std::vector<int64_t> &occ) {
    const size_t n = spans.size();
    rows.assign(n + 1, 0);
    fwd.assign(n + 1, 0);
    if (row_ptr[0] != 0) return fail(query_name("span", 0) + "row_ptr[0] = " + std::to_string(row_ptr[0]) + ", expected 0");
    for (size_t q = 0; q < n; ++q) {
        const SpanQuery &s = spans[q];
        const int64_t len = int64_t(contig_ptr[s.contig + 1]) - contig_ptr[s.contig];
        const int64_t lo = std::max<int64_t>(int64_t(s.begin) - reach, 0), hi = std::min<int64_t>(int64_t(s.end) + reach, len);
        rows[q + 1] = rows[q] + (hi - lo);
        fwd[q + 1] = fwd[q] + (s.end - s.begin);
        if (row_ptr[q + 1] != rows[q + 1])
            return fail(query_name("span", int32_t(q)) + "row_ptr[" + std::to_string(q + 1) + "] = " + std::to_string(row_ptr[q + 1]) +
                        ", expected " + std::to_string(rows[q + 1]) + " (the span's rows are the genes " + std::to_string(lo) + " .. " +
                        std::to_string(hi) + " of contig " + std::to_string(s.contig) + " at reach " + std::to_string(reach) + ")");
    }
    occ.clear();
    if (!occ_ptr) return GECCO_CRF_OK;
    occ.assign(size_t(rows[n]) + 1, 0);
    if (occ_ptr[0] != 0) return fail(query_name("span", 0) + "occ_ptr[0] = " + std::to_string(occ_ptr[0]) + ", expected 0");
    for (size_t q = 0; q < n; ++q) {
        const SpanQuery &s = spans[q];
        const int64_t g_lo = int64_t(contig_ptr[s.contig]) + std::max<int64_t>(int64_t(s.begin) - reach, 0);
        for (int64_t r = rows[q]; r < rows[q + 1]; ++r) {
            const int64_t g = g_lo + (r - rows[q]);
            occ[size_t(r) + 1] = occ[size_t(r)] + (int64_t(gene_ptr[g + 1]) - gene_ptr[g]);
            if (occ_ptr[r + 1] != occ[size_t(r) + 1])
                return fail(query_name("span", int32_t(q)) + "occ_ptr[" + std::to_string(r + 1) + "] = " + std::to_string(occ_ptr[r + 1]) +
                            ", expected " + std::to_string(occ[size_t(r) + 1]) + " (gene " + std::to_string(g) + " carries " +
                            std::to_string(int64_t(gene_ptr[g + 1]) - gene_ptr[g]) + " attribute occurrences)");
        }
    }
    return GECCO_CRF_OK;
}
}  // namespace

// ---- region posteriors (ABI 2.16.0): log P(every gene of a span carries a label of a set | x) on the whole-contig lattice, any
// number of spans behind one forward-backward pass of the batch (crf_spans.hip)
GECCO_API int gecco_crf_span_probabilities(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                           const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                           const uint32_t *allowed, const int32_t *span_contig, const int32_t *span_begin,
                                           const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans, double *logp,
                                           double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the spans, on the host and before any device work
    if (n_spans < 0) return fail("span_probabilities: negative number of spans");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_spans > 0 && (!span_contig || !span_begin || !span_end || !span_mask || !logp)) return fail("null buffer");
    std::vector<SpanQuery> spans;
    if ((rc = checked_spans(m, contig_ptr, n_contigs, span_contig, span_begin, span_end, span_mask, n_spans, spans))) return rc;
    // without spans the call is the whole-contig marginals' own
    if (n_spans == 0) return marginals_full_of_kind(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, marg, lognorm);
    // (a batch without genes cannot be: a checked span lies inside a contig with genes)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 0, 0, marg, lognorm, [&](ResidentBatch &b) {
        DeviceBlock<char> q;
        const size_t b_spans = align256(size_t(n_spans) * sizeof(SpanQuery));
        int rc = upload_queries(q, spans.data(), size_t(n_spans) * sizeof(SpanQuery), b_spans + size_t(n_spans) * 8, "hipMalloc spans",
                                "upload spans");
        if (rc) return rc;
        double *d_logp = reinterpret_cast<double *>(q.get() + b_spans);
        rc = batch_wait(plan_run_span_probabilities(b.plan, b.csr, reinterpret_cast<const SpanQuery *>(q.get()), n_spans, d_logp,
                                                    b.out<double>(0), b.out<double>(2), nullptr), "span probabilities");
        return batch_fetch(rc, logp, d_logp, size_t(n_spans) * 8, "download logp");
    });
    GECCO_GUARD_END
}

// ---- marginals given a region and knock-out attributions (ABI 2.24.0): c_t(l) = P(y_t = l | every gene of the span carries a
// label of the set, x) for the genes of a span and `reach` genes on either side, and from them the exact change of the span's
// log-probability when a gene, or one attribute occurrence of it, is taken out; any number of spans behind one forward-backward
// pass of the batch (crf_conditionals.hip)
GECCO_API int gecco_crf_span_conditionals(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                          const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                          const uint32_t *allowed, const int32_t *span_contig, const int32_t *span_begin,
                                          const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans, int32_t reach,
                                          const int64_t *row_ptr, const int64_t *occ_ptr, double *logp, double *cond,
                                          double *item_contribution, double *attr_contribution, double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the spans and of the caller's row tables, on the host and before any device work
    if (n_spans < 0) return fail("span_conditionals: negative number of spans");
    if (reach < 0) return fail("span_conditionals: reach = " + std::to_string(reach) + " is negative");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_spans > 0 && (!span_contig || !span_begin || !span_end || !span_mask || !logp || !row_ptr || !cond)) return fail("null buffer");
    if (n_spans > 0 && attr_contribution && !occ_ptr) return fail("span_conditionals: attr_contribution without occ_ptr");
    std::vector<SpanQuery> spans;
    if ((rc = checked_spans(m, contig_ptr, n_contigs, span_contig, span_begin, span_end, span_mask, n_spans, spans))) return rc;
    // without spans the call is the whole-contig marginals' own
    if (n_spans == 0) return marginals_full_of_kind(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, marg, lognorm);
    if (!gene_ptr) return fail("null buffer");  // (a checked span lies inside a contig with genes)
    std::vector<int64_t> rows, fwd, occ;
    if ((rc = check_conditional_rows(spans, reach, contig_ptr, gene_ptr, row_ptr, occ_ptr, rows, fwd, occ))) return rc;
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 0, 0, marg, lognorm, [&](ResidentBatch &b) {
        // one block: the spans, the three row tables, then logp, the walks' two workspaces, cond, and the two contributions
        const size_t ns = size_t(n_spans), L = size_t(m->m.L), n_rows = size_t(rows[ns]), n_fwd = size_t(fwd[ns]);
        const size_t n_occ = occ.empty() ? 0 : size_t(occ[n_rows]);
        Carver at;
        at.take(ns * sizeof(SpanQuery));
        const size_t o_rows = at.take((ns + 1) * 8), o_fwd = at.take((ns + 1) * 8), o_occ = at.take(occ.size() * 8 + 8);
        const size_t b_host = at.off;
        const size_t o_logp = at.take(ns * 8), o_vec = at.take(n_fwd * L * 8), o_walk = at.take(n_rows * L * 8 + 8),
                     o_cond = at.take(n_rows * L * 8 + 8), o_item = at.take(n_rows * 8 + 8), o_attr = at.take(n_occ * 8 + 8);
        std::vector<char> host(b_host, 0);
        std::memcpy(host.data(), spans.data(), ns * sizeof(SpanQuery));
        std::memcpy(host.data() + o_rows, rows.data(), (ns + 1) * 8);
        std::memcpy(host.data() + o_fwd, fwd.data(), (ns + 1) * 8);
        if (!occ.empty()) std::memcpy(host.data() + o_occ, occ.data(), occ.size() * 8);
        DeviceBlock<char> q;
        int rc = upload_queries(q, host.data(), b_host, at.off, "hipMalloc span conditionals", "upload spans");
        if (rc) return rc;
        ConditionalArgs a{};
        a.spans = reinterpret_cast<const SpanQuery *>(q.get());
        a.n_spans = n_spans;
        a.reach = reach;
        a.n_rows = int64_t(n_rows);
        a.n_fwd = int64_t(n_fwd);
        a.n_occ = int64_t(n_occ);
        a.row_ptr = reinterpret_cast<const int64_t *>(q.get() + o_rows);
        a.fwd_ptr = reinterpret_cast<const int64_t *>(q.get() + o_fwd);
        a.occ_ptr = occ.empty() ? nullptr : reinterpret_cast<const int64_t *>(q.get() + o_occ);
        a.fwd = reinterpret_cast<double *>(q.get() + o_vec);
        a.walk = reinterpret_cast<double *>(q.get() + o_walk);
        a.cond = reinterpret_cast<double *>(q.get() + o_cond);
        a.item = reinterpret_cast<double *>(q.get() + o_item);
        a.attr = reinterpret_cast<double *>(q.get() + o_attr);
        double *d_logp = reinterpret_cast<double *>(q.get() + o_logp);
        rc = batch_wait(plan_run_span_conditionals(b.plan, b.csr, a, d_logp, b.out<double>(0), b.out<double>(2), nullptr),
                        "span conditionals");
        rc = batch_fetch(rc, logp, d_logp, ns * 8, "download logp");
        rc = batch_fetch(rc, cond, a.cond, n_rows * L * 8, "download cond");
        rc = batch_fetch(rc, item_contribution, a.item, n_rows * 8, "download item_contribution");
        return batch_fetch(rc, a.occ_ptr ? attr_contribution : nullptr, a.attr, n_occ * 8, "download attr_contribution");
    });
    GECCO_GUARD_END
}

// ---- run posteriors (ABI 2.21.0): the exact start and end distributions of the run through an anchor, and the probability that
// a run is exactly a range, any number of queries behind one forward-backward pass of the batch (crf_runs.hip)
GECCO_API int gecco_crf_run_posteriors(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                       const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                       const uint32_t *allowed, const int32_t *anchor_contig, const int32_t *anchor_item,
                                       const uint32_t *anchor_mask, int32_t n_anchors, int32_t reach, double *log_anchor,
                                       double *log_start, double *log_start_beyond, double *log_end, double *log_end_beyond,
                                       const int32_t *run_contig, const int32_t *run_begin, const int32_t *run_end,
                                       const uint32_t *run_mask, int32_t n_runs, double *log_run, double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the queries, on the host and before any device work
    if (n_anchors < 0 || n_runs < 0) return fail("run_posteriors: negative number of anchors or runs");
    if (reach < 0 || reach > kMaxRunReach) return fail("run_posteriors: reach = " + std::to_string(reach) + " is outside 0 .. 65536");
    if (int64_t(n_anchors) * (int64_t(reach) + 1) >= (int64_t(1) << 31))
        return fail("run_posteriors: n_anchors * (reach + 1) = " + std::to_string(int64_t(n_anchors) * (int64_t(reach) + 1)) +
                    " does not stay below 2^31");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_anchors > 0 && (!anchor_contig || !anchor_item || !anchor_mask || !log_anchor || !log_start || !log_start_beyond || !log_end ||
                          !log_end_beyond))
        return fail("null buffer");
    if (n_runs > 0 && (!run_contig || !run_begin || !run_end || !run_mask || !log_run)) return fail("null buffer");
    std::vector<RunQuery> anchors(static_cast<size_t>(n_anchors));
    for (int32_t q = 0; q < n_anchors; ++q) {
        const int32_t c = anchor_contig[q], t = anchor_item[q];
        int64_t len;
        if ((rc = check_query_contig("anchor", q, c, n_contigs, contig_ptr, &len))) return rc;
        if ((rc = check_query_item("anchor", "item", q, c, t, len))) return rc;
        if ((rc = check_label_set("anchor", q, anchor_mask[q], m->m.L))) return rc;
        anchors[size_t(q)] = RunQuery{c, t, anchor_mask[q]};
    }
    std::vector<SpanQuery> runs(static_cast<size_t>(n_runs));
    for (int32_t q = 0; q < n_runs; ++q) {
        const int32_t c = run_contig[q], b = run_begin[q], e = run_end[q];
        int64_t len;
        if ((rc = check_query_contig("run", q, c, n_contigs, contig_ptr, &len))) return rc;
        if ((rc = check_query_range("run", q, c, b, e, len))) return rc;
        if ((rc = check_label_set("run", q, run_mask[q], m->m.L))) return rc;
        runs[size_t(q)] = SpanQuery{c, b, e, run_mask[q]};
    }
    // without queries the call is the whole-contig marginals' own
    if (n_anchors == 0 && n_runs == 0) return marginals_full_of_kind(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, marg, lognorm);
    // (a batch without genes cannot be: a checked query lies inside a contig with genes)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 0, 0, marg, lognorm, [&](ResidentBatch &b) {
        // one block: the anchors, the runs, then the outputs in the order log_anchor, start_beyond, end_beyond, run, start, end
        const size_t na = size_t(n_anchors), nr = size_t(n_runs), row = size_t(reach) + 1;
        const size_t b_anchors = align256(na * sizeof(RunQuery)), b_runs = align256(nr * sizeof(SpanQuery));
        const size_t n_small = 3 * na + nr, n_out = n_small + 2 * na * row;
        std::vector<char> host(b_anchors + b_runs);
        if (na) std::memcpy(host.data(), anchors.data(), na * sizeof(RunQuery));
        if (nr) std::memcpy(host.data() + b_anchors, runs.data(), nr * sizeof(SpanQuery));
        DeviceBlock<char> q;
        int rc = upload_queries(q, host.data(), host.size(), host.size() + n_out * 8, "hipMalloc run queries", "upload run queries");
        if (rc) return rc;
        double *d_out = reinterpret_cast<double *>(q.get() + host.size());
        RunPosteriorArgs a{};
        a.anchors = reinterpret_cast<const RunQuery *>(q.get());
        a.runs = reinterpret_cast<const SpanQuery *>(q.get() + b_anchors);
        a.n_anchors = n_anchors;
        a.n_runs = n_runs;
        a.reach = reach;
        a.log_anchor = d_out;
        a.log_start_beyond = d_out + na;
        a.log_end_beyond = d_out + 2 * na;
        a.log_run = d_out + 3 * na;
        a.log_start = d_out + n_small;
        a.log_end = a.log_start + na * row;
        rc = batch_wait(plan_run_run_posteriors(b.plan, b.csr, a, b.out<double>(0), b.out<double>(2), nullptr), "run posteriors");
        if (na) {
            rc = batch_fetch(rc, log_anchor, a.log_anchor, na * 8, "download log_anchor");
            rc = batch_fetch(rc, log_start_beyond, a.log_start_beyond, na * 8, "download log_start_beyond");
            rc = batch_fetch(rc, log_end_beyond, a.log_end_beyond, na * 8, "download log_end_beyond");
            rc = batch_fetch(rc, log_start, a.log_start, na * row * 8, "download log_start");
            rc = batch_fetch(rc, log_end, a.log_end, na * row * 8, "download log_end");
        }
        if (nr) rc = batch_fetch(rc, log_run, a.log_run, nr * 8, "download log_run");
        return rc;
    });
    GECCO_GUARD_END
}

// ---- label paths drawn from the posterior (ABI 2.17.0): forward filtering by the whole-contig marginals pass, backward sampling
// and the run queries behind it (crf_sample.hip)
GECCO_API int gecco_crf_sample_paths(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                     const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                     const uint32_t *allowed, int32_t n_samples, uint64_t seed, const int32_t *run_contig,
                                     const int32_t *run_anchor, const uint32_t *run_mask, int32_t n_runs, int8_t *y, int32_t *runs,
                                     double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (n_samples < 1 || n_samples > kMaxSamples)
        return fail("sample_paths: n_samples = " + std::to_string(n_samples) + " is outside 1 .. 1048576");
    if (n_runs < 0) return fail("sample_paths: negative n_runs");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_runs > 0 && (!run_contig || !run_anchor || !run_mask || !runs)) return fail("null buffer");
    std::vector<RunQuery> queries(static_cast<size_t>(n_runs));
    for (int32_t q = 0; q < n_runs; ++q) {
        const int32_t c = run_contig[q], t = run_anchor[q];
        int64_t len;
        if ((rc = check_query_contig("run", q, c, n_contigs, contig_ptr, &len))) return rc;
        if ((rc = check_query_item("run", "anchor", q, c, t, len))) return rc;
        if ((rc = check_label_set("run", q, run_mask[q], m->m.L))) return rc;
        queries[size_t(q)] = RunQuery{c, t, run_mask[q]};
    }
    // per gene: the paths, which need no caller's buffer
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, size_t(n_samples), 0, marg, lognorm,
                        [&](ResidentBatch &b) {
        if (b.n == 0) return int(GECCO_CRF_OK);  // (no labels, no run: a checked run lies inside a contig with genes)
        DeviceBlock<char> q;
        const size_t b_queries = align256(size_t(n_runs) * sizeof(RunQuery)), b_runs = size_t(n_runs) * size_t(n_samples) * 8;
        int rc = n_runs > 0 ? upload_queries(q, queries.data(), size_t(n_runs) * sizeof(RunQuery), b_queries + b_runs, "hipMalloc runs",
                                             "upload runs") : GECCO_CRF_OK;
        if (rc) return rc;
        int32_t *d_runs = n_runs > 0 ? reinterpret_cast<int32_t *>(q.get() + b_queries) : nullptr;
        rc = batch_wait(plan_run_sample_paths(b.plan, b.csr, n_samples, seed, reinterpret_cast<const RunQuery *>(q.get()), n_runs,
                                              b.out<int8_t>(1), d_runs, b.out<double>(0), b.out<double>(2), nullptr), "sampled paths");
        rc = batch_fetch(rc, y, b.out<int8_t>(1), size_t(b.n) * size_t(n_samples), "download paths");
        return batch_fetch(rc, runs, d_runs, b_runs, "download runs");
    });
    GECCO_GUARD_END
}

// ---- the K best label paths with their scores (ABI 2.18.0): the list Viterbi recursion behind gl_state, log Z from the
// whole-contig marginals pass (crf_kbest.hip)
GECCO_API int gecco_crf_viterbi_kbest(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                      const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                      const uint32_t *allowed, int32_t k, int8_t *y, double *score, int32_t *n_paths,
                                      double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the check of the call's own argument, on the host and before any device work
    if (k < 1 || k > kMaxKBest) return fail("viterbi_kbest: k = " + std::to_string(k) + " is outside 1 .. 32");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_contigs > 0 && (!score || !n_paths)) return fail("null buffer");
    if ((rc = check_output(contig_ptr, n_contigs, y))) return rc;
    const size_t K = size_t(k), nc = size_t(n_contigs);
    // per gene: the paths.  Per contig, behind log Z: k scores, the number of paths.  (The marginals are the pass's own output and
    // are not returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, K, K * 8 + 4, nullptr, lognorm,
                        [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: no path anywhere)
            for (size_t c = 0; c < nc; ++c) {
                n_paths[c] = 0;
                for (size_t r = 0; r < K; ++r) score[c * K + r] = -std::numeric_limits<double>::infinity();
            }
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_score = d_lognorm + nc;
        int32_t *d_n_paths = reinterpret_cast<int32_t *>(d_score + nc * K);
        DeviceBlock<char> ws;
        const size_t b_back = align256(kbest_back_bytes(b.n, m->m.L, k)), b_fin = kbest_fin_bytes(n_contigs, k);
        int rc = ws.alloc(b_back + b_fin, "hipMalloc k-best back-pointers");
        if (rc) return rc;
        uint16_t *d_back = reinterpret_cast<uint16_t *>(ws.get()), *d_fin = reinterpret_cast<uint16_t *>(ws.get() + b_back);
        rc = batch_wait(plan_run_viterbi_kbest(b.plan, b.csr, k, d_back, d_fin, b.out<int8_t>(1), d_score, d_n_paths, b.out<double>(0),
                                               d_lognorm, nullptr), "k-best paths");
        rc = batch_fetch(rc, y, b.out<int8_t>(1), size_t(b.n) * K, "download paths");
        rc = batch_fetch(rc, score, d_score, nc * K * 8, "download scores");
        return batch_fetch(rc, n_paths, d_n_paths, nc * 4, "download n_paths");
    });
    GECCO_GUARD_END
}

// ---- max-marginals (ABI 2.25.0): the score of the best whole-contig path through every (gene, label) pair, its maxima inside and
// outside label sets, and per span the best path that stays inside a set and the best one that leaves it, from a max-plus
// forward and backward walk behind gl_state; log Z, when asked for, from the whole-contig marginals pass (crf_maxmarg.hip,
// DESIGN.md §4.9p)
GECCO_API int gecco_crf_max_marginals(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                      const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                      const uint32_t *allowed, const uint32_t *set_mask, int32_t n_sets, const int32_t *span_contig,
                                      const int32_t *span_begin, const int32_t *span_end, const uint32_t *span_mask, int32_t n_spans,
                                      double *through, double *inside, double *outside, double *span_best, double *span_broken,
                                      double *best, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (n_sets < 0 || n_sets > kMaxMargSets) return fail("max_marginals: n_sets = " + std::to_string(n_sets) + " is outside 0 .. 32");
    if (n_sets > 0 && !set_mask) return fail("max_marginals: null buffer (set_mask)");
    for (int32_t s = 0; s < n_sets; ++s)
        if ((rc = check_label_set("max_marginals: set", s, set_mask[s], m->m.L))) return rc;
    if (n_sets == 0 && (inside || outside)) return fail("max_marginals: inside or outside given without a label set");
    if (n_spans < 0) return fail("max_marginals: negative number of spans");
    if (n_spans == 0 && (span_best || span_broken)) return fail("max_marginals: span_best or span_broken given without spans");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_contigs > 0 && !best) return fail("max_marginals: null buffer (best)");
    if (n_spans > 0 && (!span_contig || !span_begin || !span_end || !span_mask)) return fail("max_marginals: null buffer (spans)");
    std::vector<SpanQuery> spans(static_cast<size_t>(n_spans));
    for (int32_t q = 0; q < n_spans; ++q) {
        const int32_t c = span_contig[q], b = span_begin[q], e = span_end[q];
        int64_t len;
        if ((rc = check_query_contig("max_marginals: span", q, c, n_contigs, contig_ptr, &len))) return rc;
        if ((rc = check_query_range("max_marginals: span", q, c, b, e, len))) return rc;
        if ((rc = check_label_set("max_marginals: span", q, span_mask[q], m->m.L))) return rc;
        spans[size_t(q)] = SpanQuery{c, b, e, span_mask[q]};
    }
    const size_t nc = size_t(n_contigs), L = size_t(m->m.L), ns = size_t(n_sets);
    const size_t nq = (span_best || span_broken) ? size_t(n_spans) : 0;  // (spans without an output: nothing to walk)
    // per gene: through, inside, outside, each only when asked for.  Per contig, behind log Z: best.  (The marginals are the
    // pass's own output and are not returned; the pass runs only when lognorm is asked for.)
    const size_t per_gene = (through ? L * 8 : 0) + (inside ? ns * 8 : 0) + (outside ? ns * 8 : 0);
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, per_gene, 8, nullptr, lognorm,
                        [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: every contig's one path is the empty one -- gecco_crf_viterbi's score)
            for (size_t c = 0; c < nc; ++c) best[c] = 0.0;
            return int(GECCO_CRF_OK);
        }
        const size_t n = size_t(b.n);
        double *d_lognorm = b.out<double>(2), *d_best = d_lognorm + nc;
        MaxMargArgs a{};
        for (size_t s = 0; s < ns; ++s) a.set_mask[s] = set_mask[s];
        a.n_sets = n_sets;
        a.n_spans = int32_t(nq);
        double *at = b.out<double>(1);
        if (through) a.through = at, at += n * L;
        if (inside) a.inside = at, at += n * ns;
        if (outside) a.outside = at;
        a.best = d_best;
        // the walks' workspace, a block of its own (folded into the batch's block, a 32-label call with spans took 30 ms for 1.6:
        // profiles/MEASUREMENTS.md 7q)
        DeviceBlock<char> ws, q;
        const size_t b_half = align256(maxmarg_workspace_bytes(b.n, m->m.L) / 2);
        int rc = ws.alloc(2 * b_half, "hipMalloc max-marginal workspace");
        if (rc) return rc;
        a.fwd = reinterpret_cast<double *>(ws.get());
        a.bwd = reinterpret_cast<double *>(ws.get() + b_half);
        double *d_span_best = nullptr, *d_span_broken = nullptr;
        if (nq) {
            const size_t b_spans = align256(nq * sizeof(SpanQuery));
            if ((rc = upload_queries(q, spans.data(), nq * sizeof(SpanQuery), b_spans + 2 * nq * 8, "hipMalloc spans", "upload spans")))
                return rc;
            a.spans = reinterpret_cast<const SpanQuery *>(q.get());
            d_span_best = reinterpret_cast<double *>(q.get() + b_spans);
            d_span_broken = d_span_best + nq;
            a.span_best = span_best ? d_span_best : nullptr;
            a.span_broken = span_broken ? d_span_broken : nullptr;
        }
        rc = batch_wait(plan_run_max_marginals(b.plan, b.csr, a, b.out<double>(0), lognorm ? d_lognorm : nullptr, nullptr), "max-marginals");
        rc = batch_fetch(rc, through, a.through, n * L * 8, "download through");
        rc = batch_fetch(rc, inside, a.inside, n * ns * 8, "download inside");
        rc = batch_fetch(rc, outside, a.outside, n * ns * 8, "download outside");
        rc = batch_fetch(rc, span_best, d_span_best, nq * 8, "download span_best");
        rc = batch_fetch(rc, span_broken, d_span_broken, nq * 8, "download span_broken");
        return batch_fetch(rc, best, d_best, nc * 8, "download best");
    });
    GECCO_GUARD_END
}

// ---- decoding under a minimum run length (ABI 2.20.0): the best path among those whose every run of labels of a set has at
// least min_run genes, and the log-mass of all such paths, on a lattice expanded by a run counter behind gl_state; log Z from the
// whole-contig marginals pass (crf_minrun.hip)
GECCO_API int gecco_crf_viterbi_min_run(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                        const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                        const uint32_t *allowed, uint32_t set_mask, int32_t min_run, int8_t *y, double *score,
                                        double *lognorm_min_run, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (min_run < 1 || min_run > kMaxMinRun)
        return fail("viterbi_min_run: min_run = " + std::to_string(min_run) + " is outside 1 .. 32");
    if ((rc = check_label_set("set_mask", 0, set_mask, m->m.L))) return rc;
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_contigs > 0 && !score) return fail("null buffer");
    if ((rc = check_output(contig_ptr, n_contigs, y))) return rc;
    const size_t nc = size_t(n_contigs);
    // per gene: the path.  Per contig, behind log Z: the score, log Z_C.  (The marginals are the pass's own output and are not
    // returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 1, 16, nullptr, lognorm,
                        [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: every contig's one path is the empty one -- gecco_crf_viterbi's score, log Z_C = log Z = 0)
            for (size_t c = 0; c < nc; ++c) {
                score[c] = 0.0;
                if (lognorm_min_run) lognorm_min_run[c] = 0.0;
            }
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_score = d_lognorm + nc, *d_lognorm_mr = d_score + nc;
        DeviceBlock<char> ws;
        int rc = ws.alloc(minrun_back_bytes(b.n, m->m.L, min_run), "hipMalloc min-run back-pointers");
        if (rc) return rc;
        rc = batch_wait(plan_run_viterbi_min_run(b.plan, b.csr, set_mask, min_run, reinterpret_cast<uint8_t *>(ws.get()), b.out<int8_t>(1),
                                                 d_score, lognorm_min_run ? d_lognorm_mr : nullptr, b.out<double>(0), d_lognorm, nullptr),
                        "min-run decoding");
        rc = batch_fetch(rc, y, b.out<int8_t>(1), size_t(b.n), "download path");
        rc = batch_fetch(rc, score, d_score, nc * 8, "download score");
        return batch_fetch(rc, lognorm_min_run, d_lognorm_mr, nc * 8, "download lognorm_min_run");
    });
    GECCO_GUARD_END
}

// ---- marginals under a minimum run length (ABI 2.22.0): P(gene g has label j | x, no run of labels of the set is shorter than
// min_run) and its sum over the set, by a forward-backward on the run-counter lattice behind gl_state; log Z from the whole-contig
// marginals pass (crf_minrun.hip)
GECCO_API int gecco_crf_marginals_min_run(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                          const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                          const uint32_t *allowed, uint32_t set_mask, int32_t min_run, double *marg, double *inside,
                                          double *lognorm_min_run, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (min_run < 1 || min_run > kMaxMinRun)
        return fail("marginals_min_run: min_run = " + std::to_string(min_run) + " is outside 1 .. 32");
    if ((rc = check_label_set("marginals_min_run: set_mask", 0, set_mask, m->m.L))) return rc;
    if (!marg && !inside) return fail("marginals_min_run: marg and inside are both NULL");
    if (!lognorm_min_run) return fail("marginals_min_run: lognorm_min_run is NULL");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    const size_t nc = size_t(n_contigs), L = size_t(m->m.L);
    {  // a batch whose every contig is empty needs no device: log Z_C = log Z = 0, and nothing else is written
        bool empty = true;
        for (size_t c = 0; empty && c < nc; ++c) empty = contig_ptr[c + 1] == contig_ptr[c];
        if (empty) {
            for (size_t c = 0; c < nc; ++c) {
                lognorm_min_run[c] = 0.0;
                if (lognorm) lognorm[c] = 0.0;
            }
            return GECCO_CRF_OK;
        }
    }
    // per gene: inside, then (if asked for) the marginals under the constraint.  Per contig, behind log Z: log Z_C.  (The free
    // marginals are the pass's own output and are not returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 8 + (marg ? L * 8 : 0), 8, nullptr,
                        lognorm, [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: log Z_C = log Z = 0, and nothing else is written)
            for (size_t c = 0; c < nc; ++c) lognorm_min_run[c] = 0.0;
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_lognorm_mr = d_lognorm + nc;
        double *d_inside = b.out<double>(1), *d_marg = marg ? d_inside + size_t(b.n) : nullptr;
        DeviceBlock<char> ws;
        int rc = ws.alloc(minrun_forward_bytes(b.n, m->m.L, min_run), "hipMalloc min-run forward values");
        if (rc) return rc;
        rc = batch_wait(plan_run_marginals_min_run(b.plan, b.csr, set_mask, min_run, reinterpret_cast<double *>(ws.get()), d_marg,
                                                   inside ? d_inside : nullptr, d_lognorm_mr, b.out<double>(0), d_lognorm, nullptr),
                        "min-run marginals");
        rc = batch_fetch(rc, marg, d_marg, size_t(b.n) * L * 8, "download marginals under the constraint");
        rc = batch_fetch(rc, inside, d_inside, size_t(b.n) * 8, "download inside");
        return batch_fetch(rc, lognorm_min_run, d_lognorm_mr, nc * 8, "download lognorm_min_run");
    });
    GECCO_GUARD_END
}

// ---- circular contigs (ABI 2.28.0): every contig of the call is a ring whose last gene has a transition into its first; exact
// log Z, marginals and best path on the lattice expanded by the start label, behind gl_state (crf_ring.hip)
GECCO_API int gecco_crf_ring(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                             const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value, const uint32_t *allowed,
                             int8_t *y, double *score, double *marg, double *lognorm_ring) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (!lognorm_ring) return fail("ring: lognorm_ring is NULL");
    if (y && !score) return fail("ring: y given without score");
    if (score && !y) return fail("ring: score given without y");
    if (m->m.L > kGenMaxL) return fail("ring: num_labels = " + std::to_string(m->m.L) + " is above 32");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    const size_t nc = size_t(n_contigs), L = size_t(m->m.L);
    ResidentBatch b;
    b.plan.lattice = true;
    // per gene: the marginals and the path, each only when asked for.  Per contig: log Z of the ring, the score, the best start label.
    const size_t per_gene[2] = {marg ? L * 8 : 0, y ? size_t(1) : 0};
    rc = batch_open(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, attr_value != nullptr, allowed, allowed != nullptr, 1,
                    1, 1, false, per_gene, 24, b, true);  // (a mask of 0 is taken: that ring has no path)
    if (rc) return rc;
    if (b.n == 0) {  // (no genes: every ring's one path is the empty one -- log Z = 0 and gecco_crf_viterbi's score)
        for (size_t c = 0; c < nc; ++c) {
            lognorm_ring[c] = 0.0;
            if (score) score[c] = 0.0;
        }
        return GECCO_CRF_OK;
    }
    RingArgs q{};
    q.lognorm_ring = b.out<double>(2);
    q.marg = marg ? b.out<double>(0) : nullptr;
    // the walks' workspace, a block of its own: the forward values for the marginals, the back-pointers for the path
    DeviceBlock<char> ws;
    const size_t b_fwd = marg ? align256(ring_forward_bytes(b.n, m->m.L, n_contigs)) : 0, b_back = y ? ring_back_bytes(b.n, m->m.L) : 0;
    if (b_fwd + b_back && (rc = ws.alloc(b_fwd + b_back, "hipMalloc ring workspace"))) return rc;
    if (marg) q.fwd = reinterpret_cast<double *>(ws.get());
    if (y) {
        q.y = b.out<int8_t>(1);
        q.score = q.lognorm_ring + nc;
        q.start = reinterpret_cast<int32_t *>(q.score + nc);
        q.back = reinterpret_cast<uint8_t *>(ws.get() + b_fwd);
    }
    rc = batch_wait(plan_run_ring(b.plan, b.csr, q, nullptr), "ring");
    rc = batch_fetch(rc, marg, q.marg, size_t(b.n) * L * 8, "download ring marginals");
    rc = batch_fetch(rc, y, q.y, size_t(b.n), "download ring path");
    rc = batch_fetch(rc, score, q.score, nc * 8, "download ring score");
    return batch_fetch(rc, lognorm_ring, q.lognorm_ring, nc * 8, "download lognorm_ring");
    GECCO_GUARD_END
}

// ---- run-length potentials (ABI 2.27.0): a score g[min(n, M)] + tau max(n - M, 0) on every run of n genes with labels of a set,
// on the run-counter lattice behind gl_state: the best path and the log-mass under it, the marginals and the expected run-length
// counts; log Z from the whole-contig marginals pass (crf_runlength.hip)
namespace {
// the model arguments of the two entries, checked on the host: `who` is the entry's name
int check_run_length_model(const char *who, const gecco_crf_model *m, uint32_t set_mask, int32_t max_length, const double *length_score,
                           double tail, RunLengthScores &sc) {
    const std::string name(who);
    if (max_length < 1 || max_length > kMaxRunLength)
        return fail(name + ": max_length = " + std::to_string(max_length) + " is outside 1 .. 32");
    if (!length_score) return fail(name + ": length_score is NULL");
    sc = RunLengthScores{};
    for (int32_t d = 0; d < max_length; ++d) {
        if (!(length_score[d] < std::numeric_limits<double>::infinity()))
            return fail(name + ": length_score[" + std::to_string(d) + "] is NaN or +infinity (a score is finite or -infinity)");
        sc.g[d] = length_score[d];
    }
    if (!(tail < std::numeric_limits<double>::infinity())) return fail(name + ": tail is NaN or +infinity (a score is finite or -infinity)");
    sc.tau = tail;
    sc.M = max_length;
    return check_label_set((name + ": set_mask").c_str(), 0, set_mask, m->m.L);
}
}  // namespace

GECCO_API int gecco_crf_viterbi_run_length(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                           const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                           const uint32_t *allowed, uint32_t set_mask, int32_t max_length, const double *length_score,
                                           double tail, int8_t *y, double *score, double *lognorm_run_length, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    RunLengthScores sc;
    if ((rc = check_run_length_model("viterbi_run_length", m, set_mask, max_length, length_score, tail, sc))) return rc;
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    if (n_contigs > 0 && !score) return fail("viterbi_run_length: score is NULL");
    if (n_contigs > 0 && contig_ptr[n_contigs] > contig_ptr[0] && !y) return fail("viterbi_run_length: y is NULL");
    const size_t nc = size_t(n_contigs);
    // per gene: the path.  Per contig, behind log Z: the score, log Z_g.  (The marginals are the pass's own output and are not
    // returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 1, 16, nullptr, lognorm,
                        [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: every contig's one path is the empty one, which has no run -- log Z_g = log Z = 0)
            for (size_t c = 0; c < nc; ++c) {
                score[c] = 0.0;
                if (lognorm_run_length) lognorm_run_length[c] = 0.0;
            }
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_score = d_lognorm + nc, *d_lognorm_rl = d_score + nc;
        DeviceBlock<char> ws;
        int rc = ws.alloc(runlen_back_bytes(b.n, m->m.L, max_length), "hipMalloc run-length back-pointers");
        if (rc) return rc;
        rc = batch_wait(plan_run_viterbi_run_length(b.plan, b.csr, set_mask, sc, reinterpret_cast<uint8_t *>(ws.get()), b.out<int8_t>(1),
                                                    d_score, lognorm_run_length ? d_lognorm_rl : nullptr, b.out<double>(0), d_lognorm,
                                                    nullptr),
                        "run-length decoding");
        rc = batch_fetch(rc, y, b.out<int8_t>(1), size_t(b.n), "download path");
        rc = batch_fetch(rc, score, d_score, nc * 8, "download score");
        return batch_fetch(rc, lognorm_run_length, d_lognorm_rl, nc * 8, "download lognorm_run_length");
    });
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_marginals_run_length(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                             const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                             const uint32_t *allowed, uint32_t set_mask, int32_t max_length, const double *length_score,
                                             double tail, double *marg, double *inside, double *counts, double *lognorm_run_length,
                                             double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    RunLengthScores sc;
    if ((rc = check_run_length_model("marginals_run_length", m, set_mask, max_length, length_score, tail, sc))) return rc;
    if (!marg && !inside && !counts) return fail("marginals_run_length: marg, inside and counts are all NULL");
    if (!lognorm_run_length) return fail("marginals_run_length: lognorm_run_length is NULL");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    const size_t nc = size_t(n_contigs), L = size_t(m->m.L), M1 = size_t(max_length) + 1;
    const auto no_genes = [&] {  // log Z_g = log Z = 0, no run anywhere, and nothing else is written
        for (size_t c = 0; c < nc; ++c) lognorm_run_length[c] = 0.0;
        for (size_t k = 0; counts && k < nc * M1; ++k) counts[k] = 0.0;
    };
    {  // a batch whose every contig is empty needs no device
        bool empty = true;
        for (size_t c = 0; empty && c < nc; ++c) empty = contig_ptr[c + 1] == contig_ptr[c];
        if (empty) {
            no_genes();
            for (size_t c = 0; lognorm && c < nc; ++c) lognorm[c] = 0.0;
            return GECCO_CRF_OK;
        }
    }
    // per gene: inside, then (if asked for) the marginals under the length model.  Per contig, behind log Z: log Z_g, the counts.
    // (The free marginals are the pass's own output and are not returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 8 + (marg ? L * 8 : 0), 8 + M1 * 8,
                        nullptr, lognorm, [&](ResidentBatch &b) {
        if (b.n == 0) {
            no_genes();
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_lognorm_rl = d_lognorm + nc, *d_counts = d_lognorm_rl + nc;
        double *d_inside = b.out<double>(1), *d_marg = marg ? d_inside + size_t(b.n) : nullptr;
        DeviceBlock<char> ws;
        int rc = ws.alloc(runlen_forward_bytes(b.n, m->m.L, max_length), "hipMalloc run-length forward values");
        if (rc) return rc;
        rc = batch_wait(plan_run_marginals_run_length(b.plan, b.csr, set_mask, sc, reinterpret_cast<double *>(ws.get()), d_marg,
                                                      inside ? d_inside : nullptr, counts ? d_counts : nullptr, d_lognorm_rl,
                                                      b.out<double>(0), d_lognorm, nullptr),
                        "run-length marginals");
        rc = batch_fetch(rc, marg, d_marg, size_t(b.n) * L * 8, "download marginals under the length model");
        rc = batch_fetch(rc, inside, d_inside, size_t(b.n) * 8, "download inside");
        rc = batch_fetch(rc, counts, d_counts, nc * M1 * 8, "download counts");
        return batch_fetch(rc, lognorm_run_length, d_lognorm_rl, nc * 8, "download lognorm_run_length");
    });
    GECCO_GUARD_END
}

// ---- run counts (ABI 2.23.0): for k = 0 .. max_runs, the log-mass of the paths with exactly k runs of labels of a set (at
// k = max_runs: at least that many), and the best such path with its score, on a lattice expanded by a saturating run counter
// behind gl_state; log Z from the whole-contig marginals pass (crf_counts.hip)
GECCO_API int gecco_crf_run_counts(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                   const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value, const uint32_t *allowed,
                                   uint32_t set_mask, int32_t max_runs, double *log_mass, double *score, int8_t *y, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the call's own arguments, on the host and before any device work
    if (max_runs < 1 || max_runs > kMaxRunCounts)
        return fail("run_counts: max_runs = " + std::to_string(max_runs) + " is outside 1 .. 32");
    if ((rc = check_label_set("run_counts: set_mask", 0, set_mask, m->m.L))) return rc;
    if (y && !score) return fail("run_counts: y is given without score");
    if (!log_mass && !score) return fail("run_counts: log_mass, score and y are all NULL");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    const size_t nc = size_t(n_contigs), K1 = size_t(max_runs) + 1;
    const double ninf = -std::numeric_limits<double>::infinity();
    // per gene: the K + 1 paths, if asked for.  Per contig, behind log Z: K + 1 log-masses, K + 1 scores.  (The marginals are the
    // pass's own output and are not returned.)
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, score ? K1 : 0, 2 * K1 * 8, nullptr,
                        lognorm, [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: every contig's one path is the empty one, which has no run -- gecco_crf_viterbi's score)
            for (size_t i = 0; i < nc * K1; ++i) {
                if (log_mass) log_mass[i] = i % K1 ? ninf : 0.0;
                if (score) score[i] = i % K1 ? ninf : 0.0;
            }
            return int(GECCO_CRF_OK);
        }
        double *d_lognorm = b.out<double>(2), *d_mass = d_lognorm + nc, *d_score = d_mass + nc * K1;
        DeviceBlock<char> ws;
        int rc = score ? ws.alloc(counts_back_bytes(b.n, m->m.L, max_runs), "hipMalloc run-count back-pointers") : GECCO_CRF_OK;
        if (rc) return rc;
        rc = batch_wait(plan_run_run_counts(b.plan, b.csr, set_mask, max_runs, score ? reinterpret_cast<uint8_t *>(ws.get()) : nullptr,
                                            log_mass ? d_mass : nullptr, score ? d_score : nullptr,
                                            score ? b.out<int8_t>(1) : nullptr, b.out<double>(0), d_lognorm, nullptr),
                        "run counts");
        rc = batch_fetch(rc, log_mass, d_mass, nc * K1 * 8, "download log_mass");
        rc = batch_fetch(rc, score, d_score, nc * K1 * 8, "download score");
        return batch_fetch(rc, y, b.out<int8_t>(1), size_t(b.n) * K1, "download paths");
    });
    GECCO_GUARD_END
}

// ---- edge posteriors (ABI 2.19.0): the pairwise marginals of the whole-contig lattice, the probability that a run of labels of a
// set starts or ends at a gene, a contig's expected transition counts and its path entropy, all behind one forward-backward
// pass of the batch (crf_edges.hip)
GECCO_API int gecco_crf_edge_posteriors(const gecco_crf_model *m, int32_t device, const int32_t *contig_ptr, int32_t n_contigs,
                                        const int32_t *gene_ptr, const int32_t *attr_id, const double *attr_value,
                                        const uint32_t *allowed, const uint32_t *set_mask, int32_t n_sets, double *pair, double *enter,
                                        double *leave, double *transitions, double *entropy, double *marg, double *lognorm) {
    if (!m) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    int rc;
    // the checks of the sets, on the host and before any device work
    if (n_sets < 0 || n_sets > kMaxEdgeSets)
        return fail("edge_posteriors: n_sets = " + std::to_string(n_sets) + " is outside 1 .. 32 (0: no set, without enter and leave)");
    if (n_sets == 0 && (enter || leave)) return fail("edge_posteriors: enter and leave need a label set (n_sets = 0)");
    if (n_sets > 0 && !set_mask) return fail("null buffer");
    if ((rc = check_contig_ptr(contig_ptr, n_contigs))) return rc;
    EdgeQuery eq{};
    for (int32_t s = 0; s < n_sets; ++s) {
        if ((rc = check_label_set("set", s, set_mask[s], m->m.L))) return rc;
        eq.set_mask[s] = set_mask[s];
    }
    eq.n_sets = n_sets;
    const size_t L = size_t(m->m.L), nc = size_t(n_contigs), S = size_t(n_sets);
    return lattice_call(m, device, contig_ptr, n_contigs, gene_ptr, attr_id, attr_value, allowed, 0, 0, marg, lognorm, [&](ResidentBatch &b) {
        if (b.n == 0) {  // (no genes: no edge, no run, a path distribution of one empty path)
            for (size_t k = 0; transitions && k < nc * L * L; ++k) transitions[k] = 0.0;
            for (size_t c = 0; entropy && c < nc; ++c) entropy[c] = 0.0;
            return int(GECCO_CRF_OK);
        }
        // every contig's runs, counted from its own first gene
        std::vector<int32_t> run_ptr(nc + 1, 0);
        for (size_t c = 0; c < nc; ++c) run_ptr[c + 1] = run_ptr[c] + edge_run_count(int64_t(contig_ptr[c + 1]) - contig_ptr[c]);
        const size_t nr = size_t(run_ptr[nc]), n = size_t(b.n);
        std::vector<EdgeRun> runs(nr);
        for (size_t c = 0; c < nc; ++c)
            for (int32_t k = run_ptr[c]; k < run_ptr[c + 1]; ++k) runs[size_t(k)] = EdgeRun{int32_t(c), (k - run_ptr[c]) * kEdgeRunGenes};
        // one block: the two tables at its head, then the outputs that were asked for and the partials behind them
        Carver at;
        const size_t b_runs = nr * sizeof(EdgeRun), b_ptr = (nc + 1) * 4;
        const size_t o_runs = at.take(b_runs), o_ptr = at.take(b_ptr);
        const size_t o_pair = pair ? at.take(n * L * L * 8) : 0, o_enter = enter ? at.take(n * S * 8) : 0,
                     o_leave = leave ? at.take(n * S * 8) : 0, o_trans = transitions ? at.take(nc * L * L * 8) : 0,
                     o_npart = transitions ? at.take(nr * L * L * 8) : 0, o_ent = entropy ? at.take(nc * 8) : 0,
                     o_hpart = entropy ? at.take(nr * 8) : 0;
        DeviceBlock<char> d;
        int rc = d.alloc(at.off, "hipMalloc edge posteriors");
        if (!rc) rc = check_hip(hipMemcpy(d.get() + o_runs, runs.data(), b_runs, hipMemcpyHostToDevice), "upload runs");
        if (!rc) rc = check_hip(hipMemcpy(d.get() + o_ptr, run_ptr.data(), b_ptr, hipMemcpyHostToDevice), "upload run_ptr");
        if (rc) return rc;
        auto out = [&](bool wanted, size_t off) { return wanted ? reinterpret_cast<double *>(d.get() + off) : nullptr; };
        EdgeQuery q = eq;
        q.n_runs = int32_t(nr);
        q.runs = reinterpret_cast<const EdgeRun *>(d.get() + o_runs);
        q.run_ptr = reinterpret_cast<const int32_t *>(d.get() + o_ptr);
        q.pair = out(pair, o_pair);
        q.enter = out(enter, o_enter);
        q.leave = out(leave, o_leave);
        q.transitions = out(transitions, o_trans);
        q.npart = out(transitions, o_npart);
        q.entropy = out(entropy, o_ent);
        q.hpart = out(entropy, o_hpart);
        rc = batch_wait(plan_run_edge_posteriors(b.plan, b.csr, q, b.out<double>(0), b.out<double>(2), nullptr), "edge posteriors");
        rc = batch_fetch(rc, pair, q.pair, n * L * L * 8, "download pair");
        rc = batch_fetch(rc, enter, q.enter, n * S * 8, "download enter");
        rc = batch_fetch(rc, leave, q.leave, n * S * 8, "download leave");
        rc = batch_fetch(rc, transitions, q.transitions, nc * L * L * 8, "download transitions");
        return batch_fetch(rc, entropy, q.entropy, nc * 8, "download entropy");
    });
    GECCO_GUARD_END
}

namespace {
// grow-only scratch of the stand-alone segmenter / composition calls, one set per host thread
struct Scratch {
    DeviceScope home{DeviceScope::kLater};  // (first member: the block is freed with its device current)
    int device = -1;
    DeviceBlock<char> d;
    ~Scratch() { home.enter(device); }
    int reserve(int dev, size_t bytes) {
        if (d.get() && dev != device) {  // a block of another device: freed there
            DeviceScope there(device);
            d.release();
        }
        int rc = d.get() && bytes <= d.capacity() ? GECCO_CRF_OK : set_device(dev);
        if (rc || (rc = d.reserve(bytes, "hipMalloc scratch"))) return rc;
        device = dev;
        return GECCO_CRF_OK;
    }
};
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
}  // namespace

GECCO_API int gecco_crf_segment_ex(int32_t device, const double *p, const uint8_t *annotated, const int32_t *contig_ptr,
                                   int32_t n_contigs, const gecco_crf_refine_params *params, int32_t *seg_out, int32_t max_seg,
                                   int32_t *n_seg) {
    if (!params || !n_seg || n_contigs < 0 || (n_contigs > 0 && !contig_ptr) || max_seg < 0 || (max_seg > 0 && !seg_out)) {
        set_error("gecco_crf_segment: bad arguments");
        return GECCO_CRF_EINVAL;
    }
    *n_seg = 0;
    if (params->criterion != 0 && params->criterion != 1) {
        set_error("Unknown cluster filtering criterion");  // refine.py:165
        return GECCO_CRF_EINVAL;
    }
    int rc = check_device(device);
    if (rc) return rc;
    if (n_contigs == 0) return GECCO_CRF_OK;
    for (int32_t c = 0; c < n_contigs; ++c)
        if (contig_ptr[c + 1] < contig_ptr[c] || contig_ptr[0] != 0) {
            set_error("contig_ptr must start at 0 and be non-decreasing");
            return GECCO_CRF_EINVAL;
        }
    const size_t n = size_t(contig_ptr[n_contigs]), nc = size_t(n_contigs);
    if (n == 0) return GECCO_CRF_OK;
    if (!p || !annotated) {
        set_error("gecco_crf_segment: bad arguments");
        return GECCO_CRF_EINVAL;
    }
    SegParams sp = seg_params(*params);
    size_t nb = 0;
    if (sp.criterion == 1) {
        if (!sp.bio_ptr || sp.bio_ptr[0] != 0 || sp.bio_ptr[n] < 0 || (sp.bio_ptr[n] > 0 && !sp.bio_id)) {
            set_error("the antismash criterion needs the genes' marker domains (marker_ptr[0] = 0)");
            return GECCO_CRF_EINVAL;
        }
        for (size_t g = 0; g < n; ++g)
            if (sp.bio_ptr[g + 1] < sp.bio_ptr[g]) {
                set_error("marker_ptr must be non-decreasing");
                return GECCO_CRF_EINVAL;
            }
        nb = size_t(sp.bio_ptr[n]);
    }
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    static thread_local Scratch scratch;
    const size_t o_p = 0, o_a = o_p + al256(n * 8), o_c = o_a + al256(n + 8), o_seg = o_c + al256((nc + 1) * 4),
                 o_tot = o_seg + al256(size_t(max_seg) * 16 + 16), o_bp = o_tot + 256, o_bi = o_bp + al256((n + 1) * 4),
                 o_ws = o_bi + al256((nb + 4) * 4), bytes = o_ws + segment_workspace_bytes(int(n), n_contigs);
    if ((rc = scratch.reserve(device, bytes))) return rc;
    char *d = scratch.d.get();
    if ((rc = check_hip(hipMemcpy(d + o_p, p, n * 8, hipMemcpyHostToDevice), "H2D p"))) return rc;
    if ((rc = check_hip(hipMemcpy(d + o_a, annotated, n, hipMemcpyHostToDevice), "H2D annotated"))) return rc;
    if ((rc = check_hip(hipMemcpy(d + o_c, contig_ptr, (nc + 1) * 4, hipMemcpyHostToDevice), "H2D contig_ptr"))) return rc;
    if (sp.criterion == 1) {
        if ((rc = check_hip(hipMemcpy(d + o_bp, sp.bio_ptr, (n + 1) * 4, hipMemcpyHostToDevice), "H2D marker_ptr"))) return rc;
        if (nb && (rc = check_hip(hipMemcpy(d + o_bi, sp.bio_id, nb * 4, hipMemcpyHostToDevice), "H2D marker_id"))) return rc;
        sp.bio_ptr = reinterpret_cast<const int32_t *>(d + o_bp);
        sp.bio_id = reinterpret_cast<const int32_t *>(d + o_bi);
    }
    int32_t *d_seg = reinterpret_cast<int32_t *>(d + o_seg), *d_total = reinterpret_cast<int32_t *>(d + o_tot);
    if ((rc = check_hip(launch_segment(reinterpret_cast<const double *>(d + o_p), reinterpret_cast<const uint8_t *>(d + o_a), nullptr,
                                       reinterpret_cast<const int32_t *>(d + o_c), int(n), n_contigs, sp, d_seg, max_seg, nullptr,
                                       d_total, d + o_ws, nullptr),
                        "segment launch")))
        return rc;
    int32_t total = 0;
    if ((rc = check_hip(hipMemcpy(&total, d_total, 4, hipMemcpyDeviceToHost), "D2H count"))) return rc;
    *n_seg = total;
    if (total > max_seg) {
        set_error("gecco_crf_segment: seg_out too small");
        return GECCO_CRF_EINVAL;
    }
    if (total && (rc = check_hip(hipMemcpy(seg_out, d_seg, size_t(total) * 16, hipMemcpyDeviceToHost), "D2H segments")))
        return rc;
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_segment(int32_t device, const double *p, const uint8_t *annotated, const int32_t *contig_ptr,
                                int32_t n_contigs, double threshold, int32_t n_cds, int32_t edge_distance,
                                int32_t trim, int32_t carry_state, int32_t *seg_out, int32_t max_seg, int32_t *n_seg) {
    const gecco_crf_refine_params q = gecco_params(threshold, n_cds, edge_distance, trim, carry_state);
    return gecco_crf_segment_ex(device, p, annotated, contig_ptr, n_contigs, &q, seg_out, max_seg, n_seg);
}

GECCO_API int gecco_crf_plan_run_segment_ex(gecco_crf_plan *p, const double *d_p, const uint8_t *d_annotated,
                                            const gecco_crf_refine_params *params, int32_t *d_seg, int32_t max_seg,
                                            int32_t *d_n_seg, void *stream) {
    if (!p || !params) return GECCO_CRF_EINVAL;
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    return plan_run_segment(p->p, d_p, d_annotated, seg_params(*params), d_seg, max_seg, nullptr, d_n_seg,
                            static_cast<hipStream_t>(stream));
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_plan_run_segment(gecco_crf_plan *p, const double *d_p, const uint8_t *d_annotated, double threshold,
                                         int32_t n_cds, int32_t edge_distance, int32_t trim, int32_t carry_state,
                                         int32_t *d_seg, int32_t max_seg, int32_t *d_n_seg, void *stream) {
    const gecco_crf_refine_params q = gecco_params(threshold, n_cds, edge_distance, trim, carry_state);
    return gecco_crf_plan_run_segment_ex(p, d_p, d_annotated, &q, d_seg, max_seg, d_n_seg, stream);
}

GECCO_API int gecco_crf_domain_composition(int32_t device, const int32_t *seg, int32_t n_seg, const int32_t *dom_ptr,
                                           int32_t n_genes, const int32_t *dom_col, const double *dom_weight,
                                           int32_t n_cols, int32_t normalize, double *comp_out) {
    if (n_seg < 0 || n_genes < 0 || n_cols < 0 || (n_seg > 0 && (!seg || !dom_ptr || (n_cols > 0 && !comp_out)))) {
        set_error("gecco_crf_domain_composition: bad arguments");
        return GECCO_CRF_EINVAL;
    }
    int rc = check_device(device);
    if (rc) return rc;
    if (n_seg == 0 || n_cols == 0) return GECCO_CRF_OK;
    const size_t rows = size_t(dom_ptr[n_genes]);
    if (rows && (!dom_col || !dom_weight)) {
        set_error("gecco_crf_domain_composition: null domain arrays");
        return GECCO_CRF_EINVAL;
    }
    for (int32_t k = 0; k < n_seg; ++k) {
        const int32_t a = seg[4 * k + 2], b = seg[4 * k + 3];
        if (a < 0 || b < a || b > n_genes) {
            set_error("gecco_crf_domain_composition: segment outside the gene range");
            return GECCO_CRF_EINVAL;
        }
    }
    DeviceScope guard;
    GECCO_GUARD_BEGIN
    if ((rc = set_device(device))) return rc;
    DeviceBlock<int32_t> d_seg, d_ptr, d_col;
    DeviceBlock<double> d_w, d_tmp, d_out;
    const size_t out_n = size_t(n_seg) * size_t(n_cols);
    if ((rc = d_seg.alloc(size_t(n_seg) * 4, "hipMalloc segments"))) return rc;
    if ((rc = d_ptr.alloc(size_t(n_genes) + 1, "hipMalloc dom_ptr"))) return rc;
    if ((rc = d_col.alloc(rows, "hipMalloc dom_col"))) return rc;
    if ((rc = d_w.alloc(rows, "hipMalloc dom_weight"))) return rc;
    if ((rc = d_tmp.alloc(rows, "hipMalloc scratch"))) return rc;
    if ((rc = d_out.alloc(out_n, "hipMalloc compositions"))) return rc;
    if ((rc = check_hip(hipMemcpy(d_seg.get(), seg, size_t(n_seg) * 16, hipMemcpyHostToDevice), "H2D segments"))) return rc;
    if ((rc = check_hip(hipMemcpy(d_ptr.get(), dom_ptr, (size_t(n_genes) + 1) * 4, hipMemcpyHostToDevice), "H2D dom_ptr"))) return rc;
    if (rows && (rc = check_hip(hipMemcpy(d_col.get(), dom_col, rows * 4, hipMemcpyHostToDevice), "H2D dom_col"))) return rc;
    if (rows && (rc = check_hip(hipMemcpy(d_w.get(), dom_weight, rows * 8, hipMemcpyHostToDevice), "H2D dom_weight"))) return rc;
    if ((rc = check_hip(launch_composition(d_seg.get(), n_seg, d_ptr.get(), d_col.get(), d_w.get(), d_tmp.get(), n_cols, normalize ? 1 : 0,
                                           d_out.get(), nullptr), "composition launch")))
        return rc;
    return check_hip(hipMemcpy(comp_out, d_out.get(), out_n * 8, hipMemcpyDeviceToHost), "D2H compositions");
    GECCO_GUARD_END
}

// ---- columnar host side ---------------------------------------------------------------------------
GECCO_API int gecco_crf_pack_columns(const gecco_crf_model *m, const gecco_crf_table_columns *t, gecco_crf_packed **out) {
    if (!m || !t || !out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_packed> h(new gecco_crf_packed());
    int rc = pack_columns(m->m, *t, h->p);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API void gecco_crf_packed_free(gecco_crf_packed *p) { delete p; }
GECCO_API int gecco_crf_packed_info(const gecco_crf_packed *p, int32_t *n_genes, int32_t *n_contigs, int64_t *nnz,
                                    int32_t *n_duplicate_gene_ids, int32_t *n_unlisted_proteins, int32_t *pinned) {
    if (!p) return GECCO_CRF_EINVAL;
    if (n_genes) *n_genes = p->p.n_genes;
    if (n_contigs) *n_contigs = p->p.n_contigs;
    if (nnz) *nnz = p->p.nnz;
    if (n_duplicate_gene_ids) *n_duplicate_gene_ids = p->p.n_duplicate_gene_ids;
    if (n_unlisted_proteins) *n_unlisted_proteins = p->p.n_unlisted_proteins;
    if (pinned) *pinned = p->p.pinned ? 1 : 0;
    return GECCO_CRF_OK;
}
GECCO_API const int32_t *gecco_crf_packed_contig_ptr(const gecco_crf_packed *p) { return p ? p->p.contig_ptr : nullptr; }
GECCO_API const int32_t *gecco_crf_packed_gene_ptr(const gecco_crf_packed *p) { return p ? p->p.gene_ptr : nullptr; }
GECCO_API const int32_t *gecco_crf_packed_attr_id(const gecco_crf_packed *p) { return p ? p->p.attr_id : nullptr; }
GECCO_API const uint8_t *gecco_crf_packed_annotated(const gecco_crf_packed *p) { return p ? p->p.annotated : nullptr; }
GECCO_API const int64_t *gecco_crf_packed_gene_row(const gecco_crf_packed *p) { return p ? p->p.gene_row.data() : nullptr; }
GECCO_API const int32_t *gecco_crf_packed_row_gene(const gecco_crf_packed *p) { return p ? p->p.row_gene.data() : nullptr; }
GECCO_API const int64_t *gecco_crf_packed_row_order(const gecco_crf_packed *p) { return p ? p->p.row_order.data() : nullptr; }
GECCO_API const int64_t *gecco_crf_packed_row_ptr(const gecco_crf_packed *p) { return p ? p->p.row_ptr.data() : nullptr; }
GECCO_API const int32_t *gecco_crf_packed_marker_ptr(const gecco_crf_packed *p) { return p ? p->p.marker_ptr : nullptr; }
GECCO_API const int32_t *gecco_crf_packed_marker_id(const gecco_crf_packed *p) { return p ? p->p.marker_id : nullptr; }

GECCO_API int gecco_crf_cluster_rows_build(const gecco_crf_packed *p, const gecco_crf_table_columns *t, const int64_t *gene_end,
                                           const int64_t *feature_end, const int32_t *seg, int32_t n_seg, const double *seg_p,
                                           const int64_t *seg_off, gecco_crf_cluster_rows **out) {
    if (!p || !t || !out || n_seg < 0 || (n_seg > 0 && (!seg || !seg_p || !seg_off))) return GECCO_CRF_EINVAL;
    *out = nullptr;
    if ((t->n_genes > 0 && !gene_end) || (t->n_rows > 0 && !feature_end)) {
        set_error("cluster_rows: the tables' `end` columns are required");
        return GECCO_CRF_EINVAL;
    }
    GECCO_GUARD_BEGIN
    std::unique_ptr<gecco_crf_cluster_rows> h(new gecco_crf_cluster_rows());
    int rc = cluster_rows(p->p, *t, gene_end, feature_end, seg, n_seg, seg_p, seg_off, h->r);
    if (rc) return rc;
    *out = h.release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}
GECCO_API void gecco_crf_cluster_rows_free(gecco_crf_cluster_rows *r) { delete r; }
GECCO_API const int64_t *gecco_crf_cluster_rows_start(const gecco_crf_cluster_rows *r) { return r ? r->r.start.data() : nullptr; }
GECCO_API const int64_t *gecco_crf_cluster_rows_end(const gecco_crf_cluster_rows *r) { return r ? r->r.end.data() : nullptr; }
GECCO_API const double *gecco_crf_cluster_rows_average_p(const gecco_crf_cluster_rows *r) { return r ? r->r.average_p.data() : nullptr; }
GECCO_API const double *gecco_crf_cluster_rows_max_p(const gecco_crf_cluster_rows *r) { return r ? r->r.max_p.data() : nullptr; }
GECCO_API int gecco_crf_cluster_rows_strings(const gecco_crf_cluster_rows *r, int32_t which, const uint8_t **data,
                                             const int64_t **offsets) {
    if (!r || !data || !offsets || which < 0 || which > 3) return GECCO_CRF_EINVAL;
    const StrOut *c = which == 0 ? &r->r.sequence_id : which == 1 ? &r->r.cluster_id : which == 2 ? &r->r.proteins : &r->r.domains;
    *data = c->data.data();
    *offsets = c->offsets.data();
    return GECCO_CRF_OK;
}
GECCO_API double gecco_crf_exact_mean(const double *v, int64_t n) { return (v && n > 0) ? exact_mean(v, n) : std::nan(""); }
GECCO_API int gecco_crf_gather_f64(const double *src, int64_t n_src, const int32_t *idx, int64_t n, double *out) {
    if (n < 0 || n_src < 0 || (n > 0 && (!src || !idx || !out))) return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    return gather_f64(src, n_src, idx, n, out);
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_packed_order_info(const gecco_crf_packed *p, const int64_t *gene_start, const int64_t *gene_end, int64_t n_gene_rows,
                                          int32_t *rows_in_order, int32_t *refiner_order_differs) {
    if (!p || !rows_in_order || !refiner_order_differs || n_gene_rows < 0 || (p->p.n_genes > 0 && (!gene_start || !gene_end)))
        return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    return order_info(p->p, gene_start, gene_end, n_gene_rows, rows_in_order, refiner_order_differs);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_tsv_format(int64_t n_rows, int32_t n_cols, const int32_t *kinds, const void *const *data,
                                   const int64_t *const *offsets, const char *header, uint8_t **out, int64_t *out_len) {
    if (n_rows < 0 || n_cols < 0 || !out || !out_len || (n_cols > 0 && (!kinds || !data || !offsets))) return GECCO_CRF_EINVAL;
    *out = nullptr;
    *out_len = 0;
    for (int32_t c = 0; c < n_cols; ++c)
        if (kinds[c] < 0 || kinds[c] > 2 || (n_rows > 0 && !data[c]) || (kinds[c] == 0 && !offsets[c])) {
            set_error("tsv_format: bad column");
            return GECCO_CRF_EINVAL;
        }
    GECCO_GUARD_BEGIN
    return format_tsv(n_rows, n_cols, kinds, data, offsets, header, out, out_len);
    GECCO_GUARD_END
}
GECCO_API void gecco_crf_buffer_free(uint8_t *p) { std::free(p); }

// ---- training (ABI 2.3.0 lone, 2.5.0 batch, 2.8.0 grid) ---------------------------------------
// The three families are argument shapes of one Trainer (crf_train.hpp), and each opaque handle is that Trainer.
namespace {

Trainer *trainer_of(void *h) { return static_cast<Trainer *>(h); }
const Trainer *trainer_of(const void *h) { return static_cast<const Trainer *>(h); }

// trainer_create's arguments; `out` is not NULL.
template <class Handle>
int trainer_open(Handle **out, const char *family, int32_t device, int32_t n_sets, const int32_t *const *seq_ptr,
                 const int32_t *n_seqs, const int32_t *const *item_ptr, const int32_t *const *attr_id,
                 const int32_t *const *labels, const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                 const int32_t *step, const int32_t *const *state_fid, const int32_t *const *trans_fid,
                 const int32_t *num_features, int32_t n_problems, const int32_t *problem_set, int64_t scratch_budget_bytes) {
    DeviceScope guard;
    Trainer *t = nullptr;
    int rc = trainer_create(device, n_sets, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels, window, step,
                            state_fid, trans_fid, num_features, n_problems, problem_set, scratch_budget_bytes, family, &t);
    *out = reinterpret_cast<Handle *>(t);
    return rc;
}

int trainer_run(Trainer *t, const uint8_t *active, const double *const *w, double *f, double *const *g) {
    if (!t) return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    DeviceScope guard;
    return trainer_eval(t, active, w, f, g);
    GECCO_GUARD_END
}

void trainer_close(Trainer *t) {
    if (!t) return;
    DeviceScope guard;
    trainer_destroy(t);
}

}  // namespace

GECCO_API int gecco_crf_trainer_create(int32_t device, const int32_t *seq_ptr, int32_t n_seqs, const int32_t *item_ptr,
                                       const int32_t *attr_id, const int32_t *labels, int32_t num_attrs, int32_t num_labels,
                                       int32_t window, int32_t step, const int32_t *state_fid, const int32_t *trans_fid,
                                       int32_t num_features, gecco_crf_trainer **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    return trainer_open(out, nullptr, device, 1, &seq_ptr, &n_seqs, &item_ptr, &attr_id, &labels, &num_attrs, &num_labels,
                        &window, &step, &state_fid, &trans_fid, &num_features, 1, nullptr, 0);
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_trainer_eval(gecco_crf_trainer *t, const double *w, double *f, double *g) {
    const uint8_t active = 1;
    return trainer_run(trainer_of(t), &active, &w, f, &g);
}
GECCO_API int64_t gecco_crf_trainer_num_windows(const gecco_crf_trainer *t) { return trainer_num_windows(trainer_of(t), 0); }
GECCO_API void gecco_crf_trainer_free(gecco_crf_trainer *t) { trainer_close(trainer_of(t)); }

GECCO_API int gecco_crf_trainer_batch_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                             const int32_t *n_seqs, const int32_t *const *item_ptr,
                                             const int32_t *const *attr_id, const int32_t *const *labels,
                                             const int32_t *num_attrs, const int32_t *num_labels, int32_t window, int32_t step,
                                             const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                             const int32_t *num_features, gecco_crf_trainer_batch **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    if (n_problems < 1) return fail("trainer batch: at least one problem is needed");
    if (!seq_ptr || !n_seqs || !item_ptr || !attr_id || !labels || !num_attrs || !num_labels || !state_fid || !trans_fid ||
        !num_features)
        return fail("trainer batch: null argument");
    const std::vector<int32_t> windows(size_t(n_problems), window), steps(size_t(n_problems), step);
    return trainer_open(out, "batch", device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels,
                        windows.data(), steps.data(), state_fid, trans_fid, num_features, n_problems, nullptr, 0);
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_trainer_batch_eval(gecco_crf_trainer_batch *t, const uint8_t *active, const double *const *w, double *f,
                                           double *const *g) {
    return trainer_run(trainer_of(t), active, w, f, g);
}
GECCO_API int32_t gecco_crf_trainer_batch_num_problems(const gecco_crf_trainer_batch *t) {
    return trainer_num_problems(trainer_of(t));
}
GECCO_API int64_t gecco_crf_trainer_batch_num_windows(const gecco_crf_trainer_batch *t, int32_t k) {
    return trainer_num_windows(trainer_of(t), k);
}
GECCO_API void gecco_crf_trainer_batch_free(gecco_crf_trainer_batch *t) { trainer_close(trainer_of(t)); }

GECCO_API int gecco_crf_trainer_grid_create(int32_t device, int32_t n_sets, const int32_t *const *seq_ptr, const int32_t *n_seqs,
                                            const int32_t *const *item_ptr, const int32_t *const *attr_id,
                                            const int32_t *const *labels, const int32_t *num_attrs, const int32_t *num_labels,
                                            const int32_t *window, const int32_t *step, const int32_t *const *state_fid,
                                            const int32_t *const *trans_fid, const int32_t *num_features, int32_t n_problems,
                                            const int32_t *problem_set, int64_t scratch_budget_bytes,
                                            gecco_crf_trainer_grid **out) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    if (n_sets < 1) return fail("trainer grid: at least one set is needed");
    if (n_problems < 1) return fail("trainer grid: at least one problem is needed");
    if (!seq_ptr || !n_seqs || !item_ptr || !attr_id || !labels || !num_attrs || !num_labels || !window || !step ||
        !state_fid || !trans_fid || !num_features || !problem_set)
        return fail("trainer grid: null argument");
    return trainer_open(out, "grid", device, n_sets, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs, num_labels, window,
                        step, state_fid, trans_fid, num_features, n_problems, problem_set, scratch_budget_bytes);
    GECCO_GUARD_END
}
GECCO_API int gecco_crf_trainer_grid_eval(gecco_crf_trainer_grid *t, const uint8_t *active, const double *const *w, double *f,
                                          double *const *g) {
    return trainer_run(trainer_of(t), active, w, f, g);
}
GECCO_API int32_t gecco_crf_trainer_grid_num_problems(const gecco_crf_trainer_grid *t) {
    return trainer_num_problems(trainer_of(t));
}
GECCO_API int64_t gecco_crf_trainer_grid_num_windows(const gecco_crf_trainer_grid *t, int32_t k) {
    return trainer_num_windows(trainer_of(t), k);
}
GECCO_API int64_t gecco_crf_trainer_grid_scratch_bytes(const gecco_crf_trainer_grid *t, int32_t k) {
    return trainer_scratch_bytes(trainer_of(t), k);
}
GECCO_API void gecco_crf_trainer_grid_free(gecco_crf_trainer_grid *t) { trainer_close(trainer_of(t)); }

// ---- training with 2 to 32 labels (ABI 2.10.0), on windows or on whole sequences (2.12.0) ----
namespace {
// The two families of TrainerGeneral: `whole` has the sequences themselves as instances (no window, no step).
struct GeneralFamily {
    bool whole;
    const char *no_problem, *null_argument;
};
constexpr GeneralFamily kGeneralFamily{false, "trainer general: at least one problem is needed", "trainer general: null argument"};
constexpr GeneralFamily kSequencesFamily{true, "trainer sequences: at least one problem is needed",
                                         "trainer sequences: null argument"};

// The create of both families, with and without attribute values (`valued`: attr_value is required, ABI 2.13.0; its entry k
// holds the values of problem k's attribute entries, or NULL for a problem without), and with allowed-label sets (`partial`:
// allowed is required, ABI 2.14.0; its entry k holds one mask per item of problem k, or NULL for a labelled problem, and
// attr_value may then be NULL as a whole: no problem has values).
template <class Handle>
int general_open(Handle **out, const GeneralFamily &family, bool valued, int32_t device, int32_t n_problems,
                 const int32_t *const *seq_ptr, const int32_t *n_seqs, const int32_t *const *item_ptr,
                 const int32_t *const *attr_id, const double *const *attr_value, const int32_t *const *labels,
                 const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window, const int32_t *step,
                 const int32_t *const *state_fid, const int32_t *const *trans_fid, const int32_t *num_features,
                 bool partial = false, const uint32_t *const *allowed = nullptr, const double *const *seq_weight = nullptr,
                 const double *const *label_cost = nullptr) {
    if (!out) return GECCO_CRF_EINVAL;
    *out = nullptr;
    GECCO_GUARD_BEGIN
    if (n_problems < 1) return fail(family.no_problem);
    if (!seq_ptr || !n_seqs || !item_ptr || !attr_id || (valued && !attr_value) || (partial && !allowed) || !labels || !num_attrs || !num_labels ||
        (!family.whole && (!window || !step)) || !state_fid || !trans_fid || !num_features)
        return fail(family.null_argument);
    DeviceScope guard;
    TrainerGeneral *t = nullptr;
    const int rc = family.whole ? trainer_sequences_create(device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs,
                                                           num_labels, state_fid, trans_fid, num_features, &t, attr_value, allowed,
                                                           seq_weight, label_cost)
                                : trainer_general_create(device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, labels, num_attrs,
                                                         num_labels, window, step, state_fid, trans_fid, num_features, &t, attr_value,
                                                         allowed, seq_weight, label_cost);
    *out = reinterpret_cast<Handle *>(t);
    return rc;
    GECCO_GUARD_END
}
}  // namespace

GECCO_API int gecco_crf_trainer_general_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                               const int32_t *n_seqs, const int32_t *const *item_ptr,
                                               const int32_t *const *attr_id, const int32_t *const *labels,
                                               const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                                               const int32_t *step, const int32_t *const *state_fid,
                                               const int32_t *const *trans_fid, const int32_t *num_features,
                                               gecco_crf_trainer_general **out) {
    return general_open(out, kGeneralFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, nullptr, labels, num_attrs,
                        num_labels, window, step, state_fid, trans_fid, num_features);
}
GECCO_API int gecco_crf_trainer_general_create_valued(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                      const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                      const int32_t *const *attr_id, const double *const *attr_value,
                                                      const int32_t *const *labels, const int32_t *num_attrs,
                                                      const int32_t *num_labels, const int32_t *window, const int32_t *step,
                                                      const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                                      const int32_t *num_features, gecco_crf_trainer_general **out) {
    return general_open(out, kGeneralFamily, true, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, window, step, state_fid, trans_fid, num_features);
}
GECCO_API int gecco_crf_trainer_general_create_partial(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                       const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                       const int32_t *const *attr_id, const double *const *attr_value,
                                                       const int32_t *const *labels, const uint32_t *const *allowed,
                                                       const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                                                       const int32_t *step, const int32_t *const *state_fid,
                                                       const int32_t *const *trans_fid, const int32_t *num_features,
                                                       gecco_crf_trainer_general **out) {
    return general_open(out, kGeneralFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, window, step, state_fid, trans_fid, num_features, true, allowed);
}
// (attr_value, allowed, seq_weight and label_cost may each be NULL as a whole: no problem has them)
GECCO_API int gecco_crf_trainer_general_create_weighted(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                        const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                        const int32_t *const *attr_id, const double *const *attr_value,
                                                        const int32_t *const *labels, const uint32_t *const *allowed,
                                                        const double *const *seq_weight, const double *const *label_cost,
                                                        const int32_t *num_attrs, const int32_t *num_labels, const int32_t *window,
                                                        const int32_t *step, const int32_t *const *state_fid,
                                                        const int32_t *const *trans_fid, const int32_t *num_features,
                                                        gecco_crf_trainer_general **out) {
    return general_open(out, kGeneralFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, window, step, state_fid, trans_fid, num_features, false, allowed, seq_weight,
                        label_cost);
}
GECCO_API int gecco_crf_trainer_general_eval(gecco_crf_trainer_general *t, const uint8_t *active, const double *const *w,
                                             double *f, double *const *g) {
    if (!t) return GECCO_CRF_EINVAL;
    GECCO_GUARD_BEGIN
    DeviceScope guard;
    return trainer_general_eval(reinterpret_cast<TrainerGeneral *>(t), active, w, f, g);
    GECCO_GUARD_END
}
GECCO_API int32_t gecco_crf_trainer_general_num_problems(const gecco_crf_trainer_general *t) {
    return trainer_general_num_problems(reinterpret_cast<const TrainerGeneral *>(t));
}
GECCO_API int64_t gecco_crf_trainer_general_num_windows(const gecco_crf_trainer_general *t, int32_t k) {
    return trainer_general_num_windows(reinterpret_cast<const TrainerGeneral *>(t), k);
}
GECCO_API int64_t gecco_crf_trainer_general_scratch_bytes(const gecco_crf_trainer_general *t, int32_t k) {
    return trainer_general_scratch_bytes(reinterpret_cast<const TrainerGeneral *>(t), k);
}
GECCO_API void gecco_crf_trainer_general_free(gecco_crf_trainer_general *t) {
    if (!t) return;
    DeviceScope guard;
    trainer_general_destroy(reinterpret_cast<TrainerGeneral *>(t));
}

// ---- the whole-sequence family's handle is a TrainerGeneral whose problems have no window ---
GECCO_API int gecco_crf_trainer_sequences_create(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                 const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                 const int32_t *const *attr_id, const int32_t *const *labels,
                                                 const int32_t *num_attrs, const int32_t *num_labels,
                                                 const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                                 const int32_t *num_features, gecco_crf_trainer_sequences **out) {
    return general_open(out, kSequencesFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, nullptr, labels,
                        num_attrs, num_labels, nullptr, nullptr, state_fid, trans_fid, num_features);
}
GECCO_API int gecco_crf_trainer_sequences_create_valued(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                        const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                        const int32_t *const *attr_id, const double *const *attr_value,
                                                        const int32_t *const *labels, const int32_t *num_attrs,
                                                        const int32_t *num_labels, const int32_t *const *state_fid,
                                                        const int32_t *const *trans_fid, const int32_t *num_features,
                                                        gecco_crf_trainer_sequences **out) {
    return general_open(out, kSequencesFamily, true, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, nullptr, nullptr, state_fid, trans_fid, num_features);
}
GECCO_API int gecco_crf_trainer_sequences_create_partial(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                         const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                         const int32_t *const *attr_id, const double *const *attr_value,
                                                         const int32_t *const *labels, const uint32_t *const *allowed,
                                                         const int32_t *num_attrs, const int32_t *num_labels,
                                                         const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                                         const int32_t *num_features, gecco_crf_trainer_sequences **out) {
    return general_open(out, kSequencesFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, nullptr, nullptr, state_fid, trans_fid, num_features, true, allowed);
}
GECCO_API int gecco_crf_trainer_sequences_create_weighted(int32_t device, int32_t n_problems, const int32_t *const *seq_ptr,
                                                          const int32_t *n_seqs, const int32_t *const *item_ptr,
                                                          const int32_t *const *attr_id, const double *const *attr_value,
                                                          const int32_t *const *labels, const uint32_t *const *allowed,
                                                          const double *const *seq_weight, const double *const *label_cost,
                                                          const int32_t *num_attrs, const int32_t *num_labels,
                                                          const int32_t *const *state_fid, const int32_t *const *trans_fid,
                                                          const int32_t *num_features, gecco_crf_trainer_sequences **out) {
    return general_open(out, kSequencesFamily, false, device, n_problems, seq_ptr, n_seqs, item_ptr, attr_id, attr_value, labels,
                        num_attrs, num_labels, nullptr, nullptr, state_fid, trans_fid, num_features, false, allowed, seq_weight,
                        label_cost);
}
GECCO_API int gecco_crf_trainer_sequences_eval(gecco_crf_trainer_sequences *t, const uint8_t *active, const double *const *w,
                                               double *f, double *const *g) {
    return gecco_crf_trainer_general_eval(reinterpret_cast<gecco_crf_trainer_general *>(t), active, w, f, g);
}
GECCO_API int32_t gecco_crf_trainer_sequences_num_problems(const gecco_crf_trainer_sequences *t) {
    return trainer_general_num_problems(reinterpret_cast<const TrainerGeneral *>(t));
}
GECCO_API int64_t gecco_crf_trainer_sequences_num_sequences(const gecco_crf_trainer_sequences *t, int32_t k) {
    return trainer_general_num_windows(reinterpret_cast<const TrainerGeneral *>(t), k);  // (the instances of problem k)
}
GECCO_API int64_t gecco_crf_trainer_sequences_scratch_bytes(const gecco_crf_trainer_sequences *t, int32_t k) {
    return trainer_general_scratch_bytes(reinterpret_cast<const TrainerGeneral *>(t), k);
}
GECCO_API void gecco_crf_trainer_sequences_free(gecco_crf_trainer_sequences *t) {
    gecco_crf_trainer_general_free(reinterpret_cast<gecco_crf_trainer_general *>(t));
}

// ---- feature selection (ABI 2.4.0) ------------------------------------------------------------
GECCO_API int gecco_crf_fisher_exact(int32_t device, const int64_t *tables, int64_t n, double *pvalue) {
    GECCO_GUARD_BEGIN
    int rc = fisher_check(tables, n, pvalue);
    if (rc || n == 0) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceScope guard;
    return fisher_exact(device, tables, n, pvalue);
    GECCO_GUARD_END
}

// ---- interval join of genes and clusters (ABI 2.6.0) ------------------------------------------
GECCO_API int gecco_crf_cluster_overlaps(int32_t device, int32_t n_genes, const int32_t *gene_seq, const int64_t *gene_start,
                                         const int64_t *gene_end, int32_t n_seqs, const int32_t *cluster_ptr,
                                         const int64_t *cluster_start, const int64_t *cluster_end, uint8_t *label_out,
                                         int32_t *member_ptr_out, int32_t *member_gene_out, int64_t max_members,
                                         int64_t *n_members) {
    GECCO_GUARD_BEGIN
    int rc = overlaps_check(n_genes, gene_seq, gene_start, gene_end, n_seqs, cluster_ptr, cluster_start, cluster_end, label_out,
                            member_ptr_out, max_members, n_members);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceScope guard;
    return cluster_overlaps(device, n_genes, gene_seq, gene_start, gene_end, n_seqs, cluster_ptr, cluster_start, cluster_end,
                            label_out, member_ptr_out, member_gene_out, max_members, n_members);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_domain_composition_members(int32_t device, const int32_t *member_ptr, int32_t n_clusters,
                                                   const int32_t *member_gene, const int32_t *dom_ptr, int32_t n_genes,
                                                   const int32_t *dom_col, const double *dom_weight, int32_t n_cols,
                                                   int32_t normalize, double *comp_out) {
    GECCO_GUARD_BEGIN
    int rc = composition_members_check(member_ptr, n_clusters, member_gene, dom_ptr, n_genes, dom_col, dom_weight, n_cols,
                                       comp_out);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    if (n_clusters == 0 || n_cols == 0) return GECCO_CRF_OK;
    DeviceScope guard;
    return composition_members(device, member_ptr, n_clusters, member_gene, dom_ptr, n_genes, dom_col, dom_weight, n_cols,
                               normalize, comp_out);
    GECCO_GUARD_END
}

// ---- cluster type classifier (ABI 2.7.0; several forests at once 2.9.0) ----------------------------------------------------------
struct gecco_crf_forest {
    std::unique_ptr<Forest> f;
};

GECCO_API int gecco_crf_forest_fit(int32_t device, int32_t n_samples, int32_t n_features, const int32_t *col_ptr,
                                   const int32_t *row_idx, const float *values, int32_t n_outputs, const uint8_t *n_classes,
                                   const uint8_t *y, int32_t n_trees, const int32_t *sample_counts, const uint32_t *rand_state,
                                   int32_t max_features, gecco_crf_forest **out) {
    GECCO_GUARD_BEGIN
    if (!out) {
        set_error("gecco_crf_forest_fit: null out");
        return GECCO_CRF_EINVAL;
    }
    *out = nullptr;
    int rc = forest_fit_check(n_samples, n_features, col_ptr, row_idx, values, n_outputs, n_classes, y, n_trees, sample_counts,
                              rand_state, max_features);
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceScope guard;
    const ForestProblem p{n_samples, col_ptr, row_idx, values, n_classes, y, sample_counts, rand_state};
    std::vector<std::unique_ptr<Forest>> f;
    if ((rc = forest_fit_batch(device, 1, n_features, n_outputs, n_trees, max_features, &p, /*lone=*/true, &f))) return rc;
    *out = new gecco_crf_forest{std::move(f[0])};
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_forest_fit_batch(int32_t device, int32_t n_problems, int32_t n_features, int32_t n_outputs,
                                         int32_t n_trees, int32_t max_features, const int32_t *n_samples,
                                         const int32_t *const *col_ptr, const int32_t *const *row_idx,
                                         const float *const *values, const uint8_t *const *n_classes, const uint8_t *const *y,
                                         const int32_t *const *sample_counts, const uint32_t *const *rand_state,
                                         gecco_crf_forest **out) {
    GECCO_GUARD_BEGIN
    if (!out) {
        set_error("gecco_crf_forest_fit_batch: null out");
        return GECCO_CRF_EINVAL;
    }
    // (the range of n_problems is forest_fit_batch_check's to report: nothing is read or written past it here)
    const bool sized = n_problems >= 1 && n_problems <= kForestMaxProblems;
    for (int32_t k = 0; sized && k < n_problems; ++k) out[k] = nullptr;
    if (sized && (!n_samples || !col_ptr || !row_idx || !values || !n_classes || !y || !sample_counts || !rand_state)) {
        set_error("gecco_crf_forest_fit_batch: null buffer");
        return GECCO_CRF_EINVAL;
    }
    std::vector<ForestProblem> problems;
    for (int32_t k = 0; sized && k < n_problems; ++k)
        problems.push_back(ForestProblem{n_samples[k], col_ptr[k], row_idx[k], values[k], n_classes[k], y[k], sample_counts[k],
                                         rand_state[k]});
    int rc = forest_fit_batch_check(n_problems, n_features, n_outputs, n_trees, max_features, problems.data());
    if (rc) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceScope guard;
    std::vector<std::unique_ptr<Forest>> f;
    if ((rc = forest_fit_batch(device, n_problems, n_features, n_outputs, n_trees, max_features, problems.data(), /*lone=*/false,
                               &f)))
        return rc;
    std::vector<std::unique_ptr<gecco_crf_forest>> handles;  // (all of them, or none: an allocation may fail half way)
    handles.reserve(f.size());
    for (auto &forest : f) handles.emplace_back(new gecco_crf_forest{std::move(forest)});
    for (int32_t k = 0; k < n_problems; ++k) out[k] = handles[size_t(k)].release();
    return GECCO_CRF_OK;
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_forest_info(const gecco_crf_forest *h, int32_t *n_trees, int32_t *n_outputs, int32_t *max_n_classes,
                                    int32_t *node_count, int32_t *max_depth) {
    if (!h || !h->f) {
        set_error("gecco_crf_forest_info: null forest");
        return GECCO_CRF_EINVAL;
    }
    const Forest &f = *h->f;
    if (n_trees) *n_trees = f.n_trees;
    if (n_outputs) *n_outputs = f.n_outputs;
    if (max_n_classes) *max_n_classes = f.max_n_classes;
    for (int32_t t = 0; t < f.n_trees; ++t) {
        if (node_count) node_count[t] = f.node_count[size_t(t)];
        if (max_depth) max_depth[t] = f.max_depth[size_t(t)];
    }
    return GECCO_CRF_OK;
}

GECCO_API int gecco_crf_forest_export(const gecco_crf_forest *h, int32_t tree, int32_t *children_left, int32_t *children_right,
                                      int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                                      double *weighted_n_node_samples, double *value) {
    GECCO_GUARD_BEGIN
    if (!h || !h->f) {
        set_error("gecco_crf_forest_export: null forest");
        return GECCO_CRF_EINVAL;
    }
    DeviceScope guard;
    return forest_export(h->f.get(), tree, children_left, children_right, feature, threshold, impurity, n_node_samples,
                         weighted_n_node_samples, value);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_forest_predict(const gecco_crf_forest *h, int32_t n_rows, const double *x, double *posit) {
    GECCO_GUARD_BEGIN
    if (!h || !h->f) {
        set_error("gecco_crf_forest_predict: null forest");
        return GECCO_CRF_EINVAL;
    }
    if (n_rows < 0) {
        set_error("gecco_crf_forest_predict: n_rows must be >= 0");
        return GECCO_CRF_EINVAL;
    }
    if (n_rows == 0) return GECCO_CRF_OK;
    if (!x || !posit) {
        set_error("forest_predict: null buffer");
        return GECCO_CRF_EINVAL;
    }
    DeviceScope guard;
    const Forest *f = h->f.get();
    return forest_predict_batch(&f, 1, &n_rows, &x, &posit);
    GECCO_GUARD_END
}

GECCO_API int gecco_crf_forest_predict_batch(const gecco_crf_forest *const *h, int32_t n_problems, const int32_t *n_rows,
                                             const double *const *x, double *const *posit) {
    GECCO_GUARD_BEGIN
    std::vector<const Forest *> f;
    if (h && n_problems >= 1 && n_problems <= kForestMaxProblems)
        for (int32_t k = 0; k < n_problems; ++k) f.push_back(h[k] ? h[k]->f.get() : nullptr);
    int rc = forest_predict_batch_check(h ? f.data() : nullptr, n_problems, n_rows, x, posit);
    if (rc) return rc;
    DeviceScope guard;
    return forest_predict_batch(f.data(), n_problems, n_rows, x, posit);
    GECCO_GUARD_END
}

GECCO_API void gecco_crf_forest_free(gecco_crf_forest *h) {
    if (!h) return;
    DeviceScope guard;
    delete h;
}
