// ilupp_amd/csrc/api_ml.hip -- the multilevel preconditioner's handle (ilupp_ml; the struct itself: api_internal.h): its construction,
// single and batched, with the workers every batched construction of whole objects runs on (batch_build), its single applies, egress,
// and ilupp_hip_solve.  The batched applies of multilevel members: api_batch.hip.  (Host layer: api.hip; DESIGN_OTHER_PATHS.md 4h.13.)
#include "api_internal.h"

// ================================================================================================================================
// the multilevel ILU++ preconditioner without pivoting (include/ilupp_hip.h: ilupp_hip_ml_*).  Levels from ml.hip /
// piluc_df.hip; every level's two factors are an object of the ILUC kind (left by columns, right by rows, both unit), whose sweep
// kernels the apply borrows one half at a time: preconditioner_implementation.h:441-453 (left: all levels upwards) and :468-486
// (right: all levels downwards), each on the LAST n_level entries of the vector (sparse_implementation.h:4096-4165).
// ================================================================================================================================
// the live multilevel objects: a batched entry that is handed one in place of an ilupp_precond says so instead of reading it as one
namespace ilupp {
std::mutex g_ml_live_mu;
std::set<const void *> g_ml_live;
bool is_live_ml(const void *h) { std::lock_guard<std::mutex> lk(g_ml_live_mu); return g_ml_live.count(h) != 0; }
}  // namespace ilupp

namespace {

void ml_destroy(ilupp_ml *m)
{
    if (!m) return;
    // (the first level owns the stream the others borrow: it goes last)
    for (size_t k = m->obj.size(); k-- > 0;) if (m->obj[k]) destroy_obj(m->obj[k]);
    for (auto &l : m->dev) l.release();
    if (m->buf) (void)pool_free(m->buf);
    if (m->xdev) (void)pool_free(m->xdev);
    delete m;
}

static bool getenv_small_off() { static const bool off = getenv("ILUPP_NO_SMALL_SWEEPS") != nullptr; return off; }

// one half of the ILUC-kind apply (apply_plan, KIND_UTU): forward = the T2 loop (left factor, or right^T), backward = the T3 loop
int utu_half(ilupp_precond *p, bool forward, bool tr, double *rhs, double *out, int32_t *ticket)
{
    ensure_transposed(p);
    int32_t *err = p->ctrl;
    const ApplyPlan plan = apply_plan(KIND_UTU, tr, false, false);
    const SweepOp op = forward ? plan.first : plan.second;
    // small levels (the later, denser ones): one workgroup with the unknowns in LDS instead of a chain of hops through memory
    // (not for a factor with an empty row: p->degenerate objects keep the row-by-row kernel, which reports what it meets)
    // (up to 1 024 rows always; up to kSmallSweepMax = 4 096 when the rows are long -- more than 32 entries on average: there the general
    //  kernels' hop through memory per link of the dependency chain costs most.  Measured, apply of a whole object: 26 levels from n = 2 000,
    //  177 entries per row: 65 against 176 ms; 3 375 rows with 6 entries per row: 0.82 against 0.68 ms -- hence the second condition)
    const DevMat &M = sweep_parts(p, op).M;
    if ((p->n <= 1024 || (p->n <= kSmallSweepMax && M.nnz > 32 * (int64_t)p->n)) && !p->degenerate && !getenv_small_off())
        return sptrsv_small(p->stream, op.kind, M, rhs, out, err);
    return sweep(p, op, packed(p, op), rhs, out, ticket, err);
}

int ml_create_common(const DevMat &A, const ilupp_ml_params *ip, ilupp_ml **out)
{
    MlParams P;
    P.threshold = ip->threshold;
    P.n_pre = ip->n_preprocessing;
    if (P.n_pre < 0 || P.n_pre > 8) { set_error("ILU++: at most 8 preprocessing steps"); return ILUPP_ERR_INVALID; }
    for (int i = 0; i < P.n_pre; ++i) P.pre[i] = ip->preprocessing[i];
    P.pq_threshold = ip->pq_threshold; P.max_levels = ip->max_levels; P.min_ml_size = ip->min_ml_size;
    P.pil.small_pivot_terminates = ip->small_pivot_terminates != 0; P.pil.min_pivot = ip->min_pivot; P.pil.min_elim_factor = ip->min_elim_factor;
    P.pil.threshold_shift_schur = ip->threshold_shift_schur; P.vary_threshold_factor = ip->vary_threshold_factor;
    P.use_final_threshold = ip->use_final_threshold != 0; P.final_threshold = ip->final_threshold;
    P.pil.max_fill_in = ip->max_fill_in > 0 ? ip->max_fill_in : 0;
    P.pil.rules = ip->drop_rules; P.pil.combine = ip->combine_factor; P.pil.scale_invdiag = ip->scale_weight_invdiag != 0;
    P.pil.wgt[0] = ip->weight_standard_drop; P.pil.wgt[1] = ip->weight_standard_drop2; P.pil.wgt[2] = ip->weight_err_prop_drop;
    P.pil.wgt[3] = ip->weight_err_prop_drop2; P.pil.wgt[4] = ip->weight_pivot_drop; P.pil.wgt[5] = ip->weight_inverse_drop;
    P.pil.wgt[6] = ip->weight_weighted_drop; P.pil.init_weights_lu = ip->init_weights_lu;
    P.pil.neutral = ip->neutral_element; P.pil.min_weight = ip->min_weight;
    P.pil.piv_tol = ip->piv_tol; P.pil.permute_rows = ip->permute_rows; P.pil.total_piv = ip->total_piv; P.pil.begin_total_piv = ip->begin_total_piv != 0;
    P.pil.final_row_crit = ip->final_row_crit; P.pil.move_level_factor = ip->move_level_factor; P.pil.row_u_max = ip->row_u_max;
    if (P.pil.permute_rows < 0 || P.pil.permute_rows > 3 || P.pil.total_piv < 0 || P.pil.total_piv > 2) { set_error("ILU++: PERMUTE_ROWS / TOTAL_PIV out of range"); return ILUPP_ERR_INVALID; }
    if (P.pil.pivoting() && (P.pil.final_row_crit < -1 || P.pil.final_row_crit > 9)) {
        set_error("ILU++: FINAL_ROW_CRIT " + std::to_string(P.pil.final_row_crit) + " (rows ordered by weights instead of counts) is not built");
        return ILUPP_ERR_UNSUPPORTED;
    }
    if ((P.pil.rules & ~255) != 0) { set_error("ILU++: unknown dropping rule"); return ILUPP_ERR_INVALID; }
    // (inverse-based and weighted dropping -- recurrences over all steps -- run as chains in both factorisations: pilucdp.hip)
    struct MlGuard { ilupp_ml *m; ~MlGuard() { if (m) ml_destroy(m); } } g{new ilupp_ml()};
    ilupp_ml *m = g.m;
    m->n = A.n;
    // the first level's object owns the stream everything runs on
    ilupp_precond *p0 = new_obj(A.n);
    m->obj.push_back(p0);
    hipStream_t st = p0->stream;
    ILUPP_HIP(hipEventRecord(p0->ev[0], st));
    int rc = ml_build(st, A, P, &m->dev, &m->kernel_ms);
    if (rc) return rc;
    ILUPP_HIP(pool_malloc(&m->buf, sizeof(double) * (size_t)A.n));
    for (size_t k = 0; k < m->dev.size(); ++k) {
        MlLevelDev &l = m->dev[k];
        ilupp_precond *p = p0;
        if (k > 0) {
            p = new_obj(l.n);
            m->obj.push_back(p);
            queue_give(*p);                                    // its own queue back to the pool: the level works on the first level's
            static_cast<QueuePack &>(*p) = *p0;
            p->side = nullptr; p->jev[0] = p->jev[1] = nullptr;
            p->borrowed_queue = true;
        }
        p->kind = KIND_UTU; p->nnz_mode = NNZ_GENERIC_LU; p->input_csc = false;
        p->Lc = l.L; p->Uc = l.U;
        l.L = DevMat(); l.U = DevMat();                        // (the object owns the arrays now)
        utu_analyse(p);
    }
    ILUPP_HIP(hipEventRecord(p0->ev[1], st));
    ILUPP_HIP(stream_sync(st));
    ILUPP_HIP(hipEventElapsedTime(&m->construct_ms, p0->ev[0], p0->ev[1]));
    *out = m;
    g.m = nullptr;
    return ILUPP_OK;
}

}  // namespace

namespace ilupp {

int ml_apply_dev(ilupp_ml *m, double *x, int transpose, int part)       // part: 0 = both passes, 1 = the first only, 2 = the second only
{
    ilupp_precond *p0 = m->obj[0];
    hipStream_t st = p0->stream;
    const int nl = (int)m->obj.size();
    // (a batched launch that was not waited for still reads the levels and writes m->buf: ilupp_hip_ml_apply_batch_device)
    if (p0->batch_ev) {
        ILUPP_HIP(hipStreamWaitEvent(st, p0->batch_ev, 0));
        for (int i = 0; i < nl; ++i) m->obj[(size_t)i]->batch_ev = nullptr;
    }
    order_after_caller(st, p0->sev[0]);
    for (int i = 0; i < nl; ++i) ILUPP_HIP(hipMemsetAsync(m->obj[(size_t)i]->ctrl, 0, 64, st));
    ILUPP_HIP(hipEventRecord(p0->ev[0], st));
    const bool tr = transpose != 0;
    // first pass upwards through the levels, second pass downwards (:103-111 with :441-453, :468-486)
    for (int pass = 0; pass < 2; ++pass) {
        if (part != 0 && part != pass + 1) continue;
        for (int s = 0; s < nl; ++s) {
            const int i = pass == 0 ? s : nl - 1 - s;
            ilupp_precond *p = m->obj[(size_t)i];
            const MlLevelDev &l = m->dev[(size_t)i];
            double *xt = x + (m->n - l.n);
            int rc = ILUPP_OK;
            if (!tr && pass == 0) {            // left, ID: x /= D_l; permute_first(perm_rows); T2(L)
                ml_scale_perm(st, l.n, xt, l.Dl, l.pr, m->buf);
                rc = utu_half(p, true, false, m->buf, p->work, p->ctrl + 4);
                if (!rc) ml_take(st, l.n, p->work, nullptr, xt);
            } else if (!tr) {                  // right, ID: x *= D; T3(U); permute_last(inverse_perm_columns); x /= D_r
                ml_scale(st, l.n, xt, l.D, m->buf);
                rc = utu_half(p, false, false, m->buf, p->work, p->ctrl + 5);
                if (!rc) {
                    ml_perm_scale(st, l.n, p->work, l.ipc, l.Dr, xt);
                    fill_u64(st, reinterpret_cast<unsigned long long *>(p->work), l.n, kSentinel);
                }
            } else if (pass == 0) {            // right, TRANSPOSE: x /= D_r; permute_first(perm_columns); T2(U^T); x *= D
                ml_scale_perm(st, l.n, xt, l.Dr, l.pc, m->buf);
                rc = utu_half(p, true, true, m->buf, p->work, p->ctrl + 4);
                if (!rc) ml_take(st, l.n, p->work, l.D, xt);
            } else {                           // left, TRANSPOSE: T3(L^T); permute_last(inverse_perm_rows); x /= D_l
                ILUPP_HIP(hipMemcpyAsync(m->buf, xt, sizeof(double) * (size_t)l.n, hipMemcpyDeviceToDevice, st));
                rc = utu_half(p, false, true, m->buf, p->work, p->ctrl + 5);
                if (!rc) {
                    ml_perm_scale(st, l.n, p->work, l.ipr, l.Dl, xt);
                    fill_u64(st, reinterpret_cast<unsigned long long *>(p->work), l.n, kSentinel);
                }
            }
            if (rc) return rc;
        }
    }
    ILUPP_HIP(hipEventRecord(p0->ev[2], st));
    return ILUPP_OK;
}

int ml_finish_apply(ilupp_ml *m)
{
    ilupp_precond *p0 = m->obj[0];
    const int nl = (int)m->obj.size();
    std::vector<int32_t> err((size_t)nl, 0);
    for (int i = 0; i < nl; ++i) ILUPP_HIP(hipMemcpyAsync(&err[(size_t)i], m->obj[(size_t)i]->ctrl, sizeof(int32_t), hipMemcpyDeviceToHost, p0->stream));
    ILUPP_HIP(stream_sync(p0->stream));
    ILUPP_HIP(hipEventElapsedTime(&m->last_apply_ms, p0->ev[0], p0->ev[2]));
    for (int i = 0; i < nl; ++i)
        if (err[(size_t)i]) {
            for (int j = 0; j < nl; ++j) fill_u64(p0->stream, reinterpret_cast<unsigned long long *>(m->obj[(size_t)j]->work), m->obj[(size_t)j]->n, kSentinel);
            ILUPP_HIP(stream_sync(p0->stream));
            set_error("triangular solve: dependency wait timed out (factor not triangular?)");
            return ILUPP_ERR_TIMEOUT;
        }
    return ILUPP_OK;
}

// a batched construction that gets no stream to run on
int no_batch_stream() { set_error("batched construction: no stream"); return ILUPP_ERR_HIP; }

// how a batched construction went, for every kind of batch: the members' codes into the caller's array, if it gave one, and the first
// failure returned and named by its number
int batch_first_failure(int32_t count, const std::vector<int> &rcs, const std::vector<std::string> &msgs, int32_t *status)
{
    int first = ILUPP_OK;
    for (int32_t i = 0; i < count; ++i) {
        if (status) status[i] = rcs[(size_t)i];
        if (rcs[(size_t)i] && !first) { first = rcs[(size_t)i]; set_error("matrix " + std::to_string(i) + " of the batch: " + msgs[(size_t)i]); }
    }
    return first;
}

// The workers of a batched construction (ilupp_hip_ml_create_batch, ilupp_hip_ilucp_create_batch, ilupp_hip_ilutp_create_batch): `build(i)`
// constructs member i on the calling worker's thread and returns its code; `worst_bytes` is the device memory the largest member holds
// while it is built.  At most 64 workers (ILUPP_BATCH_WORKERS, read per call) and as many as the memory takes: 0.6 of the free bytes, the
// pool's kept blocks counted as free.  Every worker is a member of one ChainBatch, so the sequential chains of the members it builds are
// launched together with the other workers' (pilucdp.hip).  Members are independent: status[i] per member (may be null), the first
// failure is returned and reported as "matrix i of the batch: ...".  The caller holds the build lock.
int batch_build(int32_t count, double worst_bytes, int32_t *status, const std::function<int(int32_t)> &build)
{
    int workers = 64;
    if (const char *e = getenv("ILUPP_BATCH_WORKERS")) { const int v = atoi(e); if (v > 0) workers = v; }
    if (workers > count) workers = count;
    int device = 0;
    ILUPP_HIP(hipGetDevice(&device));
    {
        size_t free_b = 0, total_b = 0;
        ILUPP_HIP(hipMemGetInfo(&free_b, &total_b));
        free_b += pool_cached_bytes();
        if (worst_bytes > 0.0) { const double fit = 0.6 * (double)free_b / worst_bytes; if (fit < (double)workers) workers = fit < 1.0 ? 1 : (int)fit; }
    }
    ChainBatch *cb = chain_batch_create(workers);
    if (!cb) return no_batch_stream();
    // (the batch and its stream go when this call unwinds, whatever throws below)
    struct BatchGuard { ChainBatch *b; ~BatchGuard() { if (b) chain_batch_destroy(b); } } cbg{cb};
    std::vector<int> rcs((size_t)count, ILUPP_OK);
    std::vector<std::string> msgs((size_t)count);
    std::atomic<int32_t> next(0);
    auto work = [&](int w) {
        (void)hipSetDevice(device);
        pool_set_owner(w + 1);
        chain_batch_enter(cb);
        for (;;) {
            const int32_t i = next.fetch_add(1);
            if (i >= count) break;
            int rc;
            try { rc = build(i); }
            catch (const ilupp::HipError &e) { ilupp::d2h_cancel_all(); rc = ilupp::report(e); }
            catch (const std::bad_alloc &) { ilupp::set_error("out of host memory"); rc = ILUPP_ERR_MEMORY; }
            catch (...) { ilupp::set_error("unexpected exception in a batch worker"); rc = ILUPP_ERR_HIP; }     // (a worker must reach chain_batch_leave)
            rcs[(size_t)i] = rc;
            if (rc) msgs[(size_t)i] = ilupp::g_last_error;
        }
        chain_batch_leave(cb);
        (void)hipDeviceSynchronize();                          // (everything this worker queued is done: its kept blocks are everybody's)
        pool_disown(w + 1);
        pool_set_owner(0);
    };
    // Kept blocks of owner 0 may have been given back by calls on other objects' streams (apply temporaries, destroy) without a wait for
    // those streams: nothing of that may still be queued when up to 64 fresh streams start to take such blocks (pool.h).
    ILUPP_HIP(hipDeviceSynchronize());
    {
        // (threads that were started are joined whatever happens -- a joinable std::thread that is destroyed ends the process --, and
        // workers that could not be started are taken out of the batch's count, or the others would wait for their launches for good)
        struct Joiner { std::vector<std::thread> v; ~Joiner() { for (std::thread &t : v) if (t.joinable()) t.join(); } } pool_threads;
        int started = 1;
        try {
            for (int w = 1; w < workers; ++w) { pool_threads.v.emplace_back(work, w); ++started; }
        } catch (...) {
            for (int w = started; w < workers; ++w) { chain_batch_enter(cb); chain_batch_leave(cb); }
        }
        work(0);
    }
    chain_batch_destroy(cbg.b); cbg.b = nullptr;
    return batch_first_failure(count, rcs, msgs, status);
}

}  // namespace ilupp

extern "C" {

void ilupp_hip_ml_default_params(ilupp_ml_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 0.0;
    p->n_preprocessing = 3;
    p->preprocessing[0] = ILUPP_PRE_NORMALIZE_COLUMNS; p->preprocessing[1] = ILUPP_PRE_NORMALIZE_ROWS; p->preprocessing[2] = ILUPP_PRE_PQ_ORDERING;
    p->pq_threshold = 0.0; p->max_levels = 100; p->min_ml_size = 0;
    p->small_pivot_terminates = 1; p->min_pivot = 1e-2; p->min_elim_factor = 0.0; p->threshold_shift_schur = 0.0;
    p->vary_threshold_factor = 1.0; p->use_final_threshold = 0; p->final_threshold = 0.0;
    p->max_fill_in = 0;
    p->drop_rules = ILUPP_DROP_ERR_PROP;
    p->weight_standard_drop = p->weight_standard_drop2 = p->weight_err_prop_drop = p->weight_err_prop_drop2 = p->weight_pivot_drop = 1.0;
    p->weight_inverse_drop = 1.0; p->weight_weighted_drop = 1.0; p->init_weights_lu = 1.0;
    p->combine_factor = 0; p->neutral_element = 0.0; p->min_weight = 1.0; p->scale_weight_invdiag = 0;
    p->piv_tol = 0.0; p->permute_rows = 0; p->total_piv = 0; p->begin_total_piv = 1;        // (init case 10, :927-934)
    p->final_row_crit = -1; p->move_level_factor = 2.0; p->row_u_max = 1.5;
}

int ilupp_hip_ml_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const ilupp_ml_params *params,
                        ilupp_ml **out)
{
    return create_from_host(data, indices, indptr, n, is_csr != 0, out, [&](DevMat &A) { return ml_create_common(A, params, out); },
                            params != nullptr, "null argument");
}

int ilupp_hip_ml_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr, const int32_t *n,
                              int is_csr, const ilupp_ml_params *params, ilupp_ml **out, int32_t *status)
{
    API_TRY_BUILD
    if (count < 0 || !data || !indices || !indptr || !n || !params || !out) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) { out[i] = nullptr; if (status) status[i] = ILUPP_OK; }
    if (count == 0) return ILUPP_OK;
    // a construction with pivoting holds ~116 bytes per entry + 450 per row (two stores with their link arrays, the Schur store, both
    // orientations of the level's matrix, the tables)
    double worst = 0.0;
    for (int32_t i = 0; i < count; ++i)
        if (indptr[i] && n[i] > 0) { const double e = 116.0 * (double)indptr[i][n[i]] + 450.0 * (double)n[i] + (double)(64 << 20); if (e > worst) worst = e; }
    return batch_build(count, worst, status, [&](int32_t i) {
        MatGuard A;
        const int rc = upload(data[i], indices[i], indptr[i], n[i], is_csr != 0, &A.m);
        return rc ? rc : ml_create_common(A.m, params, &out[i]);
    });
    API_CATCH
}

int ilupp_hip_ml_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int is_csr,
                               const ilupp_ml_params *params, ilupp_ml **out)
{
    return create_from_device(d_data, d_indices, d_indptr, n, is_csr != 0, out, [&](DevMat &A) { return ml_create_common(A, params, out); },
                              params != nullptr, "null argument");
}

void ilupp_hip_ml_destroy(ilupp_ml *p)
{
    try { ml_destroy(p); } catch (...) {}
}

int ilupp_hip_ml_apply_device(ilupp_ml *m, double *d_x, int64_t len, int transpose, int sync)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    OR_RETURN(ml_apply_dev(m, d_x, transpose));
    return finish_or_hand_over(sync, *m->obj[0], [&] { return ml_finish_apply(m); });
    API_CATCH
}

int ilupp_hip_ml_apply_part_device(ilupp_ml *m, double *d_x, int64_t len, int transpose, int left, int sync)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    // ID: the left part is the first pass (upwards through the levels), the right part the second; TRANSPOSE: right^T first, then left^T
    const int part = (left != 0) == (transpose == 0) ? 1 : 2;
    OR_RETURN(ml_apply_dev(m, d_x, transpose, part));
    return finish_or_hand_over(sync, *m->obj[0], [&] { return ml_finish_apply(m); });
    API_CATCH
}

int ilupp_hip_ml_apply(ilupp_ml *m, double *x, int64_t len, int transpose)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    return apply_staged(m->obj[0]->stream, &m->xdev, m->n, x,
                        [&](double *d) { return ml_apply_dev(m, d, transpose); },
                        [&] { return ml_finish_apply(m); });
    API_CATCH
}

namespace {
// the matrix of a solve in HBM and its preconditioner (the caller holds the construction lock)
int solve_build(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const ilupp_ml_params *params, DevMat *A,
                ilupp_ml **m)
{
    API_TRY
    const int rc = upload(data, indices, indptr, n, is_csr != 0, A);
    if (rc) return rc;
    return ml_create_common(*A, params, m);
    API_CATCH
}
}  // namespace

int ilupp_hip_solve(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const double *rhs, int64_t rhs_len,
                    double rtol, double atol, int32_t max_iter, const ilupp_ml_params *params, double *x, int32_t *iterations, double *rel_reached,
                    double *abs_reached)
{
    if (!data || !indices || !indptr || !rhs || !params || !x) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
    if (rhs_len != n) { set_error("right-hand side has wrong size!"); return ILUPP_ERR_WRONG_SIZE; }            // binding.cpp:209-210
    // (the whole call under the construction lock: the iteration takes and returns pool blocks on its own stream, and the pool knows nothing
    //  of streams -- see API_TRY_BUILD)
    std::lock_guard<std::mutex> build_lock_(ilupp::g_build_mu);
    struct Guard {
        DevMat A, T; ilupp_ml *m = nullptr;
        ~Guard() { try { if (m) { (void)hipStreamSynchronize(m->obj[0]->stream); ml_destroy(m); } } catch (...) {} A.release(); T.release(); }
    } g;
    { const int rc = solve_build(data, indices, indptr, n, is_csr, params, &g.A, &g.m); if (rc) return rc; }
    API_TRY
    ilupp_ml *m = g.m;
    hipStream_t st = m->obj[0]->stream;
    const DevMat *R = &g.A;                                    // the rows of A, for the products
    if (!g.A.is_csr) { transpose_storage(st, g.A, &g.T); R = &g.T; }
    PoolBlock b_r, b_y, b_t;
    for (PoolBlock *b : {&b_r, &b_y, &b_t}) ILUPP_HIP(b->alloc(sizeof(double) * (size_t)n));
    struct SyncOnExit { hipStream_t st; ~SyncOnExit() { (void)hipStreamSynchronize(st); } } quiesce{st};      // (before the blocks go back)
    double *r = b_r.as<double>(), *y = b_y.as<double>(), *tmp = b_t.as<double>();
    ILUPP_HIP(hipMemcpyAsync(r, rhs, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    { const int rc = ml_apply_dev(m, r, 0, 1); if (rc) return rc; }                                              // r = L' b (preconditioned_rhs)
    auto op = [&](const double *in, double *out) -> int {       // out = L'(A(R' in))
        ILUPP_HIP(hipMemcpyAsync(tmp, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        int rc = ml_apply_dev(m, tmp, 0, 2);
        if (rc) return rc;
        rc = ilupp_hip_spmv_device(R->val, R->idx, R->ptr, n, R->nnz, tmp, out, st);
        if (rc) return rc;
        return ml_apply_dev(m, out, 0, 1);
    };
    int32_t it = 0; double rel = 0.0, res = 0.0;
    { const int rc = bicgstab_split(st, n, op, r, y, 1, max_iter, rtol, atol, &it, &rel, &res); if (rc) return rc; }
    { const int rc = ml_apply_dev(m, y, 0, 2); if (rc) return rc; }                                              // x = R' y (adapt_solution)
    { const int rc = ml_finish_apply(m); if (rc) return rc; }
    ILUPP_HIP(hipMemcpy(x, y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (iterations) *iterations = it;
    if (rel_reached) *rel_reached = rel;
    if (abs_reached) *abs_reached = res;
    if (!(rel < rtol && res < atol)) { set_error("did not converge"); return ILUPP_ERR_NOT_CONVERGED; }         // iterative_solvers_implementation.h:497
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_ml_sync(ilupp_ml *m)
{
    API_TRY
    if (!m) return ILUPP_ERR_INVALID;
    return ml_finish_apply(m);
    API_CATCH
}

int32_t ilupp_hip_ml_levels(const ilupp_ml *m) { return m ? (int32_t)m->obj.size() : 0; }

int64_t ilupp_hip_ml_total_nnz(const ilupp_ml *m)          // preconditioner.h:312 with preconditioner_implementation.h:551-569
{
    if (!m) return 0;
    int64_t sum = 0;
    for (const ilupp_precond *p : m->obj) sum += (p->Lc.nnz - p->n) + (p->Uc.nnz - p->n) + p->n;
    return sum;
}

int ilupp_hip_ml_level_info(const ilupp_ml *m, int32_t level, int32_t *n, int64_t *nnz_left, int64_t *nnz_right)
{
    if (!m || level < 0 || level >= (int32_t)m->obj.size()) { set_error("no such level"); return ILUPP_ERR_INVALID; }
    const ilupp_precond *p = m->obj[(size_t)level];
    if (n) *n = p->n;
    if (nnz_left) *nnz_left = p->Lc.nnz;
    if (nnz_right) *nnz_right = p->Uc.nnz;
    return ILUPP_OK;
}

int ilupp_hip_ml_level_copy(const ilupp_ml *m, int32_t level, double *l_data, int32_t *l_indices, int32_t *l_indptr, double *u_data, int32_t *u_indices,
                            int32_t *u_indptr, double *middle, int32_t *perm_rows, int32_t *perm_cols, int32_t *inv_perm_rows, int32_t *inv_perm_cols,
                            double *d_left, double *d_right)
{
    API_TRY
    if (!m || level < 0 || level >= (int32_t)m->obj.size()) { set_error("no such level"); return ILUPP_ERR_INVALID; }
    const ilupp_precond *p = m->obj[(size_t)level];
    const MlLevelDev &l = m->dev[(size_t)level];
    ILUPP_HIP(stream_sync(p->stream));
    const size_t n = (size_t)p->n;
    get_host(l_data, p->Lc.val, sizeof(double) * (size_t)p->Lc.nnz); get_host(l_indices, p->Lc.idx, sizeof(int32_t) * (size_t)p->Lc.nnz); get_host(l_indptr, p->Lc.ptr, sizeof(int32_t) * (n + 1));
    get_host(u_data, p->Uc.val, sizeof(double) * (size_t)p->Uc.nnz); get_host(u_indices, p->Uc.idx, sizeof(int32_t) * (size_t)p->Uc.nnz); get_host(u_indptr, p->Uc.ptr, sizeof(int32_t) * (n + 1));
    get_host(middle, l.D, sizeof(double) * n);
    get_host(perm_rows, l.pr, sizeof(int32_t) * n); get_host(perm_cols, l.pc, sizeof(int32_t) * n);
    get_host(inv_perm_rows, l.ipr, sizeof(int32_t) * n); get_host(inv_perm_cols, l.ipc, sizeof(int32_t) * n);
    get_host(d_left, l.Dl, sizeof(double) * n); get_host(d_right, l.Dr, sizeof(double) * n);
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_ml_timings(const ilupp_ml *m, float *construct_ms, float *kernel_ms, float *last_apply_ms)
{
    if (!m) return ILUPP_ERR_INVALID;
    if (construct_ms) *construct_ms = m->construct_ms;
    if (kernel_ms) *kernel_ms = m->kernel_ms;
    if (last_apply_ms) *last_apply_ms = m->last_apply_ms;
    return ILUPP_OK;
}

}  // extern "C"
