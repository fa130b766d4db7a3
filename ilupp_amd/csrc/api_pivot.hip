// ilupp_amd/csrc/api_pivot.hip -- the pivoting preconditioners' handle (ilupp_ilucp; the struct itself: api_internal.h): ILUCP and ILUTP
// constructions, single and batched, and the single applies (host layer: api.hip).
#include "api_internal.h"

// ===================================================================================================================
// ILUCP: ILUCPPreconditioner, binding.cpp:343-356 -> preconditioner_implementation.h:1117-1147 -> ILUCP4 (ilucp.hip)
// ===================================================================================================================
// The factors come for the major-order view of the input ("Acol"): L by columns, U by rows with the pivot first and ORIGINAL column indices,
// perm[k] = the column of step k.  With U's indices read through the inverse permutation the pair is an object of the ILUC kind (both
// array triples upper CSR with the diagonal first), and the permuted solves of the reference (triangular_solve_perm,
// sparse_implementation.h:4196-4218) are that object's sweeps between a gather and a scatter:
//   COLUMN input, apply / ROW input, apply_trans:   t = (L U')^{-1} x;      x[perm[k]] = t[k]          (:4209-4218 after the plain solve with L)
//   COLUMN input, apply_trans / ROW input, apply:   y[i] = x[perm[i]];      x = (L U')^{-T} y          (:4196-4206 before the plain solve with L^T)
namespace {

// the member's own stream behind the batched launch that last used it (apply_batch_run), before anything else touches tmp or the factors go
void after_batch(ilupp_ilucp *m)
{
    if (!m->batch_ev) return;
    ILUPP_HIP(hipStreamWaitEvent(m->obj->stream, m->batch_ev, 0));
    m->batch_ev = nullptr;
}

}  // namespace

namespace ilupp {

// ILUCP: COLUMN input + apply, ROW input + apply_trans start with the plain factor; ILUTP: ROW input + apply, COLUMN input + apply_trans
bool pivot_plain_first(const ilupp_ilucp *m, int transpose)
{
    return m->row_kind ? ((transpose == 0) == m->input_csr) : ((transpose != 0) == m->input_csr);
}

}  // namespace ilupp

namespace {

__global__ void k_cp_map_indices(int64_t nnz, const int32_t *__restrict__ idx, const int32_t *__restrict__ map, int32_t *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nnz) out[j] = map[idx[j]];
}
__global__ void k_cp_invert(int32_t n, const int32_t *__restrict__ p, int32_t *__restrict__ inv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) inv[p[i]] = i;
}
__global__ void k_cp_gather(int32_t n, const double *__restrict__ x, const int32_t *__restrict__ perm, double *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[perm[i]];
}
__global__ void k_cp_scatter(int32_t n, const double *__restrict__ t, const int32_t *__restrict__ perm, double *__restrict__ x)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[perm[i]] = t[i];
}

void ilucp_destroy(ilupp_ilucp *m)
{
    if (!m) return;
    if (m->batch_ev && m->obj) (void)hipStreamWaitEvent(m->obj->stream, m->batch_ev, 0);      // (destroy_obj waits for the stream)
    if (m->obj) destroy_obj(m->obj);
    m->U.release();
    for (void *q : {(void *)m->perm, (void *)m->tmp, (void *)m->xdev}) if (q) (void)pool_free(q);
    delete m;
}

// What the constructions of the two kinds share: the handle and its object, perm and tmp, the event pair round `factor(m, p, st)`, the
// matrix given back, `fill(m, p, st)` -- the ilupp_precond made from the factor call's result --, the times and the hand-over.
template <class Factor, class Fill>
int pivot_create_frame(DevMat &A, int32_t n, int is_csr, bool row_kind, ilupp_ilucp **out, Factor &&factor, Fill &&fill)
{
    struct Guard { ilupp_ilucp *m; ~Guard() { if (m) ilucp_destroy(m); } } g{new ilupp_ilucp};
    ilupp_ilucp *m = g.m;
    m->n = n; m->input_csr = is_csr != 0; m->row_kind = row_kind;
    m->obj = new_obj(n);
    ilupp_precond *p = m->obj;
    hipStream_t st = p->stream;
    ILUPP_HIP(pool_malloc(&m->perm, sizeof(int32_t) * (size_t)n));
    ILUPP_HIP(pool_malloc(&m->tmp, sizeof(double) * (size_t)n));
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    const int rc = factor(m, p, st);
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    A.release();
    if (rc) return rc;
    fill(m, p, st);
    finish_timing(p, m->kernel_ms);
    *out = m;
    g.m = nullptr;
    return ILUPP_OK;
}

int ilucp_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos, double mem_factor,
                        ilupp_ilucp **out)
{
    MatGuard gl;
    return pivot_create_frame(A, n, is_csr, false, out,
        [&](ilupp_ilucp *m, ilupp_precond *, hipStream_t st) {
            return ilucp_factor(st, A, max_fill_in, threshold, piv_tol, row_pos, mem_factor, &gl.m, &m->U, m->perm, &m->zero_pivots, &m->kernel_ms);
        },
        [&](ilupp_ilucp *m, ilupp_precond *p, hipStream_t st) {
            // U' = U with its column indices in the permuted numbering (values and pointers shared in content, own arrays)
            DevMat Up;
            Up.n = n; Up.nnz = m->U.nnz; Up.is_csr = true; Up.owns = true;
            PoolBlock b_inv;
            ILUPP_HIP(b_inv.alloc(sizeof(int32_t) * (size_t)n));
            hipLaunchKernelGGL(k_cp_invert, dim3((n + 255) / 256), dim3(256), 0, st, n, m->perm, b_inv.as<int32_t>());
            ILUPP_HIP(pool_malloc(&Up.ptr, sizeof(int32_t) * (size_t)(n + 1)));
            ILUPP_HIP(pool_malloc(&Up.idx, sizeof(int32_t) * (size_t)(Up.nnz > 0 ? Up.nnz : 1)));
            ILUPP_HIP(pool_malloc(&Up.val, sizeof(double) * (size_t)(Up.nnz > 0 ? Up.nnz : 1)));
            ILUPP_HIP(hipMemcpyAsync(Up.ptr, m->U.ptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToDevice, st));
            if (Up.nnz > 0) {
                ILUPP_HIP(hipMemcpyAsync(Up.val, m->U.val, sizeof(double) * (size_t)Up.nnz, hipMemcpyDeviceToDevice, st));
                hipLaunchKernelGGL(k_cp_map_indices, dim3((unsigned)((Up.nnz + 255) / 256)), dim3(256), 0, st, Up.nnz, m->U.idx, b_inv.as<int32_t>(), Up.idx);
            }
            ILUPP_HIP(stream_sync(st));
            p->kind = KIND_UTU; p->nnz_mode = NNZ_GENERIC_LU; p->input_csc = false;
            p->Lc = gl.m; p->Uc = Up;
            gl.m = DevMat();                                            // (the object owns the arrays now)
            utu_analyse(p);
        });
}

// The pivoted solve of x (device, n doubles; overwritten), on the member's own stream: the plain solve then the scatter through perm, or
// the gather then the transposed solve.  The result is in m->tmp.
int pivot_solve(ilupp_ilucp *m, double *x, int transpose)
{
    const int32_t n = m->n;
    ilupp_precond *p = m->obj;
    hipStream_t st = p->stream;
    if (pivot_plain_first(m, transpose)) {
        OR_RETURN(apply_dev(p, x, 0));
        hipLaunchKernelGGL(k_cp_scatter, dim3((n + 255) / 256), dim3(256), 0, st, n, x, m->perm, m->tmp);
    } else {
        hipLaunchKernelGGL(k_cp_gather, dim3((n + 255) / 256), dim3(256), 0, st, n, x, m->perm, m->tmp);
        OR_RETURN(apply_dev(p, m->tmp, 1));
    }
    return ILUPP_OK;
}

}  // namespace

extern "C" {

int ilupp_hip_ilucp_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, int32_t max_fill_in,
                           double threshold, double piv_tol, int32_t row_pos, double mem_factor, ilupp_ilucp **out)
{
    return create_from_host(data, indices, indptr, n, true, out,
                            [&](DevMat &A) { return ilucp_create_common(A, n, is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, out); });
}

void ilupp_hip_ilucp_destroy(ilupp_ilucp *m) { ilucp_destroy(m); }

int ilupp_hip_ilucp_apply(ilupp_ilucp *m, double *x, int64_t len, int transpose)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    after_batch(m);
    return apply_staged(m->obj->stream, &m->xdev, m->n, x,
                        [&](double *d) { return pivot_solve(m, d, transpose); },
                        [&] { return finish_apply(m->obj); }, m->tmp);
    API_CATCH
}

int64_t ilupp_hip_ilucp_total_nnz(const ilupp_ilucp *m) { return m ? m->obj->Lc.nnz + m->U.nnz : 0; }      /* preconditioner.h:208-209 */
int32_t ilupp_hip_ilucp_zero_pivots(const ilupp_ilucp *m) { return m ? m->zero_pivots : 0; }

/* sizes, then copies: L of the view by columns (the 1 first), U by rows (the pivot first, original column indices), the permutation */
int ilupp_hip_ilucp_info(const ilupp_ilucp *m, int32_t *n, int64_t *nnz_l, int64_t *nnz_u, float *kernel_ms)
{
    if (!m) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
    if (n) *n = m->n;
    if (nnz_l) *nnz_l = m->obj->Lc.nnz;
    if (nnz_u) *nnz_u = m->U.nnz;
    if (kernel_ms) *kernel_ms = m->kernel_ms;
    return ILUPP_OK;
}

int ilupp_hip_ilucp_copy(const ilupp_ilucp *m, double *l_data, int32_t *l_indices, int32_t *l_indptr, double *u_data, int32_t *u_indices,
                         int32_t *u_indptr, int32_t *perm)
{
    API_TRY
    if (!m) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
    const ilupp_precond *p = m->obj;
    ILUPP_HIP(stream_sync(p->stream));
    const size_t n = (size_t)m->n;
    get_host(l_data, p->Lc.val, sizeof(double) * (size_t)p->Lc.nnz); get_host(l_indices, p->Lc.idx, sizeof(int32_t) * (size_t)p->Lc.nnz); get_host(l_indptr, p->Lc.ptr, sizeof(int32_t) * (n + 1));
    get_host(u_data, m->U.val, sizeof(double) * (size_t)m->U.nnz); get_host(u_indices, m->U.idx, sizeof(int32_t) * (size_t)m->U.nnz); get_host(u_indptr, m->U.ptr, sizeof(int32_t) * (n + 1));
    get_host(perm, m->perm, sizeof(int32_t) * n);
    return ILUPP_OK;
    API_CATCH
}

}  // extern "C"

namespace {

int ilutp_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos, double mem_factor,
                        ilupp_ilucp **out)
{
    return pivot_create_frame(A, n, is_csr, true, out,
        [&](ilupp_ilucp *m, ilupp_precond *p, hipStream_t st) {
            return ilutp_factor(st, A, max_fill_in, threshold, piv_tol, row_pos, mem_factor, &p->Lc, &p->Uc, &m->U, m->perm, &m->zero_pivots, &m->kernel_ms);
        },
        [&](ilupp_ilucp *, ilupp_precond *p, hipStream_t st) {
            // an object of the ILUT kind: L by rows with its 1 last, U (permuted numbering) by rows with the pivot first
            p->kind = KIND_LU; p->nnz_mode = NNZ_ILUT; p->input_csc = false;
            p->compact = sweep_tables(st, p, {&p->Lc, true, &p->sL, &p->dL}, {&p->Uc, false, &p->sU, &p->dU}, true, &p->max_row_len);
        });
}

}  // namespace

extern "C" int ilupp_hip_ilutp_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, int32_t max_fill_in,
                                      double threshold, double piv_tol, int32_t row_pos, double mem_factor, ilupp_ilucp **out)
{
    return create_from_host(data, indices, indptr, n, true, out,
                            [&](DevMat &A) { return ilutp_create_common(A, n, is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, out); });
}

// ---- many matrices at once: the chains of the members side by side, one workgroup each (k_ilucp_batch / k_ilutp_batch) ----
namespace {

// The device memory one construction holds (ilucp_factor / ilutp_factor and the object built from their result), R = the reserved entries
// = min(max_fill_in * n, (Integer) mem_factor * nnz), slot = n + 64:
//   the stores of R + 1 entries             ILUCP 32 bytes per entry (U: index, link, row, value; L: index, value), ILUTP 24 (U and L: index, value)
//   the slot tables                         ILUCP 16 int32 + 5 double tables of `slot` = 104 slot; ILUTP 5 int32 of slot + (5 int32 + 3 double) of 4 slot = 196 slot
//   the sort buffers                        ILUCP: two key arrays of n and the in-kernel sort's of up to 2 n, 8 bytes each = 32 n;
//                                           ILUTP: the segmented sorts of the compress step, keys and values twice over = 24 R
//   the compressed factors                  L, U and U in the other numbering, 12 bytes per entry, each at most R entries = 36 R
//   the uploaded matrix                     12 nnz + 4 (n + 1)
// + 64 MiB for what does not scale with the matrix (the sorts' and scans' temporaries, the sweeps' tables, the pool's rounding).
double pivot_member_bytes(bool tp, int32_t n, int64_t nnz, int32_t max_fill_in, double mem_factor)
{
    int64_t mf = max_fill_in < 1 ? 1 : max_fill_in;
    if (mf > n) mf = n;
    const double a = (double)mf * (double)n, b = (double)((int32_t)mem_factor) * (double)nnz;
    const double R = a < b ? (a > 0.0 ? a : 0.0) : (b > 0.0 ? b : 0.0);
    const double slot = (double)n + 64.0;
    const double stores = (tp ? 24.0 : 32.0) * (R + 1.0), tables = (tp ? 196.0 : 104.0) * slot, sorts = tp ? 24.0 * R : 32.0 * (double)n;
    return stores + tables + sorts + 36.0 * R + 12.0 * (double)nnz + 4.0 * ((double)n + 1.0) + (double)(64 << 20);
}

int pivot_create_batch(bool tp, int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr, const int32_t *n,
                       int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos, double mem_factor, ilupp_ilucp **out,
                       int32_t *status)
{
    if (count < 0 || !data || !indices || !indptr || !n || !out) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) { out[i] = nullptr; if (status) status[i] = ILUPP_OK; }
    if (count == 0) return ILUPP_OK;
    double worst = 0.0;
    for (int32_t i = 0; i < count; ++i)
        if (indptr[i] && n[i] > 0) { const double e = pivot_member_bytes(tp, n[i], indptr[i][n[i]], max_fill_in, mem_factor); if (e > worst) worst = e; }
    return batch_build(count, worst, status, [&](int32_t i) {
        MatGuard A;
        const int rc = upload(data[i], indices[i], indptr[i], n[i], true, &A.m);
        if (rc) return rc;
        return tp ? ilutp_create_common(A.m, n[i], is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, &out[i])
                  : ilucp_create_common(A.m, n[i], is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, &out[i]);
    });
}

}  // namespace

extern "C" int ilupp_hip_ilucp_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                            const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos,
                                            double mem_factor, ilupp_ilucp **out, int32_t *status)
{
    API_TRY_BUILD
    return pivot_create_batch(false, count, data, indices, indptr, n, is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, out, status);
    API_CATCH
}

extern "C" int ilupp_hip_ilutp_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                            const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos,
                                            double mem_factor, ilupp_ilucp **out, int32_t *status)
{
    API_TRY_BUILD
    return pivot_create_batch(true, count, data, indices, indptr, n, is_csr, max_fill_in, threshold, piv_tol, row_pos, mem_factor, out, status);
    API_CATCH
}

namespace ilupp {

// the single apply in place on a device vector, on the member's own stream behind the caller's
int pivot_apply_dev(ilupp_ilucp *m, double *x, int transpose)
{
    const int32_t n = m->n;
    hipStream_t st = m->obj->stream;
    after_batch(m);
    order_after_caller(st, m->obj->sev[0]);
    OR_RETURN(pivot_solve(m, x, transpose));
    ILUPP_HIP(hipGetLastError());
    ILUPP_HIP(hipMemcpyAsync(x, m->tmp, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    return ILUPP_OK;
}

}  // namespace ilupp

extern "C" {

int ilupp_hip_ilucp_apply_device(ilupp_ilucp *m, double *d_x, int64_t len, int transpose, int sync)
{
    API_TRY
    if (!m) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
    if (!d_x) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    if (len != m->n) { set_error("vector has wrong size for preconditioner!"); return ILUPP_ERR_WRONG_SIZE; }
    const int rc = pivot_apply_dev(m, d_x, transpose);
    if (rc) return rc;
    return finish_or_hand_over(sync, *m->obj, [&] { return finish_apply(m->obj); });
    API_CATCH
}

}  // extern "C"
