// ilupp_amd/csrc/ilut.hip -- Saad's ILUT(p, tau), heap variant, for gfx950: the host driver.
//
// Replaces ILUT_heap (reference ILUT.hpp:199-278), threshold_and_drop (dropping.hpp:8-34), the working-row
// containers vector_sparse_dynamic / vector_sparse_ordered (sparse.h:169-323, sparse_implementation.h:950-1093),
// append_row_with_prefix/suffix (:3190-3230) and compress (:3696-3722).
//
// The sparsity pattern of L and U depends on the VALUES (thresholds, top-k by magnitude), so nothing can be scheduled ahead:
// the rows are computed by a row-wise dataflow kernel, one wave per row (ilut_wp.hip: the working row as three
// insertion-ordered pieces in LDS, in 64 K global pieces, or -- the largest capacity class -- in pieces as long as the matrix is
// wide).  Rows go to fixed-pitch slabs (L: p entries per row in plain arrays; U: one record of whole 128-byte lines per row -- length,
// columns, values -- because other rows fetch it while the kernel runs); the compaction pass here drops exact zeros like compress(0.0)
// and makes the CSR arrays of L (unit diagonal last) and U (pivot first).
#include <stdio.h>
#include <stdlib.h>

#include <hipcub/hipcub.hpp>

#include "common.h"

namespace ilupp {

// ---- compaction of the fixed-pitch slabs into CSR, dropping exact zeros (compress(0.0), :3696-3722) -------
// (a row of the slab is lay.si ints / lay.sv doubles / lay.sl ints behind the previous one in the three arrays: p, p, 1 for L's plain
// slabs; the strides of the record slab for U -- common.h: UrowLayout)
__global__ void k_slab_count(int32_t n, UrowLayout lay, const int32_t *__restrict__ rlen, const double *__restrict__ rval, int32_t *__restrict__ cnt)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int c = 0;
    const size_t b = (size_t)r * lay.sv;
    const int len = rlen[(size_t)r * lay.sl];
    for (int q = 0; q < len; ++q) c += (fabs(rval[b + q]) > 0.0) ? 1 : 0;
    cnt[r] = c;
}
__global__ void k_slab_fill(int32_t n, UrowLayout lay, const int32_t *__restrict__ rlen, const int32_t *__restrict__ ridx,
                            const double *__restrict__ rval, const int32_t *__restrict__ ptr,
                            int32_t *__restrict__ idx, double *__restrict__ val)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int o = ptr[r];
    const size_t bi = (size_t)r * lay.si, bv = (size_t)r * lay.sv;
    const int len = rlen[(size_t)r * lay.sl];
    for (int q = 0; q < len; ++q)
        if (fabs(rval[bv + q]) > 0.0) { idx[o] = ridx[bi + q]; val[o] = rval[bv + q]; ++o; }
}

static void compact_slab(hipStream_t st, int32_t n, UrowLayout lay, const int32_t *rlen, const int32_t *ridx, const double *rval, DevMat *M)
{
    int32_t *cnt = nullptr;
    ILUPP_HIP(pool_malloc(&cnt, sizeof(int32_t) * (size_t)n));
    const unsigned gb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_slab_count, dim3(gb), dim3(256), 0, st, n, lay, rlen, rval, cnt);
    M->n = n; M->is_csr = true; M->owns = true;
    ILUPP_HIP(pool_malloc(&M->ptr, sizeof(int32_t) * (size_t)(n + 1)));
    ILUPP_HIP(hipMemsetAsync(M->ptr, 0, sizeof(int32_t), st));
    size_t tmp_bytes = 0;
    ILUPP_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, cnt, M->ptr + 1, n, st));
    void *tmp = nullptr;
    ILUPP_HIP(pool_malloc(&tmp, tmp_bytes > 0 ? tmp_bytes : 16));
    ILUPP_HIP(hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, cnt, M->ptr + 1, n, st));
    int32_t tot = 0;
    ILUPP_HIP(hipMemcpyAsync(&tot, M->ptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ILUPP_HIP(hipStreamSynchronize(st));
    ILUPP_HIP(pool_free(tmp)); ILUPP_HIP(pool_free(cnt));
    M->nnz = tot;
    ILUPP_HIP(pool_malloc(&M->idx, sizeof(int32_t) * (size_t)(tot > 0 ? tot : 1)));
    ILUPP_HIP(pool_malloc(&M->val, sizeof(double) * (size_t)(tot > 0 ? tot : 1)));
    hipLaunchKernelGGL(k_slab_fill, dim3(gb), dim3(256), 0, st, n, lay, rlen, ridx, rval, M->ptr, M->idx, M->val);
}

// ILUT of the row-major view held in A; on ILUPP_ERR_ZERO_PIVOT *err_row is the first row with a zero pivot
int ilut_factor(hipStream_t st, const DevMat &A, int32_t max_fill_in, double threshold, DevMat *L, DevMat *U,
                int32_t *err_row, float *kernel_ms)
{
    const int32_t n = A.n;
    int32_t p = max_fill_in;
    if (p < 1) p = 1;
    if (p > n) p = n;                                           // ILUT.hpp:211-212
    const size_t slab = (size_t)n * p;
    // U's rows as records of whole 128-byte lines: [length][p columns][pad to 8][p values] (other rows fetch them while the kernel runs)
    const size_t voff = ((size_t)4 + 4 * (size_t)p + 7) & ~(size_t)7;
    const size_t rec = (voff + 8 * (size_t)p + 127) & ~(size_t)127;
    if (rec / 4 > 0x7fffffffULL) { set_error("ILUT: the fill budget is too large for the row records"); return ILUPP_ERR_UNSUPPORTED; }
    const UrowLayout ulay = {(int32_t)(rec / 4), (int32_t)(rec / 8), (int32_t)(rec / 4)}, llay = {p, p, 1};
    PoolBlock b_Lri, b_Urec, b_Lrv, b_Llen, b_ctrl;
    ILUPP_HIP(b_Lri.alloc(sizeof(int32_t) * slab));
    ILUPP_HIP(b_Urec.alloc(rec * (size_t)n));
    ILUPP_HIP(b_Lrv.alloc(sizeof(double) * slab));
    ILUPP_HIP(b_Llen.alloc(sizeof(int32_t) * (size_t)n));
    ILUPP_HIP(b_ctrl.alloc(256));
    unsigned char *urec = b_Urec.as<unsigned char>();
    int32_t *Lri = b_Lri.as<int32_t>(), *Uri = reinterpret_cast<int32_t *>(urec + 4), *Llen = b_Llen.as<int32_t>(),
            *Ulen = reinterpret_cast<int32_t *>(urec), *ctrl = b_ctrl.as<int32_t>();
    double *Lrv = b_Lrv.as<double>(), *Urv = reinterpret_cast<double *>(urec + voff);
    const int rw = ilut_rows_wp(st, A, p, threshold, Lri, Lrv, Llen, Uri, Urv, Ulen, ulay, ctrl, kernel_ms);
    if (rw == 1) {
        set_error("ILUT: a working row does not fit the largest capacity class (the matrix is too wide for the memory budget)");
        return ILUPP_ERR_UNSUPPORTED;
    }
    int32_t hw[4] = {0, 0, 0, 0};
    ILUPP_HIP(hipMemcpyAsync(hw, ctrl, 16, hipMemcpyDeviceToHost, st));
    ILUPP_HIP(hipStreamSynchronize(st));
    int rc = rw;
    if (rc == ILUPP_OK && hw[2] != 0x7fffffff) { rc = ILUPP_ERR_ZERO_PIVOT; if (err_row) *err_row = hw[2]; }
    if (rc == ILUPP_OK) {
        compact_slab(st, n, llay, Llen, Lri, Lrv, L);
        compact_slab(st, n, ulay, Ulen, Uri, Urv, U);
        ILUPP_HIP(hipStreamSynchronize(st));
    }
    return rc;
}

// ---- the compaction of MANY members (ilupp_hip_ilut_create_batch*) -----------------------------------------------------------------------
// One workgroup per member: k_slab_count's count of both slabs, row by row, and the two row-pointer arrays by a workgroup-wide running scan
// over the rows (256 rows a round, the carry in registers: k_ilu0_symbolic_batch's scan), then the member's record for the call's one read-back.
static constexpr int kIbThreads = 256;
__global__ void __launch_bounds__(kIbThreads)
k_ilut_count_batch(const IlutBatchDesc *__restrict__ table, IlutBatchInfo *__restrict__ info)
{
    __shared__ int s_wl[kIbThreads / 64], s_wu[kIbThreads / 64];
    __shared__ int s_maxlen;
    const IlutBatchDesc *d = table + blockIdx.x;
    const int n = d->n, p = d->p, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const UrowLayout ul = d->ul;
    const int32_t *Llen = d->Llen, *Ulen = d->Ulen;
    const double *Lrv = d->Lrv, *Urv = d->Urv;
    int32_t *lptr = d->lptr, *uptr = d->uptr;
    if (tid == 0) { s_maxlen = 0; lptr[0] = 0; uptr[0] = 0; }
    int maxlen = 0, carry_l = 0, carry_u = 0;
    for (int base = 0; base < n; base += kIbThreads) {
        const int r = base + tid;
        int nl = 0, nu = 0;
        if (r < n) {
            const int ll = Llen[r], lu = Ulen[(size_t)r * ul.sl];
            const size_t bl = (size_t)r * p, bu = (size_t)r * ul.sv;
            for (int q = 0; q < ll; ++q) nl += (fabs(Lrv[bl + q]) > 0.0) ? 1 : 0;
            for (int q = 0; q < lu; ++q) nu += (fabs(Urv[bu + q]) > 0.0) ? 1 : 0;
            maxlen = max(maxlen, max(nl, nu));
        }
        int xl = nl, xu = nu;                        // inclusive scan over the wave, then over the waves' totals
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int tl = __shfl_up(xl, off), tu = __shfl_up(xu, off);
            if (lane >= off) { xl += tl; xu += tu; }
        }
        if (lane == 63) { s_wl[w] = xl; s_wu[w] = xu; }
        __syncthreads();
        int before_l = 0, before_u = 0, all_l = 0, all_u = 0;
#pragma unroll
        for (int k = 0; k < kIbThreads / 64; ++k) {
            if (k < w) { before_l += s_wl[k]; before_u += s_wu[k]; }
            all_l += s_wl[k]; all_u += s_wu[k];
        }
        if (r < n) { lptr[r + 1] = carry_l + before_l + xl; uptr[r + 1] = carry_u + before_u + xu; }
        carry_l += all_l; carry_u += all_u;
        __syncthreads();                             // (the totals are read: the next round may write them)
    }
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (tid == 0) {
        const int32_t *ctrl = d->ctrl;
        IlutBatchInfo o;
        o.status = ctrl[1]; o.zero_row = ctrl[2] == 0x7fffffff ? -1 : ctrl[2];
        o.nnz_l = carry_l; o.nnz_u = carry_u; o.max_row_len = s_maxlen;
        o.outgrew = ctrl[3]; o.pool = ctrl[4]; o.uslots = ctrl[5]; o.kept = ctrl[6]; o.left_tier2 = ctrl[24];
        for (int q = 0; q < 6; ++q) o.pad[q] = 0;
        info[blockIdx.x] = o;
    }
}

// k_slab_fill for both slabs of every member: blockIdx.y = the member, one thread per row
__global__ void k_ilut_fill_batch(const IlutBatchDesc *__restrict__ table)
{
    const IlutBatchDesc *d = table + blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d->n || !d->lidx || !d->uidx) return;    // (a member that failed or takes the single path has no arrays to fill)
    const int p = d->p;
    const UrowLayout ul = d->ul;
    {
        int o = d->lptr[r];
        const size_t b = (size_t)r * p;
        const int len = d->Llen[r];
        for (int q = 0; q < len; ++q)
            if (fabs(d->Lrv[b + q]) > 0.0) { d->lidx[o] = d->Lri[b + q]; d->lval[o] = d->Lrv[b + q]; ++o; }
    }
    {
        int o = d->uptr[r];
        const size_t bi = (size_t)r * ul.si, bv = (size_t)r * ul.sv;
        const int len = d->Ulen[(size_t)r * ul.sl];
        for (int q = 0; q < len; ++q)
            if (fabs(d->Urv[bv + q]) > 0.0) { d->uidx[o] = d->Uri[bi + q]; d->uval[o] = d->Urv[bv + q]; ++o; }
    }
}

int ilut_batch_count_launch(hipStream_t st, int32_t count, const IlutBatchDesc *d_table, IlutBatchInfo *d_info)
{
    if (count <= 0) return ILUPP_OK;
    hipLaunchKernelGGL(k_ilut_count_batch, dim3((unsigned)count), dim3(kIbThreads), 0, st, d_table, d_info);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

int ilut_batch_fill_launch(hipStream_t st, int32_t count, const IlutBatchDesc *d_table, int32_t max_n)
{
    if (count <= 0) return ILUPP_OK;
    hipLaunchKernelGGL(k_ilut_fill_batch, dim3((unsigned)((max_n + 255) / 256), (unsigned)count), dim3(256), 0, st, d_table);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
