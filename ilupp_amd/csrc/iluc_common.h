// ilupp_amd/csrc/iluc_common.h -- what the dataflow factorisations share on the host (iluc_df.hip: ILUC2, reference ILUC.hpp:112-207;
// piluc_df.hip: partialILUC of the multilevel preconditioner, reference ILUCDP.hpp:1405-2231; icholt_df.hip: ICholT): the layout of the
// control words and ready queues, the passes over A that run before the Crout steps (defined in iluc_df.hip), the exclusive scan (also
// ml.hip's), lengths -> row pointers, and the holders of an attempt's blocks, which go back when the scope ends: an ILUPP_HIP that throws
// in the middle must not leak them.
#pragma once

#include <hipcub/hipcub.hpp>

#include "common.h"
#include "df_ladder.h"

namespace ilupp {

static constexpr int kCuQ = 64;           // ready queues (step i goes to queue i % nq); icholt_df.hip's columns use the same layout
static constexpr int kCuQBase = 64;       // ctrl word of queue 0's head; queue q: head at kCuQBase + 64 q, tail 32 words later
static constexpr unsigned kCuSpinLimit = 1u << 22;

__device__ __forceinline__ unsigned long long cu_pack2(int lo, int hi)
{
    return (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32);
}

// pending[x]: entries of A left of the diagonal in row x and above it in column x; colcnt[c]: rows below the diagonal in column c
__global__ void k_iluc_prep(int32_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, int32_t *pending, int32_t *colcnt);
__global__ void k_iluc_rowof(int32_t n, const int32_t *__restrict__ ptr, int32_t *__restrict__ rowof);
// the sub-diagonal part of A by columns in the order the reference walks its listA / headA chains (ILUC.hpp:74-101): by pairwise ranking
// where columns are short, by the sequential threading itself (host, pattern only) where they are long
int iluc_column_order(hipStream_t st, int32_t m, const DevMat &Av, const int32_t *colcnt, const int32_t *colptr, int32_t *fillc, int32_t *colpos,
                      const int32_t *rowof, int32_t *colord);
// the steps nothing reaches go to the ready queues
__global__ void k_iluc_seed(int32_t m, int32_t nq, const int32_t *__restrict__ pending, int32_t *rq, int32_t *ctrl);

// out[i] = in[0] + ... + in[i - 1] for i < count.  Without `scratch` the scan is waited for.  With a block of the caller's it is only
// queued on st, and the block must live until it has run (the pool knows nothing of streams).
// In: const int32_t * or int32_t * -- hipcub instantiates its kernels per iterator type, and every file passes the type it always passed,
// so that its device code stays what it was
template <class In>
inline void scan_i32(hipStream_t st, In in, int32_t *out, int count, PoolBlock *scratch = nullptr)
{
    PoolBlock own;
    PoolBlock &tmp = scratch ? *scratch : own;
    size_t tb = 0;
    ILUPP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, count, st));
    ILUPP_HIP(tmp.alloc(tb > 0 ? tb : 1));
    ILUPP_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, count, st));
    if (!scratch) ILUPP_HIP(hipStreamSynchronize(st));
}

// lengths of m rows (len[m] = 0) -> their row pointers, and the read-back of ptr[m] queued behind the scan: *nnz holds it after the
// caller's wait, until which `scratch` must live
template <class In>
inline void rowptr_nnz_queue(hipStream_t st, In len, int32_t *ptr, int32_t m, int32_t *nnz, PoolBlock &scratch)
{
    scan_i32(st, len, ptr, m + 1, &scratch);
    ILUPP_HIP(hipMemcpyAsync(nnz, ptr + m, sizeof(int32_t), hipMemcpyDeviceToHost, st));
}

// a pool block of n elements of T
template <class T>
struct PoolArray : PoolBlock {
    void alloc(size_t n) { ILUPP_HIP(PoolBlock::alloc(sizeof(T) * n)); }
    void zero(hipStream_t st, size_t n) { ILUPP_HIP(hipMemsetAsync(p, 0, sizeof(T) * n, st)); }
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
};
#define DF_LDS_CLASS(family, C) family[C].entries, family[C].slots, family[C].records, false      // template arguments of the launch of LDS class C

static constexpr int32_t kDfNone = 0x7fffffff;          // ctrl[3] while no step has reported itself there

// The ready queues and control words of an attempt: at most kCuQ queues of ceil(m / nq) steps each (step i goes to queue i % nq, so the
// number of steps a queue will ever get is known), ctrl[0 .. kCuQBase) for the status words, then 64 words per queue.
struct DfQueues {
    PoolArray<int32_t> rq, ctrl;
    size_t rq_len = 0;
    static constexpr size_t ctrl_len = kCuQBase + 64 * kCuQ;
    void alloc(int32_t m)
    {
        rq_len = (size_t)kCuQ * (size_t)((m + kCuQ - 1) / kCuQ) + (size_t)m;
        rq.alloc(rq_len); ctrl.alloc(ctrl_len);
    }
    // empty queues, zero control words; with_none: nothing reported in ctrl[3] (the kernels take the minimum there)
    void clear(hipStream_t st, bool with_none = true)
    {
        static const int32_t none = kDfNone;
        ILUPP_HIP(hipMemsetAsync(rq, 0xff, sizeof(int32_t) * rq_len, st));
        ctrl.zero(st, ctrl_len);
        if (with_none) ILUPP_HIP(hipMemcpyAsync(ctrl.get() + 3, &none, sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    static int queues_for(int waves) { return waves < kCuQ ? waves : kCuQ; }        // (every queue needs a worker)
};

// What both Crout attempts need before their steps start: the counters of announced entries, the sub-diagonal part of A by columns in
// the reference's traversal order (colptr / colord; rowof: the row of a CSR position), and the touch records of the steps.
// The pre-pass: count_columns, the scan of colcnt into colptr (called by the attempt, with its file's pointer type), column_order.
struct CroutWork {
    PoolArray<int32_t> pending, colcnt, colptr, fillc, colpos, colord, rowof, cntL, cntU;
    PoolArray<unsigned long long> recL, recU;                          // [m][T][4]
    int32_t m = 0;
    void alloc(int32_t rows, int64_t nnz, int T)
    {
        m = rows;
        const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
        pending.alloc(m); colcnt.alloc(m + 1); colptr.alloc(m + 1); fillc.alloc(m + 1);
        colpos.alloc(nz); colord.alloc(nz); rowof.alloc(nz);
        cntL.alloc(m); cntU.alloc(m); recL.alloc((size_t)m * T * 4); recU.alloc((size_t)m * T * 4);
    }
    void clear(hipStream_t st) { pending.zero(st, m); colcnt.zero(st, m + 1); fillc.zero(st, m + 1); cntL.zero(st, m); cntU.zero(st, m); }
    void count_columns(hipStream_t st, const DevMat &Av)
    {
        const int gb = (m + 255) / 256;
        hipLaunchKernelGGL(k_iluc_prep, dim3(gb), dim3(256), 0, st, m, Av.ptr, Av.idx, pending, colcnt);
        hipLaunchKernelGGL(k_iluc_rowof, dim3(gb), dim3(256), 0, st, m, Av.ptr, rowof);
    }
    int column_order(hipStream_t st, const DevMat &Av) { return iluc_column_order(st, m, Av, colcnt, colptr, fillc, colpos, rowof, colord); }
};

}  // namespace ilupp
