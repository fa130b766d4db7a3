// ilupp_amd/csrc/ilu0_batch.hip -- the numeric ILU(0) re-factorisation of MANY small objects in ONE launch: one workgroup per member, the
// member's rows side by side inside it (gfx950 only).
//
// The objects keep their patterns, schedules and tables; only the VALUES of the two CSR triangles change (same pattern, new values of A).
// One re-factorisation alone is a latency chain that costs two host waits (ilupp_hip_ilu0_refactor_device); a batch of members fills the
// chip's CUs and waits for nothing.
//
// Per member (RefactorDesc: A's CSR triple, L's and U's triples, n, nnzA, the status word):
//   pass 1, a PROOF that reads everything and writes nothing: aptr[n] == nnzA, and row by row A's stored row is exactly L's strictly-lower
//     indices followed by U's diagonal-plus-upper indices (every extent is checked against nnzA before an index of A is read through it).
//     On any difference the status word becomes 1 and the workgroup returns: the factor stays bitwise as it was.  The pass also finds the
//     member's longest row.
//   pass 2, compute_ilu0 of the reference operation for operation (ILU0.hpp:26-66, sparse_vec_update :8-23; k_ilu0_numeric of ilu0.hip is
//     the same loop): row-wise IKJ, k ascending over the row's strictly-lower entries, l_ik = w_k / u_kk, then w_j = w_j - l_ik * u_kj for
//     every column j > k present in both rows (separate multiply and subtract: -ffp-contract=off).  L's unit diagonal is written too.  A
//     zero or non-finite pivot is no error: the Inf / NaN that follows is what the single call gives, bit for bit.
//
// Rows run side by side in batch_sweep's idiom (sptrsv_batch.hip): one lane per row (rows t, t + 256, ...: a lane's rows ascend, so the
// lowest unfinished row of the member is always somebody's current row), every lane retries its pending pivot row once per trip of its
// wave, no lane ever blocks inside divergent code.  A finished row is published by a workgroup-scope RELEASE store of its flag in LDS
// behind its value stores; a consumer ACQUIRES the flag at workgroup scope before it reads the pivot row's U values.  All waves of a
// workgroup sit on one CU with one L1 (the `tmp` hand-over of sptrsv_batch.hip relies on the same); nothing here crosses a CU, and
// members share nothing.  Waits are bounded as batch_sweep's: a workgroup progress counter and an idle limit; a wave that gives up sets
// the member's status to 2 and every other wave of the workgroup leaves.
//
// The working row.  An elimination is a chain of dependent loads, and the chain of a member's levels is what the launch lasts.  A lane keeps
// its working row in LDS: per stored entry the column, the working value and -- for the strictly-lower entries, which name the pivot rows
// -- where that pivot's U row starts and how long it is (pattern only: fetched when the row is opened, before any pivot row is finished).
// The pivot row's entries come kRG at a time with their loads in flight together, so an elimination costs one trip to memory behind the
// flag instead of one per entry, and the merge walks the row in LDS; the row's L and U values are stored once, when it is finished.
//
// ROW CAP.  That takes 20 bytes x 256 lanes = 5 120 bytes per entry of the member's longest row behind the 4 n bytes of flags, and both
// must fit into the LDS a workgroup may have: longest row <= (cap - 4 n) / 5 120 and never above kRfMaxRow = 31 (28 entries at n = 4 000,
// 16 at n = 20 000).  A member above it is not launched (the host sends it to the single path, route 1: ilu0_refactor_batch_fits).  The
// cap is also what bounds a trip: a lane opens at most one row (31 entries) and eliminates at most 30 pivots of 31 LDS steps each, tens
// of microseconds at the worst, against an idle limit of 2^20 trips of a waiting wave (tenths of a second).
//
// LDS: 4 n bytes of flags, then 5 120 bytes per entry of the longest row (dynamic); four words static.
//
// FIRST CONSTRUCTION of many members (ilupp_hip_ilu0_create_batch*): two more launches of one workgroup per member around one read-back.
//   k_ilu0_symbolic_batch reads A's pattern row by row -- 0 <= aptr[r] <= aptr[r + 1] <= nnzA before an index is read through them, column
//     indices strictly ascending inside [0, n), the diagonal present --, counts the strictly-lower and the diagonal-plus-upper entries and
//     writes L's and U's row pointers with a workgroup-wide running scan over the rows (256 rows a round, the carry in registers; L's rows
//     carry one entry more, the unit diagonal).  It leaves a CreateInfo per member: nnz(L), nnz(U), the longest row, the first row without
//     a diagonal, and the flags that send the member to the single constructor or refuse it.
//   k_ilu0_create_batch, once the host has allocated the exact index and value arrays: the two patterns in the layout ilu0_write_patterns /
//     ilu0_unit_diagonal leave (L strictly lower ascending, the unit diagonal last; U the diagonal first, then ascending), a workgroup
//     barrier that makes them visible to the workgroup's other waves, and then pass 2 above on the member -- refactor_member, the same
//     device function with the same LDS layout, row cap, bounded waits and status words as k_ilu0_refactor_batch.
#include <limits.h>

#include "common.h"
#include "refactor_batch.h"

namespace ilupp {

// pass 2 for one member; the working rows in LDS (wv, wc, wk0, wkl: entry q of this lane at [q * 256 + tid])
__device__ __forceinline__ void refactor_rows(const RefactorDesc &d, int *rf_done, double *wv, int *wc, int *wk0, int *wkl,
                                              unsigned *s_progress, int *s_fail)
{
    const int n = d.n, tid = threadIdx.x;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr, uptr = (rf_cint)d.uptr, uidx = (rf_cint)d.uidx;
    const rf_cdbl aval = (rf_cdbl)d.aval;
    const rf_dbl lval = (rf_dbl)d.lval, uval = (rf_dbl)d.uval;      // (written by one lane, read by others)
    constexpr unsigned kIdleLimit = 1u << 20;       // trips of a wave without progress anywhere in the workgroup, as batch_sweep
    unsigned seen = 0, idle = 0;
    int r = tid;
    bool alive = r < n, need_init = true;
    int a0 = 0, len = 0, cl = 0, l0 = 0, u0 = 0, p = 0;
    auto col = [&](int q) -> int { return wc[q * kRfThreads + tid]; };
    auto wget = [&](int q) -> double { return wv[q * kRfThreads + tid]; };
    auto wset = [&](int q, double v) { wv[q * kRfThreads + tid] = v; };
    while (__ballot(alive) != 0ull) {
        if (idle > kIdleLimit) {
            if ((tid & 63) == 0) __hip_atomic_store(s_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            break;
        }
        bool did = false;
        if (alive) {
            if (need_init) {                                                    // U[i,:] = A[i,:]   (ILU0.hpp:36-37)
                a0 = aptr[r]; len = aptr[r + 1] - a0;
                l0 = lptr[r]; cl = lptr[r + 1] - l0 - 1; u0 = uptr[r];
                // (kRG entries' loads in flight together: a loop of load-then-store to LDS waits for memory once per entry)
                for (int q0 = 0; q0 < len; q0 += kRG) {
                    int c[kRG];
                    double v[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < len) { c[q] = aidx[a0 + q0 + q]; v[q] = aval[a0 + q0 + q]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < len) { wc[(q0 + q) * kRfThreads + tid] = c[q]; wv[(q0 + q) * kRfThreads + tid] = v[q]; }
                }
                for (int q0 = 0; q0 < cl; q0 += kRG) {
                    int b[kRG], e[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < cl) { const int k = wc[(q0 + q) * kRfThreads + tid]; b[q] = uptr[k]; e[q] = uptr[k + 1]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < cl) { wk0[(q0 + q) * kRfThreads + tid] = b[q]; wkl[(q0 + q) * kRfThreads + tid] = e[q] - b[q]; }
                }
                p = 0;
                need_init = false;
                did = true;
            }
            while (p < cl) {                                                    // for k < i in row  (ILU0.hpp:47-62)
                const int k = col(p);
                if (__hip_atomic_load(&rf_done[k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) break;      // row k not finished: next trip
                const int ku0 = wk0[p * kRfThreads + tid], kl = wkl[p * kRfThreads + tid];
                const double piv = uval[ku0];                                   // the first entry of U's row k
                const double l_ik = wget(p) / piv;                              // ILU0.hpp:52
                int pp = p + 1;
                bool stop = false;
                for (int jb = 1; jb < kl && !stop; jb += kRG) {                 // sparse_vec_update (ILU0.hpp:8-23), kRG entries' loads together
                    int m[kRG];
                    double u[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (jb + q < kl) { m[q] = uidx[ku0 + jb + q]; u[q] = uval[ku0 + jb + q]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (jb + q < kl && !stop) {
                            while (pp < len && col(pp) < m[q]) ++pp;
                            if (pp >= len) {
                                stop = true;
                            } else if (col(pp) == m[q]) {
                                const double prod = l_ik * u[q];
                                wset(pp, wget(pp) - prod);
                                ++pp;
                            }
                        }
                }
                wset(p, l_ik);                                                  // ILU0.hpp:61
                ++p;
                did = true;
            }
            if (p == cl) {
                for (int q = 0; q < cl; ++q) lval[l0 + q] = wv[q * kRfThreads + tid];
                for (int q = cl; q < len; ++q) uval[u0 + q - cl] = wv[q * kRfThreads + tid];
                lval[l0 + cl] = 1.0;                                            // L's unit diagonal (ILU0.hpp:93)
                __hip_atomic_store(&rf_done[r], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);      // behind the row's value stores
                r += kRfThreads;
                alive = r < n;
                need_init = true;
                did = true;
            }
        }
        if (__ballot(did) != 0ull) {
            if ((tid & 63) == 0) atomicAdd(s_progress, 1u);
            idle = 0;
        } else {
            const unsigned now = __hip_atomic_load(s_progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (now != seen) { seen = now; idle = 0; } else ++idle;
            if (__hip_atomic_load(s_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0) break;      // (another wave gave up: its rows never come)
        }
    }
}

// pass 2 for one member whose pattern is proved (or was just written), behind a workgroup barrier: the LDS behind the flags carved into the
// lanes' working rows, the rows factored, the member's status word written.  What k_ilu0_refactor_batch and k_ilu0_create_batch share.
__device__ __forceinline__ void refactor_member(const RefactorDesc &d, unsigned char *rf_lds, unsigned lds_bytes, int maxlen, int32_t *status,
                                                unsigned *s_progress, int *s_fail)
{
    const int n = d.n, tid = threadIdx.x;
    int *rf_done = reinterpret_cast<int *>(rf_lds);
    const size_t fb = rf_flag_bytes(n), rows = (size_t)maxlen * kRfRowBytes;
    if (maxlen > kRfMaxRow || fb + rows > (size_t)lds_bytes) {
        // (a row above the cap: the host launches no such member -- its routing reads the longest row the analysis recorded; no value was written)
        if (tid == 0) status[d.member] = 2;
        return;
    }
    double *wv = reinterpret_cast<double *>(rf_lds + fb);
    int *wc = reinterpret_cast<int *>(wv + (size_t)maxlen * kRfThreads);
    int *wk0 = wc + (size_t)maxlen * kRfThreads, *wkl = wk0 + (size_t)maxlen * kRfThreads;
    refactor_rows(d, rf_done, wv, wc, wk0, wkl, s_progress, s_fail);
    __syncthreads();
    if (tid == 0) status[d.member] = *s_fail != 0 ? 2 : 0;
}

__global__ void __launch_bounds__(kRfThreads)
k_ilu0_refactor_batch(const RefactorDesc *__restrict__ table, int32_t *__restrict__ status, const unsigned lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail, s_bad, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    int *rf_done = reinterpret_cast<int *>(rf_lds);                             // row r of the member is finished (its L and U values are stored)
    if (tid == 0) { s_progress = 0; s_fail = 0; s_maxlen = 0; s_bad = (int64_t)d.aptr[n] != d.nnzA ? 1 : 0; }
    for (int i = tid; i < n; i += kRfThreads) rf_done[i] = 0;

    // ---- pass 1: the proof ----
    bool bad = false;
    int maxlen = 0;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr, lidx = (rf_cint)d.lidx, uptr = (rf_cint)d.uptr,
                  uidx = (rf_cint)d.uidx;
    for (int r = tid; r < n; r += kRfThreads) {
        const int a0 = aptr[r], a1 = aptr[r + 1];
        const int l0 = lptr[r], cl = lptr[r + 1] - l0 - 1, u0 = uptr[r], ul = uptr[r + 1] - u0;
        if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA || cl < 0 || ul < 1 || a1 - a0 != cl + ul) { bad = true; continue; }
        for (int q0 = 0; q0 < cl + ul; q0 += kRG) {  // (kRG entries' loads in flight together)
            int a[kRG], f[kRG];
#pragma unroll
            for (int q = 0; q < kRG; ++q)
                if (q0 + q < cl + ul) { a[q] = aidx[a0 + q0 + q]; f[q] = q0 + q < cl ? lidx[l0 + q0 + q] : uidx[u0 + (q0 + q - cl)]; }
#pragma unroll
            for (int q = 0; q < kRG; ++q) if (q0 + q < cl + ul) bad |= a[q] != f[q];
        }
        maxlen = max(maxlen, a1 - a0);
    }
    __syncthreads();                                 // (thread 0's words and the flags are there)
    if (bad) __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (s_bad != 0) {
        if (tid == 0) status[d.member] = 1;          // (one writer per member: its own word; nothing else was written)
        return;
    }

    refactor_member(d, rf_lds, lds_bytes, s_maxlen, status, &s_progress, &s_fail);
}

// ---- first construction: the symbolic launch ----

__global__ void __launch_bounds__(kRfThreads)
k_ilu0_symbolic_batch(const RefactorDesc *__restrict__ table, CreateInfo *__restrict__ info)
{
    __shared__ int s_wl[kRfThreads / 64], s_wu[kRfThreads / 64];                // the waves' totals of one round of the scan
    __shared__ int s_missing, s_flags, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx;
    const rf_int lptr = (rf_int)d.lptr, uptr = (rf_int)d.uptr;
    if (tid == 0) { s_missing = INT_MAX; s_flags = 0; s_maxlen = 0; lptr[0] = 0; uptr[0] = 0; }
    bool bad = false;
    int maxlen = 0, missing = INT_MAX;
    int carry_l = 0, carry_u = 0;                    // entries of L and of U in the rows of the rounds before
    for (int base = 0; base < n; base += kRfThreads) {
        const int r = base + tid;
        int nl = 0, nu = 0;                          // row r's entries in L (the unit diagonal counted) and in U
        if (r < n) {
            const int a0 = aptr[r], a1 = aptr[r + 1];
            nl = 1;
            if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA) {
                bad = true;                          // (nothing is read through such extents)
            } else {
                const int len = a1 - a0;
                int cl = 0, prev = -1;
                bool diag = false;
                for (int q0 = 0; q0 < len; q0 += kRG) {      // (kRG entries' loads in flight together)
                    int c[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < len) c[q] = aidx[a0 + q0 + q];
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (q0 + q < len) {
                            bad |= c[q] <= prev || c[q] >= n;              // (prev >= -1: a negative index is caught too)
                            cl += c[q] < r ? 1 : 0;
                            diag |= c[q] == r;
                            prev = c[q];
                        }
                }
                nl = cl + 1; nu = len - cl;
                if (!diag) missing = min(missing, r);
                maxlen = max(maxlen, len);
            }
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
        for (int k = 0; k < kRfThreads / 64; ++k) {
            if (k < w) { before_l += s_wl[k]; before_u += s_wu[k]; }
            all_l += s_wl[k]; all_u += s_wu[k];
        }
        if (r < n) { lptr[r + 1] = carry_l + before_l + xl; uptr[r + 1] = carry_u + before_u + xu; }
        carry_l += all_l; carry_u += all_u;
        __syncthreads();                             // (the totals are read: the next round may write them)
    }
    if (bad) atomicOr(&s_flags, kCreateUnsorted);
    atomicMin(&s_missing, missing);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (tid == 0) {
        CreateInfo o;
        o.nnz_l = carry_l; o.nnz_u = carry_u; o.max_row_len = s_maxlen;
        o.missing = s_missing == INT_MAX ? -1 : s_missing;
        o.flags = s_flags | ((int64_t)aptr[n] != d.nnzA ? kCreateNnzDiffers : 0);
        o.pad[0] = o.pad[1] = o.pad[2] = 0;
        info[blockIdx.x] = o;
    }
}

// ---- first construction: the patterns, then the factorisation ----
__global__ void __launch_bounds__(kRfThreads)
k_ilu0_create_batch(const RefactorDesc *__restrict__ table, int32_t *__restrict__ status, const unsigned lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail, s_bad, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    int *rf_done = reinterpret_cast<int *>(rf_lds);
    if (tid == 0) { s_progress = 0; s_fail = 0; s_maxlen = 0; s_bad = 0; }
    for (int i = tid; i < n; i += kRfThreads) rf_done[i] = 0;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr, uptr = (rf_cint)d.uptr;
    const rf_int lidx = (rf_int)d.lidx, uidx = (rf_int)d.uidx;
    bool bad = false;
    int maxlen = 0;
    for (int r = tid; r < n; r += kRfThreads) {
        const int a0 = aptr[r], a1 = aptr[r + 1];
        const int l0 = lptr[r], cl = lptr[r + 1] - l0 - 1, u0 = uptr[r], ul = uptr[r + 1] - u0;
        // (the row pointers are the symbolic launch's; a matrix that is no longer the one it read writes nothing)
        if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA || cl < 0 || ul < 1 || a1 - a0 != cl + ul) { bad = true; continue; }
        for (int q0 = 0; q0 < cl + ul; q0 += kRG) {  // (kRG entries' loads in flight together)
            int c[kRG];
#pragma unroll
            for (int q = 0; q < kRG; ++q) if (q0 + q < cl + ul) c[q] = aidx[a0 + q0 + q];
#pragma unroll
            for (int q = 0; q < kRG; ++q)
                if (q0 + q < cl + ul) { if (q0 + q < cl) lidx[l0 + q0 + q] = c[q]; else uidx[u0 + (q0 + q - cl)] = c[q]; }
        }
        lidx[l0 + cl] = r;                           // L's unit diagonal comes last (ILU0.hpp:93)
        maxlen = max(maxlen, a1 - a0);
    }
    __syncthreads();                                 // (thread 0's words and the flags are there)
    if (bad) __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();                                 // (... and the patterns, for the workgroup's other waves: refactor_rows reads uidx of other lanes' rows)
    if (s_bad != 0) {
        if (tid == 0) status[d.member] = 1;
        return;
    }
    refactor_member(d, rf_lds, lds_bytes, s_maxlen, status, &s_progress, &s_fail);
}

// bytes of dynamic LDS one workgroup of k_ilu0_refactor_batch may take on the current device
// (... and of k_ilu0_create_batch, which has the same static words: the smaller of the two, so that one routing serves both launches)
static size_t ilu0_refactor_batch_lds_cap()
{
    const size_t a = kernel_lds_cap<k_ilu0_refactor_batch>(), b = kernel_lds_cap<k_ilu0_create_batch>();
    return a < b ? a : b;
}

// the largest n of a member of the launch: its flags and working rows of kRfMinRow entries fit (a member of that n with longer rows does not)
static constexpr int kRfMinRow = 8;
int64_t ilu0_refactor_batch_max_n()
{
    const size_t cap = ilu0_refactor_batch_lds_cap(), rows = (size_t)kRfMinRow * kRfRowBytes;
    return cap > rows + 8 ? (int64_t)((cap - rows) / sizeof(int)) - 1 : 0;
}

// the bytes of LDS a member of n rows whose longest row has max_row_len entries asks of the launch (flags + working rows), or 0 when it is
// above the row cap: max_row_len > kRfMaxRow, or flags and rows do not fit into the LDS a workgroup may have
size_t ilu0_refactor_batch_fits(int32_t n, int32_t max_row_len)
{
    if (max_row_len < 1 || max_row_len > kRfMaxRow) return 0;
    const size_t want = rf_flag_bytes(n) + (size_t)max_row_len * kRfRowBytes;
    return want <= ilu0_refactor_batch_lds_cap() ? want : 0;
}

// `count` members, one workgroup each; lds_bytes: the largest ilu0_refactor_batch_fits among them; member k's status goes to d_status[table[k].member]
int ilu0_refactor_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, int32_t *d_status, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > ilu0_refactor_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_ilu0_refactor_batch, dim3((unsigned)count), dim3(kRfThreads), lds_bytes, st, d_table, d_status, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// the symbolic launch of a batched first construction: member k's record goes to d_info[k]
int ilu0_symbolic_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, CreateInfo *d_info)
{
    if (count <= 0) return ILUPP_OK;
    hipLaunchKernelGGL(k_ilu0_symbolic_batch, dim3((unsigned)count), dim3(kRfThreads), 0, st, d_table, d_info);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// its create launch: as ilu0_refactor_batch_launch (status 1: the matrix is not the one the symbolic launch read, nothing was written)
int ilu0_create_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, int32_t *d_status, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > ilu0_refactor_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_ilu0_create_batch, dim3((unsigned)count), dim3(kRfThreads), lds_bytes, st, d_table, d_status, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
