// ilupp_amd/csrc/ichol0_batch.hip -- IChol(0) of MANY small SPD systems: the numeric re-factorisation in ONE launch and the first
// construction in two, one workgroup per member, the member's rows side by side inside it (gfx950 only).  What ilu0_batch.hip is for
// ILU(0), plus the one piece only IChol(0) needs: the transposed copy of the factor is kept current by the same launch.
//
// Per member (RefactorDesc): A's CSR triple, n, nnzA (A's stored entries, upper triangle included), the status word, and
//   l* = the factor Lc: row-major lower triangle in the single constructor's layout (what k_tri_fill leaves: A's stored entries with
//        column <= row in stored order, i.e. strictly lower ascending and the diagonal LAST);
//   u* = the `u*` fields carry the triple of LcT, the factor's transposed storage (row c ascending, the diagonal FIRST), which the batched
//        apply and cg_batch read next to Lc -- or three null pointers for a member that has none yet.
//
//   pass 1, a PROOF that reads everything and writes nothing: aptr[n] == nnzA, every extent 0 <= aptr[r] <= aptr[r + 1] <= nnzA before an
//     index of A is read through it, and row by row the entries of A's stored row with column <= r, in stored order, are exactly L's row
//     -- strictly ascending, the diagonal last.  Entries above the diagonal are ignored (natural_triangular_part of the reference drops
//     them; a matrix that differs only there is accepted and gives the factor of its lower triangle).  On any difference the status word
//     becomes 1 and the workgroup returns: factor and transposed copy stay bitwise as they were.  The pass also finds L's longest row.
//   pass 2, compute_ichol0 of the reference operation for operation (IChol.hpp:16-59; k_ichol0_numeric of ichol.hip is the same loop): for
//     the entries (i, j) of row i in order, dp = the sum over the matching columns of row i and row j, both without their last entry, in
//     ascending column order with separate multiply and add (-ffp-contract=off); below the diagonal (A_ij - dp) / L_jj, on it
//     sqrt(A_ii - dp), the same sqrt and division under the same flags as k_ichol0_numeric.  A negative or zero pivot is no error: the
//     NaN / Inf that follows is what the single constructor gives, bit for bit.
//
// Rows run side by side in the idiom of refactor_rows (ilu0_batch.hip) and batch_sweep (sptrsv_batch.hip): one lane per row (rows t,
// t + 256, ...: a lane's rows ascend, so the member's lowest unfinished row is always somebody's current row), every lane retries its
// pending pivot row once per trip of its wave, no lane blocks inside divergent code.  A finished row is published by a workgroup-scope
// RELEASE store of its flag in LDS behind its value stores; a consumer ACQUIRES the flag before it reads row j.  Nothing crosses a CU
// and members share nothing.  Waits are bounded by the workgroup's progress counter and an idle limit; a wave that gives up sets status
// 2 and the others leave.
//
// The working row lives in LDS per lane: per entry of L's row its column, its value and -- for the entries below the diagonal -- where
// pivot row j starts in L and how long it is without its diagonal (pattern only: fetched when the row is opened, before any flag is
// waited for).  Row j's indices and values come kRG at a time with their loads in flight together.  The row's values are stored to lval
// once, then the flag is released; AFTER the release, off the dependency chain of the rows that wait for this one, the same lane writes
// each value into the transposed copy: entry (r, c) is found by binary search for r in tidx[tptr[c] .. tptr[c + 1]), kRG searches in
// lock step.
//
// ROW CAP.  A working entry takes 20 bytes per lane: 5 120 bytes per entry of L's longest row behind the 4 n bytes of flags, and both
// must fit into the LDS a workgroup may have (160 KiB less the kernels' static words): longest row of L <= (cap - 4 n) / 5 120 and never
// above kRfMaxRow = 31 -- 28 entries at n = 4 000, 16 at n = 20 000, the caps of the ILU(0) launch, but counted on L's rows, which are
// about half of A's.  A member above it is not launched (route 1: ichol0_refactor_batch_fits).
//
// FIRST CONSTRUCTION: k_ichol0_symbolic_batch reads A's pattern (extents before anything is read through them, column indices strictly
// ascending inside [0, n), the diagonal present), counts the entries with column <= r and writes L's row pointers with a workgroup-wide
// running scan; CreateInfo: nnz_l = entries of L, nnz_u = 0, max_row_len = L's longest row.  k_ichol0_create_batch, once the host has
// allocated the exact arrays: L's indices in k_tri_fill's layout, a workgroup barrier, then pass 2 through the same device function.
#include <limits.h>

#include "common.h"
#include "refactor_batch.h"

namespace ilupp {

// a * b with a as the multiply's FIRST source operand.  Where both operands are NaNs of different bits (behind a zero pivot: 0 / 0, Inf - Inf,
// sqrt of a negative number) the instruction hands on the first one's, and the compiler commutes a plain product as it likes: it did, against
// k_ichol0_numeric's W(a) * val[b] (seen in the ISA of both), and behind a zero pivot the two factors' NaNs were not the same bits.  (Finite
// products do not depend on the order.)
__device__ __forceinline__ double mul_in_order(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return a * b;
#endif
}

// pass 2 for one member; the working rows in LDS (wv, wc, wk0, wkl: entry q of this lane at [q * 256 + tid])
__device__ __forceinline__ void ichol0_rows(const RefactorDesc &d, int *rf_done, double *wv, int *wc, int *wk0, int *wkl,
                                            unsigned *s_progress, int *s_fail)
{
    const int n = d.n, tid = threadIdx.x;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr, lidx = (rf_cint)d.lidx;
    const rf_cint tptr = (rf_cint)d.uptr, tidx = (rf_cint)d.uidx;
    const rf_cdbl aval = (rf_cdbl)d.aval;
    const rf_dbl lval = (rf_dbl)d.lval, tval = (rf_dbl)d.uval;      // (lval: written by one lane, read by others)
    const bool haveT = d.uptr != nullptr && d.uidx != nullptr && d.uval != nullptr;
    constexpr unsigned kIdleLimit = 1u << 20;       // trips of a wave without progress anywhere in the workgroup, as batch_sweep
    unsigned seen = 0, idle = 0;
    int r = tid;
    bool alive = r < n, need_init = true;
    int len = 0, l0 = 0, p = 0;
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
            if (need_init) {                                                    // row i of A's lower triangle (IChol.hpp:47)
                const int a0 = aptr[r], alen = aptr[r + 1] - a0;
                l0 = lptr[r]; len = lptr[r + 1] - l0;
                int k = 0;
                // (kRG entries' loads in flight together; a sorted row ends the walk within a group of its diagonal)
                for (int q0 = 0; q0 < alen && k < len; q0 += kRG) {
                    int c[kRG];
                    double v[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < alen) { c[q] = aidx[a0 + q0 + q]; v[q] = aval[a0 + q0 + q]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (q0 + q < alen && c[q] <= r && k < len) { wc[k * kRfThreads + tid] = c[q]; wv[k * kRfThreads + tid] = v[q]; ++k; }
                }
                if (k != len) {
                    // (the matrix is no longer the one the proof read: nothing is reached through a working row that is not there)
                    __hip_atomic_store(s_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    len = 0;                                                    // (no step below runs on it)
                    alive = false;
                }
                for (int q0 = 0; q0 < len - 1; q0 += kRG) {
                    int b[kRG], e[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < len - 1) { const int j = wc[(q0 + q) * kRfThreads + tid]; b[q] = lptr[j]; e[q] = lptr[j + 1]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (q0 + q < len - 1) { wk0[(q0 + q) * kRfThreads + tid] = b[q]; wkl[(q0 + q) * kRfThreads + tid] = e[q] - b[q] - 1; }
                }
                p = 0;
                need_init = false;
                did = true;
            }
            while (p < len - 1) {                                               // the entries below the diagonal (IChol.hpp:49-51)
                const int j = col(p);
                if (__hip_atomic_load(&rf_done[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) break;      // row j not finished: next trip
                const int j0 = wk0[p * kRfThreads + tid], kl = wkl[p * kRfThreads + tid];      // row j without its diagonal
                const double L_jj = lval[j0 + kl];                              // the diagonal is the last entry of row j
                double dp = 0.0;                                                // sparse_dot_product (IChol.hpp:16-28)
                int a = 0;
                bool stop = false;
                for (int jb = 0; jb < kl && !stop; jb += kRG) {                 // kRG entries' loads together
                    int m[kRG];
                    double u[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (jb + q < kl) { m[q] = lidx[j0 + jb + q]; u[q] = lval[j0 + jb + q]; }
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (jb + q < kl && !stop) {
                            while (a < len - 1 && col(a) < m[q]) ++a;           // (row i without its diagonal)
                            if (a >= len - 1) {
                                stop = true;
                            } else if (col(a) == m[q]) {
                                const double pr = mul_in_order(wget(a), u[q]);      // W(a) * val[b], as k_ichol0_numeric's ISA has it
                                dp = dp + pr;
                                ++a;
                            }
                        }
                }
                wset(p, (wget(p) - dp) / L_jj);
                ++p;
                did = true;
            }
            if (p == len - 1) {
                double dp = 0.0;                                                // the row with itself, without the diagonal (IChol.hpp:52-53)
                for (int a = 0; a < len - 1; ++a) { const double w = wget(a); const double pr = w * w; dp = dp + pr; }
                wset(p, sqrt(wget(p) - dp));
                for (int q = 0; q < len; ++q) lval[l0 + q] = wget(q);
                __hip_atomic_store(&rf_done[r], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);      // behind the row's value stores
                if (haveT) {
                    // the transposed copy, off the chain: value (r, c) goes to where row c of LcT names row r
                    for (int q0 = 0; q0 < len; q0 += kRG) {
                        int lo[kRG], hi[kRG], end[kRG];
#pragma unroll
                        for (int q = 0; q < kRG; ++q) {
                            lo[q] = hi[q] = end[q] = 0;
                            if (q0 + q < len) { const int c = col(q0 + q); lo[q] = tptr[c]; hi[q] = end[q] = tptr[c + 1]; }
                        }
                        for (int it = 0; it < 32; ++it) {                       // (an extent is below 2^31: 31 halvings at the most)
                            int mid[kRG], t[kRG];
                            bool any = false;
#pragma unroll
                            for (int q = 0; q < kRG; ++q) if (lo[q] < hi[q]) { mid[q] = lo[q] + ((hi[q] - lo[q]) >> 1); t[q] = tidx[mid[q]]; any = true; }
                            if (!any) break;
#pragma unroll
                            for (int q = 0; q < kRG; ++q) if (lo[q] < hi[q]) { if (t[q] < r) lo[q] = mid[q] + 1; else hi[q] = mid[q]; }
                        }
#pragma unroll
                        for (int q = 0; q < kRG; ++q)
                            if (q0 + q < len && lo[q] < end[q] && tidx[lo[q]] == r) tval[lo[q]] = wget(q0 + q);
                    }
                }
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
// lanes' working rows, the rows factored, the member's status word written.  What k_ichol0_refactor_batch and k_ichol0_create_batch share.
__device__ __forceinline__ void ichol0_member(const RefactorDesc &d, unsigned char *rf_lds, unsigned lds_bytes, int maxlen, int32_t *status,
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
    ichol0_rows(d, rf_done, wv, wc, wk0, wkl, s_progress, s_fail);
    __syncthreads();
    if (tid == 0) status[d.member] = *s_fail != 0 ? 2 : 0;
}

// row r of the proof: A's stored entries with column <= r, in stored order, are L's row lidx[l0 .. l0 + len), strictly ascending with the
// diagonal last (the extents a0 <= a1 are checked by the caller)
template <class AI, class LI>
__device__ __forceinline__ bool ichol0_row_differs(AI aidx, int a0, int a1, LI lidx, int l0, int len, int r)
{
    bool bad = false;
    int k = 0, prev = -1;
    for (int q0 = a0; q0 < a1; q0 += kRG) {          // (kRG entries' loads in flight together)
        int c[kRG];
#pragma unroll
        for (int q = 0; q < kRG; ++q) if (q0 + q < a1) c[q] = aidx[q0 + q];
#pragma unroll
        for (int q = 0; q < kRG; ++q)
            if (q0 + q < a1 && c[q] <= r) {
                if (k < len) bad |= lidx[l0 + k] != c[q];
                bad |= c[q] <= prev;
                prev = c[q];
                ++k;
            }
    }
    return bad || k != len || prev != r;
}

__global__ void __launch_bounds__(kRfThreads)
k_ichol0_refactor_batch(const RefactorDesc *__restrict__ table, int32_t *__restrict__ status, const unsigned lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail, s_bad, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    int *rf_done = reinterpret_cast<int *>(rf_lds);                             // row r of the member is finished (its values are stored to lval)
    if (tid == 0) { s_progress = 0; s_fail = 0; s_maxlen = 0; s_bad = (int64_t)d.aptr[n] != d.nnzA ? 1 : 0; }
    for (int i = tid; i < n; i += kRfThreads) rf_done[i] = 0;

    // ---- pass 1: the proof ----
    bool bad = false;
    int maxlen = 0;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr, lidx = (rf_cint)d.lidx;
    for (int r = tid; r < n; r += kRfThreads) {
        const int a0 = aptr[r], a1 = aptr[r + 1];
        const int l0 = lptr[r], len = lptr[r + 1] - l0;
        if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA || len < 1) { bad = true; continue; }
        bad |= ichol0_row_differs(aidx, a0, a1, lidx, l0, len, r);
        maxlen = max(maxlen, len);
    }
    __syncthreads();                                 // (thread 0's words and the flags are there)
    if (bad) __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (s_bad != 0) {
        if (tid == 0) status[d.member] = 1;          // (one writer per member: its own word; nothing else was written)
        return;
    }

    ichol0_member(d, rf_lds, lds_bytes, s_maxlen, status, &s_progress, &s_fail);
}

// ---- first construction: the symbolic launch ----
__global__ void __launch_bounds__(kRfThreads)
k_ichol0_symbolic_batch(const RefactorDesc *__restrict__ table, CreateInfo *__restrict__ info)
{
    __shared__ int s_wl[kRfThreads / 64];                                       // the waves' totals of one round of the scan
    __shared__ int s_missing, s_flags, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx;
    const rf_int lptr = (rf_int)d.lptr;
    if (tid == 0) { s_missing = INT_MAX; s_flags = 0; s_maxlen = 0; lptr[0] = 0; }
    bool bad = false;
    int maxlen = 0, missing = INT_MAX;
    int carry_l = 0;                                 // entries of L in the rows of the rounds before
    for (int base = 0; base < n; base += kRfThreads) {
        const int r = base + tid;
        int nl = 0;                                  // row r's entries in L: column <= r
        if (r < n) {
            const int a0 = aptr[r], a1 = aptr[r + 1];
            if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA) {
                bad = true;                          // (nothing is read through such extents)
            } else {
                const int len = a1 - a0;
                int prev = -1;
                bool diag = false;
                for (int q0 = 0; q0 < len; q0 += kRG) {      // (kRG entries' loads in flight together)
                    int c[kRG];
#pragma unroll
                    for (int q = 0; q < kRG; ++q) if (q0 + q < len) c[q] = aidx[a0 + q0 + q];
#pragma unroll
                    for (int q = 0; q < kRG; ++q)
                        if (q0 + q < len) {
                            bad |= c[q] <= prev || c[q] >= n;              // (prev >= -1: a negative index is caught too)
                            nl += c[q] <= r ? 1 : 0;
                            diag |= c[q] == r;
                            prev = c[q];
                        }
                }
                if (!diag) missing = min(missing, r);
                maxlen = max(maxlen, nl);
            }
        }
        int xl = nl;                                 // inclusive scan over the wave, then over the waves' totals
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int tl = __shfl_up(xl, off);
            if (lane >= off) xl += tl;
        }
        if (lane == 63) s_wl[w] = xl;
        __syncthreads();
        int before_l = 0, all_l = 0;
#pragma unroll
        for (int k = 0; k < kRfThreads / 64; ++k) {
            if (k < w) before_l += s_wl[k];
            all_l += s_wl[k];
        }
        if (r < n) lptr[r + 1] = carry_l + before_l + xl;
        carry_l += all_l;
        __syncthreads();                             // (the totals are read: the next round may write them)
    }
    if (bad) atomicOr(&s_flags, kCreateUnsorted);
    atomicMin(&s_missing, missing);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();
    if (tid == 0) {
        CreateInfo o;
        o.nnz_l = carry_l; o.nnz_u = 0; o.max_row_len = s_maxlen;
        o.missing = s_missing == INT_MAX ? -1 : s_missing;
        o.flags = s_flags | ((int64_t)aptr[n] != d.nnzA ? kCreateNnzDiffers : 0);
        o.pad[0] = o.pad[1] = o.pad[2] = 0;
        info[blockIdx.x] = o;
    }
}

// ---- first construction: the pattern, then the factorisation ----
__global__ void __launch_bounds__(kRfThreads)
k_ichol0_create_batch(const RefactorDesc *__restrict__ table, int32_t *__restrict__ status, const unsigned lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail, s_bad, s_maxlen;
    const RefactorDesc d = table[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    int *rf_done = reinterpret_cast<int *>(rf_lds);
    if (tid == 0) { s_progress = 0; s_fail = 0; s_maxlen = 0; s_bad = 0; }
    for (int i = tid; i < n; i += kRfThreads) rf_done[i] = 0;
    const rf_cint aptr = (rf_cint)d.aptr, aidx = (rf_cint)d.aidx, lptr = (rf_cint)d.lptr;
    const rf_int lidx = (rf_int)d.lidx;
    bool bad = false;
    int maxlen = 0;
    for (int r = tid; r < n; r += kRfThreads) {
        const int a0 = aptr[r], a1 = aptr[r + 1];
        const int l0 = lptr[r], len = lptr[r + 1] - l0;
        // (the row pointers are the symbolic launch's; a matrix that is no longer the one it read writes nothing outside its rows)
        if (a0 < 0 || a1 < a0 || (int64_t)a1 > d.nnzA || len < 1) { bad = true; continue; }
        int k = 0, prev = -1;
        for (int q0 = a0; q0 < a1; q0 += kRG) {      // (kRG entries' loads in flight together)
            int c[kRG];
#pragma unroll
            for (int q = 0; q < kRG; ++q) if (q0 + q < a1) c[q] = aidx[q0 + q];
#pragma unroll
            for (int q = 0; q < kRG; ++q)
                if (q0 + q < a1 && c[q] <= r) {      // what k_tri_fill keeps, in stored order
                    if (k < len) lidx[l0 + k] = c[q];
                    bad |= c[q] <= prev;             // (ascending from 0 on: the pivot rows pass 2 reads through these exist)
                    prev = c[q];
                    ++k;
                }
        }
        bad |= k != len || prev != r;
        maxlen = max(maxlen, len);
    }
    __syncthreads();                                 // (thread 0's words and the flags are there)
    if (bad) __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    atomicMax(&s_maxlen, maxlen);
    __syncthreads();                                 // (... and the pattern, for the workgroup's other waves: ichol0_rows reads lidx of other lanes' rows)
    if (s_bad != 0) {
        if (tid == 0) status[d.member] = 1;
        return;
    }
    ichol0_member(d, rf_lds, lds_bytes, s_maxlen, status, &s_progress, &s_fail);
}

// ---- the single re-factorisation's first step, rows over the chip: the proof, then L.val = A's lower-triangle values ----
__global__ void k_ichol0_refill_proof(int32_t n, int64_t nnzA, const int32_t *__restrict__ aptr, const int32_t *__restrict__ aidx,
                                      const int32_t *__restrict__ lptr, const int32_t *__restrict__ lidx, int32_t *__restrict__ bad_out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    bool bad = r == 0 && (int64_t)aptr[n] != nnzA;
    const int a0 = aptr[r], a1 = aptr[r + 1];
    const int l0 = lptr[r], len = lptr[r + 1] - l0;
    if (a0 < 0 || a1 < a0 || (int64_t)a1 > nnzA || len < 1) bad = true;
    else bad |= ichol0_row_differs(aidx, a0, a1, lidx, l0, len, r);
    if (bad) atomicExch(bad_out, 1);
}

__global__ void k_ichol0_refill(int32_t n, const int32_t *__restrict__ aptr, const int32_t *__restrict__ aidx, const double *__restrict__ aval,
                                const int32_t *__restrict__ lptr, double *__restrict__ lval)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int o = lptr[r];
    const int end = lptr[r + 1];
    for (int q = aptr[r]; q < aptr[r + 1] && o < end; ++q)
        if (aidx[q] <= r) lval[o++] = aval[q];
}

int ichol0_refill_proof(hipStream_t st, int32_t n, int64_t nnzA, const int32_t *aptr, const int32_t *aidx, const DevMat &L, int32_t *d_bad)
{
    ILUPP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_ichol0_refill_proof, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, nnzA, aptr, aidx, L.ptr, L.idx, d_bad);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

int ichol0_refill(hipStream_t st, int32_t n, const int32_t *aptr, const int32_t *aidx, const double *aval, DevMat *L)
{
    hipLaunchKernelGGL(k_ichol0_refill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, aptr, aidx, aval, L->ptr, L->val);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// bytes of dynamic LDS one workgroup of k_ichol0_refactor_batch may take on the current device
// (... and of k_ichol0_create_batch, which has the same static words: the smaller of the two, so that one routing serves both launches)
static size_t ichol0_refactor_batch_lds_cap()
{
    const size_t a = kernel_lds_cap<k_ichol0_refactor_batch>(), b = kernel_lds_cap<k_ichol0_create_batch>();
    return a < b ? a : b;
}

// the largest n of a member of the launch: its flags and working rows of kRfMinRow entries fit (a member of that n with longer rows does not)
static constexpr int kRfMinRow = 8;
int64_t ichol0_refactor_batch_max_n()
{
    const size_t cap = ichol0_refactor_batch_lds_cap(), rows = (size_t)kRfMinRow * kRfRowBytes;
    return cap > rows + 8 ? (int64_t)((cap - rows) / sizeof(int)) - 1 : 0;
}

// the bytes of LDS a member of n rows whose factor's longest row has max_row_len entries asks of the launch (flags + working rows), or 0
// when it is above the row cap: max_row_len > kRfMaxRow, or flags and rows do not fit into the LDS a workgroup may have
size_t ichol0_refactor_batch_fits(int32_t n, int32_t max_row_len)
{
    if (max_row_len < 1 || max_row_len > kRfMaxRow) return 0;
    const size_t want = rf_flag_bytes(n) + (size_t)max_row_len * kRfRowBytes;
    return want <= ichol0_refactor_batch_lds_cap() ? want : 0;
}

// `count` members, one workgroup each; lds_bytes: the largest ichol0_refactor_batch_fits among them; member k's status goes to d_status[table[k].member]
int ichol0_refactor_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, int32_t *d_status, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > ichol0_refactor_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_ichol0_refactor_batch, dim3((unsigned)count), dim3(kRfThreads), lds_bytes, st, d_table, d_status, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// the symbolic launch of a batched first construction: member k's record goes to d_info[k]
int ichol0_symbolic_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, CreateInfo *d_info)
{
    if (count <= 0) return ILUPP_OK;
    hipLaunchKernelGGL(k_ichol0_symbolic_batch, dim3((unsigned)count), dim3(kRfThreads), 0, st, d_table, d_info);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// its create launch: as ichol0_refactor_batch_launch (status 1: the matrix is not the one the symbolic launch read)
int ichol0_create_batch_launch(hipStream_t st, int32_t count, const RefactorDesc *d_table, int32_t *d_status, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > ichol0_refactor_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_ichol0_create_batch, dim3((unsigned)count), dim3(kRfThreads), lds_bytes, st, d_table, d_status, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
