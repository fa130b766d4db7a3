// ilupp_amd/csrc/sptrsv_batch.hip -- the whole apply of MANY pivoting preconditioners (ILUCP / ILUTP objects) in ONE launch: one workgroup per
// member, the permutation and both sweeps inside that workgroup, the unknowns in LDS.
//
// One apply of such an object is a latency chain, not a bandwidth problem: two sweeps whose rows wait for each other, a gather or a scatter
// through the pivoting permutation, and the launches and hand-overs around them.  Alone it leaves 255 of the chip's 256 CUs idle; a batch of
// members (one per system that is being solved) fills them.  Each sweep is k_sptrsv_small's algorithm (sptrsv_small.hip): one lane per row
// (rows t, t + 256, ...; backwards from the last row for the backward kinds), the unknowns in an LDS array that starts all-sentinel (the data
// is the flag), a row's off-diagonal entries consumed strictly in the order of its sweep kind as their unknowns appear, acc = acc - val * x as a separate
// multiply and subtract, one division by the diagonal found by position -- the reference's arithmetic (triangular_solve,
// sparse_implementation.h:4040-4087, and the permuted solves :4196-4218), hence its bits.  No lane ever blocks.
//
// The two orders of ilupp_hip_ilucp_apply:
//   plain first:   t = sweep2(sweep1(x));  x[perm[k]] = t[k]     -- the permutation is folded into the second sweep's store
//   gather first:  y[i] = x[perm[i]];      x = sweep2(sweep1(y)) -- the permutation is folded into the first sweep's right-hand-side read
// In place without a hazard: every read of the member's vector is the right-hand side of a row of the FIRST sweep (open_row, whose value the
// row's division consumes before the row is stored), every write of it is the store of a row of the SECOND sweep, and a workgroup barrier
// that every wave passes only when all its rows of the first sweep are stored stands between the two; a member that gives up in its first
// sweep never starts the second and leaves its vector as it was.
//
// Between the sweeps the first one's result is the second one's right-hand side: it stays in LDS (a second array for the second sweep's
// unknowns) when 16 n bytes fit into the launch's dynamic LDS; otherwise the first sweep also writes its rows to the member's `tmp` in HBM,
// the barrier makes them visible to the workgroup (one CU, one L1), the ONE LDS array is filled with sentinels again and the second sweep
// reads its right-hand sides from `tmp`.
#include "common.h"

namespace ilupp {

static constexpr int kBatchThreads = 256;      // one wave per SIMD, as k_sptrsv_small
static constexpr int kBG = 8;                  // entries of a row held in one register group

// One sweep of the member by the whole workgroup.  SWEEP_FWD_LAST_ASC: rows ascending, the diagonal LAST in the row, the entries before
// it first-to-last; SWEEP_BWD_FIRST_ASC: rows descending, the diagonal FIRST, the entries behind it first-to-last; SWEEP_BWD_FIRST_DESC:
// the same storage with those entries taken last-to-first (the reference's scatter loop T4 read as a gather, sptrsv.hip).
// Right-hand side of row r: rlds[r] when rlds is given, else rsrc[rmap ? rmap[r] : r].  The unknown goes to xs[r] (LDS) and, when odst is
// given, to odst[omap ? omap[r] : r].  Every wave leaves through the barrier at the end; *s_fail is set when a wave gave up.
__device__ __forceinline__ void batch_sweep(const int kind, const int n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                            const double *__restrict__ val, unsigned long long *xs, const unsigned long long *rlds,
                                            const double *rsrc, const int32_t *__restrict__ rmap, double *odst,
                                            const int32_t *__restrict__ omap, unsigned *s_progress, int *s_fail)
{
    const int tid = threadIdx.x;
    const bool fwd = kind == SWEEP_FWD_LAST_ASC;
    const int step = kind == SWEEP_BWD_FIRST_DESC ? -1 : 1;
    for (int i = tid; i < n; i += kBatchThreads) xs[i] = kSentinel;
    __syncthreads();
    int r = fwd ? tid : n - 1 - tid;                // this lane's current row
    bool alive = fwd ? r < n : r >= 0;
    int j = 0, jend = 0, jf = 0;                    // the off-diagonal entries of the row in the order they are taken, entry k at base + step * k: [j, jend) still to consume; fetched up to jf
    int base = 0;
    double acc = 0.0, diag = 1.0;
    // two groups of entries in registers: one is consumed while the other one's loads are in flight
    int c0[kBG] = {0}, c1[kBG] = {0};
    double v0[kBG] = {0.0}, v1[kBG] = {0.0};
    int have0 = 0, have1 = 0, at = 0;
    auto fetch1 = [&]() {                           // the next group into c1 / v1
        have1 = jend - jf < kBG ? jend - jf : kBG;
#pragma unroll
        for (int q = 0; q < kBG; ++q) if (q < have1) { c1[q] = idx[base + step * (jf + q)]; v1[q] = val[base + step * (jf + q)]; }
        jf += have1;
    };
    // Bounded waits as in k_sptrsv_small: a wave gives up only when NO wave of the workgroup has made progress for kIdleLimit of its own
    // trips (or a row has no diagonal, or another wave has given up already).
    constexpr unsigned kIdleLimit = 1u << 20;
    unsigned seen = 0, idle = 0;
    bool broken = false;
    auto open_row = [&]() {
        const int b = ptr[r], e = ptr[r + 1];
        if (e <= b) { broken = true; return; }      // (a row without its diagonal: nothing to divide by)
        j = 0; jend = e - b - 1;
        if (fwd) { base = b; diag = val[e - 1]; }
        else { base = step > 0 ? b + 1 : e - 1; diag = val[b]; }
        acc = rlds ? __longlong_as_double((long long)rlds[r]) : rsrc[rmap ? rmap[r] : r];
        jf = 0;
        have0 = jend < kBG ? jend : kBG;
#pragma unroll
        for (int q = 0; q < kBG; ++q) if (q < have0) { c0[q] = idx[base + step * q]; v0[q] = val[base + step * q]; }
        jf = have0;
        at = 0;
        fetch1();
    };
    if (alive) open_row();
    while (__ballot(alive) != 0ull) {
        if (__ballot(broken) != 0ull || idle > kIdleLimit) {
            if ((tid & 63) == 0) __hip_atomic_store(s_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            break;
        }
        bool did = false;
        if (alive) {
            if (j < jend) {
                if (at == have0) {                  // the group is used up: the other one takes its place, the one after it is asked for
#pragma unroll
                    for (int q = 0; q < kBG; ++q) { c0[q] = c1[q]; v0[q] = v1[q]; }
                    have0 = have1; at = 0;
                    fetch1();
                }
                // as many entries of the group as have their unknown, in the order they are taken
                unsigned long long xb[kBG];
#pragma unroll
                for (int q = 0; q < kBG; ++q)
                    xb[q] = (q >= at && q < have0) ? __hip_atomic_load(&xs[c0[q]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kSentinel;
#pragma unroll
                for (int q = 0; q < kBG; ++q)
                    if (q == at && q < have0 && xb[q] != kSentinel) {
                        const double p = v0[q] * __longlong_as_double((long long)xb[q]);
                        acc = acc - p;
                        ++at; ++j;
                        did = true;
                    }
            } else {
                const double x = acc / diag;
                __hip_atomic_store(&xs[r], (unsigned long long)__double_as_longlong(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (odst) odst[omap ? omap[r] : r] = x;
                r += fwd ? kBatchThreads : -kBatchThreads;
                alive = fwd ? r < n : r >= 0;
                if (alive) open_row();
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
    __syncthreads();
}

__global__ void __launch_bounds__(kBatchThreads)
k_pivot_apply_batch(const PivotApplyDesc *__restrict__ table, double *xbase, const unsigned lds_bytes)
{
    extern __shared__ unsigned long long lds[];     // the unknowns of a sweep, sentinel = not yet: one array of n, or two
    __shared__ unsigned s_progress;
    __shared__ int s_fail;
    const PivotApplyDesc d = table[blockIdx.x];
    const int n = d.n;
    if (threadIdx.x == 0) { s_progress = 0; s_fail = 0; }
    // (the first sweep's fill-and-barrier publishes the two words before any wave looks at them)
    double *x = xbase + d.xoff;
    const bool two = (size_t)16 * (size_t)n <= (size_t)lds_bytes;
    // first sweep: right-hand sides from the member's vector (through perm when the gather comes first)
    batch_sweep(d.kind1, n, d.ptr1, d.idx1, d.val1, lds, nullptr, x, d.plain_first ? nullptr : d.perm, two ? nullptr : d.tmp, nullptr,
                &s_progress, &s_fail);
    if (s_fail == 0) {
        // second sweep: right-hand sides = the first one's unknowns; its store is the member's vector (through perm when the plain solve came first)
        batch_sweep(d.kind2, n, d.ptr2, d.idx2, d.val2, two ? lds + n : lds, two ? lds : nullptr, d.tmp, nullptr, x,
                    d.plain_first ? d.perm : nullptr, &s_progress, &s_fail);
    }
    if (threadIdx.x == 0) *d.err = s_fail;          // (one writer per member: its own word, whatever the other members do)
}

// bytes of dynamic LDS one workgroup of k_pivot_apply_batch may take on the current device: what the device gives a workgroup minus the
// kernel's static words; the kernel is told once per device that it may ask for that much
size_t pivot_apply_batch_lds_cap()
{
    static thread_local int cap_dev = -1;
    static thread_local size_t cap = 0;
    int dev = 0;
    ILUPP_HIP(hipGetDevice(&dev));
    if (cap_dev != dev) {
        int max_lds = 0;
        ILUPP_HIP(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        hipFuncAttributes fa;
        ILUPP_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_pivot_apply_batch)));
        const size_t room = (size_t)max_lds > fa.sharedSizeBytes ? (size_t)max_lds - fa.sharedSizeBytes : 0;
        ILUPP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pivot_apply_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)room));
        cap = room;
        cap_dev = dev;
    }
    return cap;
}

// `count` members, one workgroup each; member i's vector is d_x + table[i].xoff; lds_bytes for every workgroup (<= the cap)
int pivot_apply_batch_launch(hipStream_t st, int32_t count, const PivotApplyDesc *d_table, double *d_x, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > pivot_apply_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_pivot_apply_batch, dim3((unsigned)count), dim3(kBatchThreads), lds_bytes, st, d_table, d_x, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
