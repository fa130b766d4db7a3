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
//
// The non-pivoting classes (ILU0, ILUT, ILUC, IChol0, ICholT) take the same launch: a descriptor with perm == nullptr is an apply without a
// permutation, its two triangles those of apply_plan / sweep_parts (api_batch.hip: batch_describe).
//
// Two more kernels further down, each one workgroup per system with this apply (apply_member) inside its loop: k_bicgstab_batch, the whole
// left-preconditioned BiCGstab SOLVE of many small systems in one launch, and k_cg_batch, the whole preconditioned CG solve of many small
// symmetric positive definite systems.  Both take members of every class above, pivoting or not, or without a preconditioner, mixed in
// one launch.
//
// Between the apply's kernel and the two solvers: k_ml_apply_batch, the whole apply of MANY multilevel ILU++ preconditioners in one launch -- one workgroup per
// member walks ml_apply_dev (api_ml.hip) statement for statement: pass 0 upwards through the member's levels, pass 1 downwards, every level
// on the LAST n_l entries of the member's vector, each step a scale / permute into right-hand sides, ONE sweep of the level's object
// (batch_sweep above, the unknowns in the one LDS array of n_0), and a take / permute back into the tail.
// In place without a hazard: a level's gather reads entries of the tail that its take overwrites later, so a step never writes the tail
// while it is being read -- (1) EVERY right-hand side of the step is written to the member's scratch `tmp` in HBM (n doubles of the
// object's own, and an object is a member at most once per call) before (2) a workgroup barrier, behind which nothing reads the tail until
// (3) the sweep, which reads `tmp` and writes LDS only, has passed its closing barrier; (4) the take then reads LDS (through the
// permutation) and writes the tail, every lane its own entries, and (5) a second barrier ends the step: the next step's gather reads the
// finished tail, its sweep refills an LDS array nobody reads any more, and its right-hand sides overwrite a `tmp` whose readers have left
// the sweep.  One CU and one L1 touch vector and scratch.  A member whose sweep gives up stops there: its vector is unspecified.
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

// The apply of one member by its workgroup, dst = M^-1 src; in place when dst == src (see the file's header), else src is left as it is.
// `arr` holds lds_bytes of LDS for the sweeps' unknowns.  *s_fail != 0 afterwards: a sweep gave up (a member that gives up in its first
// sweep never starts the second and leaves dst as it was).
__device__ __forceinline__ void apply_member(const PivotApplyDesc &d, const double *src, double *dst, unsigned long long *arr,
                                             const unsigned lds_bytes, unsigned *s_progress, int *s_fail)
{
    const int n = d.n;
    const bool two = (size_t)16 * (size_t)n <= (size_t)lds_bytes;
    // first sweep: right-hand sides from src (through perm when the gather comes first)
    batch_sweep(d.kind1, n, d.ptr1, d.idx1, d.val1, arr, nullptr, src, d.plain_first ? nullptr : d.perm, two ? nullptr : d.tmp, nullptr,
                s_progress, s_fail);
    if (*s_fail == 0) {
        // second sweep: right-hand sides = the first one's unknowns; its store is dst (through perm when the plain solve came first)
        batch_sweep(d.kind2, n, d.ptr2, d.idx2, d.val2, two ? arr + n : arr, two ? arr : nullptr, d.tmp, nullptr, dst,
                    d.plain_first ? d.perm : nullptr, s_progress, s_fail);
    }
}

__global__ void __launch_bounds__(kBatchThreads)
k_pivot_apply_batch(const PivotApplyDesc *__restrict__ table, double *xbase, const unsigned lds_bytes)
{
    extern __shared__ unsigned long long lds[];     // the unknowns of a sweep, sentinel = not yet: one array of n, or two
    __shared__ unsigned s_progress;
    __shared__ int s_fail;
    const PivotApplyDesc d = table[blockIdx.x];
    if (threadIdx.x == 0) { s_progress = 0; s_fail = 0; }
    // (the first sweep's fill-and-barrier publishes the two words before any wave looks at them)
    double *x = xbase + d.xoff;
    apply_member(d, x, x, lds, lds_bytes, &s_progress, &s_fail);
    if (threadIdx.x == 0) *d.err = s_fail;          // (one writer per member: its own word, whatever the other members do)
}

// bytes of dynamic LDS one workgroup of k_pivot_apply_batch may take on the current device
size_t pivot_apply_batch_lds_cap() { return kernel_lds_cap<k_pivot_apply_batch>(); }

// `count` members, one workgroup each; member i's vector is d_x + table[i].xoff; lds_bytes for every workgroup (<= the cap)
int pivot_apply_batch_launch(hipStream_t st, int32_t count, const PivotApplyDesc *d_table, double *d_x, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > pivot_apply_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_pivot_apply_batch, dim3((unsigned)count), dim3(kBatchThreads), lds_bytes, st, d_table, d_x, (unsigned)lds_bytes);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

// ---- the whole apply of MANY multilevel ILU++ preconditioners in ONE launch: one workgroup per member ---------------------------------
// The apply of one member by its workgroup, in place on x (n doubles): ml_apply_dev of api_ml.hip with the element operations of ml.hip's
// vector kernels in their exact form -- a division stays a division, a multiply a separate multiply -- and batch_sweep for the sweeps, so
// the member has the bits of its single apply.  lv: the member's level records; arr: 8 n bytes of LDS.  The hazards: the file's header.
// *s_fail != 0 afterwards: a sweep gave up and the member stopped there.
__device__ __forceinline__ void ml_apply_member(const MlApplyDesc &d, const MlLevelDesc *__restrict__ lv, double *x, unsigned long long *arr,
                                                unsigned *s_progress, int *s_fail)
{
    const int tid = threadIdx.x;
    const bool tr = d.transpose != 0;
    double *rhs = d.tmp;
    for (int pass = 0; pass < 2; ++pass) {
        for (int s = 0; s < d.levels; ++s) {
            const MlLevelDesc l = lv[pass == 0 ? s : d.levels - 1 - s];
            const int n = l.n;
            double *xt = x + (d.n - n);
            if (pass == 0) {                   // ID: x /= D_l, permute_first(perm_rows); TRANSPOSE: x /= D_r, permute_first(perm_columns)
                const double *Dg = tr ? l.Dr : l.Dl;
                for (int i = tid; i < n; i += kBatchThreads) { const int g = l.gather[i]; rhs[i] = xt[g] / Dg[g]; }
            } else if (!tr) {                  // ID: x *= D
                for (int i = tid; i < n; i += kBatchThreads) rhs[i] = xt[i] * l.D[i];
            } else {
                for (int i = tid; i < n; i += kBatchThreads) rhs[i] = xt[i];
            }
            __syncthreads();
            // (one call for both passes: the inlined sweep stands in the code once)
            batch_sweep(pass == 0 ? l.kind1 : l.kind2, n, pass == 0 ? l.ptr1 : l.ptr2, pass == 0 ? l.idx1 : l.idx2, pass == 0 ? l.val1 : l.val2,
                        arr, nullptr, rhs, nullptr, nullptr, nullptr, s_progress, s_fail);
            if (*s_fail != 0) return;          // (uniform: read behind the sweep's closing barrier, and nobody writes it outside a sweep)
            if (pass == 0) {                   // ID: x = w; TRANSPOSE: x = w * D
                for (int i = tid; i < n; i += kBatchThreads) {
                    const double v = __longlong_as_double((long long)arr[i]);
                    xt[i] = tr ? v * l.D[i] : v;
                }
            } else {                           // ID: permute_last(inverse_perm_columns), x /= D_r; TRANSPOSE: permute_last(inverse_perm_rows), x /= D_l
                const double *Dt = tr ? l.Dl : l.Dr;
                for (int i = tid; i < n; i += kBatchThreads) xt[i] = __longlong_as_double((long long)arr[l.take[i]]) / Dt[i];
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kBatchThreads)
k_ml_apply_batch(const MlApplyDesc *__restrict__ table, const MlLevelDesc *__restrict__ levels, double *xbase)
{
    extern __shared__ unsigned long long lds[];     // the unknowns of a sweep, sentinel = not yet: one array of n_0
    __shared__ unsigned s_progress;
    __shared__ int s_fail;
    const MlApplyDesc d = table[blockIdx.x];
    if (threadIdx.x == 0) { s_progress = 0; s_fail = 0; }
    // (the barrier behind the first level's right-hand sides publishes the two words before any wave looks at them)
    ml_apply_member(d, levels + d.first, xbase + d.xoff, lds, &s_progress, &s_fail);
    if (threadIdx.x == 0) *d.err = s_fail;          // (one writer per member: its own word, whatever the other members do)
}

// bytes of dynamic LDS one workgroup of k_ml_apply_batch may take on the current device
size_t ml_apply_batch_lds_cap() { return kernel_lds_cap<k_ml_apply_batch>(); }

// `count` members, one workgroup each; member i's vector is d_x + table[i].xoff, its levels d_levels + table[i].first; lds_bytes for every
// workgroup (<= the cap): 8 bytes per unknown of the launch's largest member
int ml_apply_batch_launch(hipStream_t st, int32_t count, const MlApplyDesc *d_table, const MlLevelDesc *d_levels, double *d_x, size_t lds_bytes)
{
    if (count <= 0) return ILUPP_OK;
    if (lds_bytes > ml_apply_batch_lds_cap()) return ILUPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_ml_apply_batch, dim3((unsigned)count), dim3(kBatchThreads), lds_bytes, st, d_table, d_levels, d_x);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}


// ---- the whole left-preconditioned BiCGstab solve of MANY small systems in ONE launch: one workgroup per member --------------------
// k_bicgstab_batch runs _bicgstab_block of ilupp_amd/device.py with k = 1, statement for statement, for its member: the SpMV of
// k_spmv_rows (one sum per row in stored order from 0.0), the apply above, the dot products in the shape of ilupp_hip_block_dot_device for
// this n, the updates of k_block_update<1>, IEEE division and the correctly rounded square root -- so every member has the bits of
// bicgstab(A_k, b_k[:, None], M_k), the same solve done alone with those launches.  The member's preconditioner is left open: a
// descriptor with perm != nullptr is an ILUCP / ILUTP member; perm == nullptr a non-pivoting one (ILU0, ILUT, ILUC, IChol0, ICholT: the
// two triangles of apply_plan / sweep_parts, tmp from the scratch's block), which apply_member applies without a permutation;
// ptr1 == nullptr a member without a preconditioner, prec_ of _bicgstab_block being the identity: the apply is skipped (the branch is
// uniform over the workgroup), r = r0*, Ap = A p, As = A s.  The seven vectors y, r, r0*, p, s, Ap, As lie in the member's part of the
// workspace; one CU touches them (its L1 and L2 keep them), and every hand-over between two phases of the workgroup is a
// __syncthreads().
//
// Dynamic LDS: [2][2][kDotMaxNb] doubles of dot scratch (the chunks' partial sums of up to two dots at once, two buffers used in
// turn), then the sweeps' one or two arrays of n.
static constexpr int kDotMaxNb = 128;                          // chunks of a dot: n <= 256 kDotMaxNb
static constexpr int kDotScratch = 2 * 2 * kDotMaxNb;          // doubles
static constexpr int kBicgstabBatchVectors = 7;

// the tree over the lower 64 of 256 values a wave holds as v[l] = (t[l] + t[l + 128]) + (t[l + 64] + t[l + 192]): strides 32 .. 1,
// lane l < s takes v[l] + v[l + s] as sh[w] = sh[w] + sh[w + s] does; lane 0 holds the sum
__device__ __forceinline__ double wave_tree(double v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const double o = __shfl_down(v, s); v = v + o; }
    return v;
}

// ND (1 or 2) dot products a[q] . b[q] of n elements by the whole workgroup, in the shape of k_bdot_part<1> / k_bdot_finish: nb chunks of
// `chunk` <= 256 consecutive rows; partial v of chunk c is 0.0 + a[lo + v] * b[lo + v] (0.0 past the chunk's end); the tree over the 256
// partials -- strides 128 and 64 are the lane's own four values, the rest wave_tree; then the finishing tree over s0[t] = 0.0 +
// partial[t] (0.0 from nb on).  A wave takes the chunks w, w + 4, ...; the partial sums meet in `part` (one barrier), and EVERY wave adds
// them up, so every lane returns the same bits.  part: 2 * kDotMaxNb doubles, not the buffer of the call before.
template <int ND>
__device__ __forceinline__ void wg_dots(const int n, const int nb, const int chunk, const double *a0, const double *b0, const double *a1,
                                        const double *b1, double *part, double *out)
{
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < nb; c += kBatchThreads / 64) {
        const int lo = c * chunk, hi = min(n, lo + chunk);
        double t[ND][4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = lo + l + 64 * m;
#pragma unroll
            for (int q = 0; q < ND; ++q) {
                const double *a = q ? a1 : a0, *b = q ? b1 : b0;
                double acc = 0.0;
                if (i < hi) { const double p = a[i] * b[i]; acc = acc + p; }
                t[q][m] = acc;
            }
        }
#pragma unroll
        for (int q = 0; q < ND; ++q) {
            const double lo2 = t[q][0] + t[q][2], hi2 = t[q][1] + t[q][3];      // stride 128, then stride 64
            const double v = wave_tree(lo2 + hi2);
            if (l == 0) part[q * kDotMaxNb + c] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ND; ++q) {
        double t[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = l + 64 * m;
            double s0 = 0.0;
            if (i < nb) s0 = s0 + part[q * kDotMaxNb + i];
            t[m] = s0;
        }
        const double lo2 = t[0] + t[2], hi2 = t[1] + t[3];
        out[q] = __shfl(wave_tree(lo2 + hi2), 0);
    }
}

// dst = A src: one lane per row, acc = acc + val * x in stored order from 0.0 (k_spmv_rows)
__device__ __forceinline__ void wg_spmv(const int n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                        const double *__restrict__ val, const double *src, double *dst)
{
    for (int r = threadIdx.x; r < n; r += kBatchThreads) {
        const int q0 = ptr[r], q1 = ptr[r + 1];
        double acc = 0.0;
        for (int q = q0; q < q1; q += kBG) {         // kBG entries' loads in flight together, added one after the other in stored order
            int c[kBG];
            double v[kBG], xv[kBG];
#pragma unroll
            for (int w = 0; w < kBG; ++w) if (q + w < q1) { c[w] = idx[q + w]; v[w] = val[q + w]; }
#pragma unroll
            for (int w = 0; w < kBG; ++w) if (q + w < q1) xv[w] = src[c[w]];
#pragma unroll
            for (int w = 0; w < kBG; ++w) if (q + w < q1) { const double p = v[w] * xv[w]; acc = acc + p; }
        }
        dst[r] = acc;
    }
}

__device__ __forceinline__ bool scalar_ok(const double v) { return v != 0.0 && isfinite(v); }      // what a recurrence may divide by

// The way out of a solver kernel: r.r at the exit (unless the loop's last check has just taken it) and the iterate copied to the member's
// slice of the output -- a member whose sweep gave up leaves both as they were -- then the member's own words.  `last`: ||r_0|| of the
// preconditioned residuals (BiCGstab) / ||b|| (CG).
__device__ __forceinline__ void solve_member_exit(const PivotApplyDesc &d, const PivotSolveDesc &e, const int n, const int nb, const int chunk,
                                                  const double *r, const double *xw, double *x, double *part, const bool failed,
                                                  const bool active, const bool converged, const bool zero, const bool have_rr, double rr,
                                                  const long long iters, const double last, long long *iterations, int32_t *flags,
                                                  double *rr_out, double *last_out)
{
    const int tid = threadIdx.x;
    if (!failed) {
        if (!have_rr) { double v[2]; wg_dots<1>(n, nb, chunk, r, r, nullptr, nullptr, part, v); rr = v[0]; }      // (r.r at the exit)
        for (int i = tid; i < n; i += kBatchThreads) x[i] = xw[i];
    }
    if (tid == 0) {                                  // (one writer per member: its own words, whatever the other members do)
        *d.err = failed ? 1 : 0;
        iterations[e.member] = iters;
        flags[e.member] = (active ? 1 : 0) | (converged ? 2 : 0) | (failed ? 4 : 0) | (zero ? 8 : 0);
        rr_out[e.member] = rr;
        last_out[e.member] = last;
    }
}

// A MULTILEVEL member of the solve (k_bicgstab_batch<true> only) travels in the same PivotApplyDesc: plain_first == kMlMember marks it,
// ptr1 points at its level records (MlLevelDesc, the launch's level table), kind1 is their number, kind2 the direction, tmp its n doubles
// of scratch.  Its apply is ml_apply_member in place on dst, behind a plain copy (which changes no bits) where dst is not src.
static constexpr int kMlMember = 2;
__device__ __forceinline__ void apply_member_or_ml(const PivotApplyDesc &d, const double *src, double *dst, unsigned long long *arr,
                                                   const unsigned lds_bytes, unsigned *s_progress, int *s_fail)
{
    if (d.plain_first != kMlMember) { apply_member(d, src, dst, arr, lds_bytes, s_progress, s_fail); return; }      // (uniform over the workgroup)
    if (dst != src) {
        for (int i = threadIdx.x; i < d.n; i += kBatchThreads) dst[i] = src[i];
        __syncthreads();
    }
    MlApplyDesc m;
    m.n = d.n; m.levels = d.kind1; m.first = 0; m.transpose = d.kind2; m.xoff = 0; m.tmp = d.tmp; m.err = nullptr;
    ml_apply_member(m, reinterpret_cast<const MlLevelDesc *>(d.ptr1), dst, arr, s_progress, s_fail);
}

// ML: the launch has a multilevel member (the apply is then a choice on the descriptor); false: the kernel as it always was
template <bool ML>
__global__ void __launch_bounds__(kBatchThreads)
k_bicgstab_batch(const PivotApplyDesc *__restrict__ table, const PivotSolveDesc *__restrict__ systems, const double *bbase,
                 const double *x0base, double *xbase, double *work, const unsigned sweep_bytes, const int maxiter, const double rtol,
                 const int check_every, long long *iterations, int32_t *flags, double *rr_out, double *init_out)
{
    extern __shared__ unsigned long long lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail;
    const PivotApplyDesc d = table[blockIdx.x];
    const PivotSolveDesc e = systems[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    if (tid == 0) { s_progress = 0; s_fail = 0; }
    double *dots = reinterpret_cast<double *>(lds);
    unsigned long long *arr = lds + kDotScratch;
    const int nb = (n + 255) / 256, chunk = (n + nb - 1) / nb;      // (n <= 256 kDotMaxNb)
    unsigned turn = 0;
    auto part = [&]() { return dots + (turn++ & 1u) * (2 * kDotMaxNb); };
    const bool has_m = d.ptr1 != nullptr;
    double *y = work + e.woff, *r = y + n, *r0 = r + n, *p = r0 + n, *s = p + n, *Ap = s + n, *As = Ap + n;
    const double *b = bbase + d.xoff;
    const double *x0 = x0base ? x0base + d.xoff : nullptr;
    double *x = xbase + d.xoff;

    // The loop as a sequence of HALF steps, so that the SpMV, the apply and the pair of dots behind it stand in the code once (the apply
    // is two inlined sweeps: three copies of it would not fit the instruction cache):
    //   half 0 (once):   y = x0 or 0; r0* = b (or b - A y); r = M^-1 r0*; r0* = r; p = r; init = sqrt(r.r); zero = (b.b == 0) | (init == 0)
    //   half 1:          Ap = M^-1 (A p); rho = r.r0*; apr = Ap.r0*; alpha = rho / apr; s = r - alpha Ap
    //   half 2:          As = M^-1 (A s); omega = (As.s) / (As.As); y += alpha p; y += omega s; r = s - omega As;
    //                    beta = ((r.r0*) / rho) * (alpha / omega); p = p - omega Ap; p = beta p + r; the convergence test
    for (int i = tid; i < n; i += kBatchThreads) y[i] = x0 ? x0[i] : 0.0;
    __syncthreads();                                 // (also publishes s_progress and s_fail: a member without M meets no sweep's barrier)
    bool failed = false, zero = false, active = false, converged = false, have_rr = false;
    double init = 0.0, rho = 0.0, alpha = 0.0, rr = 0.0, v2[2];
    long long iters = 0;
    for (int half = 0, it = 0;; half = half == 1 ? 2 : 1) {
        double *vec = half == 0 ? r : half == 1 ? Ap : As;
        if (half != 0 || x0) {
            wg_spmv(n, e.aptr, e.aidx, e.aval, half == 0 ? y : half == 1 ? p : s, half == 0 ? As : vec);
            __syncthreads();
        }
        if (half == 0) {
            if (x0) { for (int i = tid; i < n; i += kBatchThreads) r[i] = b[i] - As[i]; }
            else { for (int i = tid; i < n; i += kBatchThreads) r[i] = b[i]; }
            __syncthreads();
        }
        if (has_m) {
            if constexpr (ML) apply_member_or_ml(d, vec, vec, arr, sweep_bytes, &s_progress, &s_fail);
            else apply_member(d, vec, vec, arr, sweep_bytes, &s_progress, &s_fail);
            if (s_fail != 0) { failed = true; active = false; break; }
        }
        if (half == 0) {
            for (int i = tid; i < n; i += kBatchThreads) { const double v = r[i]; r0[i] = v; p[i] = v; }
            __syncthreads();
        }
        wg_dots<2>(n, nb, chunk, half == 2 ? As : r, half == 0 ? r : half == 1 ? r0 : s, half == 0 ? b : vec, half == 0 ? b : half == 1 ? r0 : As,
                   part(), v2);
        if (half == 0) {
            init = __dsqrt_rn(v2[0]);
            zero = v2[1] == 0.0 || init == 0.0;
            active = !zero;
            converged = zero;
            if (!active || maxiter <= 0) break;
        } else if (half == 1) {
            rho = v2[0];
            if (!(scalar_ok(rho) && scalar_ok(v2[1]))) { active = false; break; }      // breakdown: nothing more is touched, not converged
            alpha = rho / v2[1];
            for (int i = tid; i < n; i += kBatchThreads) { const double aap = alpha * Ap[i]; s[i] = r[i] - aap; }
            __syncthreads();
        } else {
            const double omega = v2[0] / v2[1];
            if (!scalar_ok(omega)) { active = false; break; }
            for (int i = tid; i < n; i += kBatchThreads) {
                const double ap = alpha * p[i];
                double yv = y[i] + ap;
                const double os = omega * s[i];
                yv = yv + os;
                y[i] = yv;
                const double oas = omega * As[i];
                r[i] = s[i] - oas;
            }
            __syncthreads();
            wg_dots<1>(n, nb, chunk, r, r0, nullptr, nullptr, part(), v2);
            const double beta = (v2[0] / rho) * (alpha / omega);
            for (int i = tid; i < n; i += kBatchThreads) {
                const double oap = omega * Ap[i];
                const double pv = p[i] - oap;
                const double bp = beta * pv;
                p[i] = bp + r[i];
            }
            __syncthreads();
            ++iters;
            ++it;
            if (check_every > 0 && it % check_every == 0 && rtol > 0.0) {
                wg_dots<1>(n, nb, chunk, r, r, nullptr, nullptr, part(), v2);
                rr = v2[0];
                have_rr = true;                      // (r stays as it is from here to the exit when the loop ends now)
                const double rel = __dsqrt_rn(rr) / init;
                if (rel <= rtol) { converged = true; active = false; break; }
            }
            if (it >= maxiter) break;
            have_rr = false;
        }
    }
    solve_member_exit(d, e, n, nb, chunk, r, y, x, part(), failed, active, converged, zero, have_rr, rr, iters, init, iterations, flags, rr_out,
                      init_out);
}


// ---- the whole preconditioned CG solve of MANY small symmetric positive definite systems in ONE launch: one workgroup per member ----
// k_cg_batch runs _cg_block of ilupp_amd/device.py with k = 1, statement for statement, for its member, out of the same pieces as the
// kernel above: wg_spmv, apply_member (z = M^-1 r, r left as it is), wg_dots, the updates of k_block_update<0>, IEEE division and the
// correctly rounded square root -- so every member has the bits of cg(A_k, b_k[:, None], M_k).  The descriptors are those of the
// batched apply with perm == nullptr (IChol0, ICholT, ILU0, ILUT, ILUC); ptr1 == nullptr: a member without a preconditioner, z = r.
// The FIVE vectors x, r, z, p, Ap lie in the member's part of the workspace (x too: a member whose sweep gives up leaves its slice of
// the output as it was); a member without a preconditioner leaves its z unused.  Dynamic LDS as above: kDotScratch doubles, then the
// sweeps' one or two arrays of n.
static constexpr int kCgBatchVectors = 5;

__global__ void __launch_bounds__(kBatchThreads)
k_cg_batch(const PivotApplyDesc *__restrict__ table, const PivotSolveDesc *__restrict__ systems, const double *bbase, const double *x0base,
           double *xbase, double *work, const unsigned sweep_bytes, const int maxiter, const double rtol, const int check_every,
           long long *iterations, int32_t *flags, double *rr_out, double *bnorm_out)
{
    extern __shared__ unsigned long long lds[];
    __shared__ unsigned s_progress;
    __shared__ int s_fail;
    const PivotApplyDesc d = table[blockIdx.x];
    const PivotSolveDesc e = systems[blockIdx.x];
    const int n = d.n, tid = threadIdx.x;
    if (tid == 0) { s_progress = 0; s_fail = 0; }
    double *dots = reinterpret_cast<double *>(lds);
    unsigned long long *arr = lds + kDotScratch;
    const int nb = (n + 255) / 256, chunk = (n + nb - 1) / nb;      // (n <= 256 kDotMaxNb)
    unsigned turn = 0;
    auto part = [&]() { return dots + (turn++ & 1u) * (2 * kDotMaxNb); };
    const bool has_m = d.ptr1 != nullptr;
    double *xw = work + e.woff, *r = xw + n, *z = has_m ? r + n : r, *p = r + 2 * n, *Ap = p + n;
    const double *b = bbase + d.xoff;
    const double *x0 = x0base ? x0base + d.xoff : nullptr;
    double *x = xbase + d.xoff;

    // x = x0 or 0; r = b, or b - A x
    for (int i = tid; i < n; i += kBatchThreads) xw[i] = x0 ? x0[i] : 0.0;
    __syncthreads();                                 // (also publishes s_progress and s_fail)
    if (x0) {
        wg_spmv(n, e.aptr, e.aidx, e.aval, xw, Ap);
        __syncthreads();
        for (int i = tid; i < n; i += kBatchThreads) r[i] = b[i] - Ap[i];
    } else {
        for (int i = tid; i < n; i += kBatchThreads) r[i] = b[i];
    }
    __syncthreads();
    bool failed = false, zero = false, active = false, converged = false, have_rr = false, first = true;
    double bnorm = 0.0, rz = 0.0, rr = 0.0, v2[2];
    long long iters = 0;
    for (int it = 0;;) {
        // loop top: the one place where the apply stands
        if (has_m) {
            apply_member(d, r, z, arr, sweep_bytes, &s_progress, &s_fail);
            if (s_fail != 0) { failed = true; active = false; break; }
        }
        double rz_new;
        if (first) {
            first = false;
            wg_dots<2>(n, nb, chunk, r, z, b, b, part(), v2);
            rz_new = v2[0];
            bnorm = __dsqrt_rn(v2[1]);
            wg_dots<1>(n, nb, chunk, r, r, nullptr, nullptr, part(), v2);
            rr = v2[0];
            have_rr = true;
            zero = bnorm == 0.0 || rr == 0.0;
            active = !zero;
            converged = zero;
            if (!active || maxiter <= 0) break;
            for (int i = tid; i < n; i += kBatchThreads) p[i] = z[i];
        } else {
            wg_dots<1>(n, nb, chunk, r, z, nullptr, nullptr, part(), v2);
            rz_new = v2[0];
            const double beta = rz_new / rz;
            for (int i = tid; i < n; i += kBatchThreads) { const double pb = p[i] * beta; p[i] = z[i] + pb; }
        }
        __syncthreads();
        rz = rz_new;
        // loop body
        wg_spmv(n, e.aptr, e.aidx, e.aval, p, Ap);
        __syncthreads();
        wg_dots<1>(n, nb, chunk, p, Ap, nullptr, nullptr, part(), v2);
        const double pap = v2[0];
        const double alpha = rz / pap;
        if (!scalar_ok(pap)) { active = false; break; }      // breakdown: nothing more is touched, not converged
        for (int i = tid; i < n; i += kBatchThreads) {
            const double pa = p[i] * alpha;
            xw[i] = xw[i] + pa;
            const double apa = Ap[i] * alpha;
            r[i] = r[i] - apa;
        }
        __syncthreads();
        have_rr = false;
        ++iters;
        ++it;
        if (check_every > 0 && it % check_every == 0 && rtol > 0.0) {
            wg_dots<1>(n, nb, chunk, r, r, nullptr, nullptr, part(), v2);
            rr = v2[0];
            have_rr = true;
            const double rel = __dsqrt_rn(rr) / bnorm;
            if (rel <= rtol) { converged = true; active = false; break; }
        }
        if (it >= maxiter) break;
    }
    solve_member_exit(d, e, n, nb, chunk, r, xw, x, part(), failed, active, converged, zero, have_rr, rr, iters, bnorm, iterations, flags, rr_out,
                      bnorm_out);
}

// ---- the host side of the two solver kernels ---------------------------------------------------------------------------------------
// (ml: the instantiation of the BiCGstab kernel that takes multilevel members -- a kernel of its own with a cap of its own)
static size_t solve_batch_lds_cap(BatchSolver s, bool ml)
{
    if (s == BATCH_CG) return kernel_lds_cap<k_cg_batch>();
    return ml ? kernel_lds_cap<k_bicgstab_batch<true>>() : kernel_lds_cap<k_bicgstab_batch<false>>();
}

// the largest n of a member of the solve's launch: the dot scratch and 8 n bytes for the sweeps fit, and the dot has at most kDotMaxNb chunks
int64_t solve_batch_max_n(BatchSolver s, bool ml)
{
    const size_t cap = solve_batch_lds_cap(s, ml), scratch = sizeof(double) * (size_t)kDotScratch;
    const int64_t by_lds = cap > scratch ? (int64_t)((cap - scratch) / 8) : 0;
    return by_lds < 256 * kDotMaxNb ? by_lds : 256 * kDotMaxNb;
}

int solve_batch_work_factor(BatchSolver s) { return s == BATCH_CG ? kCgBatchVectors : kBicgstabBatchVectors; }

// `count` members, one workgroup each; sweep_bytes of LDS for the sweeps of every workgroup (the dot scratch comes on top)
int solve_batch_launch(BatchSolver s, hipStream_t st, int32_t count, const PivotApplyDesc *d_table, const PivotSolveDesc *d_systems,
                       const double *d_b, const double *d_x0, double *d_x, double *d_work, size_t sweep_bytes, int32_t maxiter, double rtol,
                       int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_last, bool ml)
{
    if (count <= 0) return ILUPP_OK;
    if (ml && s == BATCH_CG) return ILUPP_ERR_UNSUPPORTED;      // (the multilevel preconditioner is not symmetric: no such instantiation)
    const size_t lds_bytes = sizeof(double) * (size_t)kDotScratch + sweep_bytes;
    if (lds_bytes > solve_batch_lds_cap(s, ml)) return ILUPP_ERR_UNSUPPORTED;
    const auto kernel = s == BATCH_CG ? k_cg_batch : ml ? k_bicgstab_batch<true> : k_bicgstab_batch<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3(kBatchThreads), lds_bytes, st, d_table, d_systems, d_b, d_x0, d_x, d_work,
                       (unsigned)sweep_bytes, (int)maxiter, rtol, (int)check_every, reinterpret_cast<long long *>(d_iterations), d_flags, d_rr,
                       d_last);
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
