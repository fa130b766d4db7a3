// ilupp_amd/csrc/sptrsm_lvl.hip -- k right-hand sides per sweep over the level-ordered records of sptrsv_lvl.hip (gfx950 only).
//
// The block apply (ilupp_hip_apply_block*): X is row-major n x k (row r's k values contiguous), and one launch solves a chunk of KB
// of its columns.  The records are the single sweep's (LevelSweep: rows in level order, [off-diagonal entries in the reference's
// order ..., diagonal], columns as positions), so the factor's indices and values are read once per chunk instead of once per column,
// and every round trip of the dependency chain carries KB columns' arithmetic.
//
// Layout: KB consecutive lanes per row, lane u of a row owns column u.  Each lane is k_sptrsv_lvl's lane for its column: the same
// window of W entries, the same accumulation in stored order (acc = acc - v * x, -ffp-contract=off), the same division by the
// diagonal, the canonical NaN for an empty row and for any NaN result.  Columns never meet.  The unknowns are handed over through a
// private n x KB buffer in position order (xp, all-sentinel before the launch): the data is the flag, per value, as in the single
// kernel -- the KB lanes of a row load their KB values of a dependency as one coalesced access (KB = 8: one 64-byte line), and each
// lane waits only for its own value.  A workgroup takes a ticket and owns BLOCK / KB consecutive positions; a row reads rows of
// earlier tickets (memory) or of its own workgroup (LDS), never of a later one.  Every wait is bounded and gives up into `err`.
#include "common.h"

namespace ilupp {

static constexpr unsigned kLmSpinLimit = 1u << 22;      // (k_sptrsv_lvl's bound)

template <int W, int BLOCK, int KB>                     // W: dependencies fetched per round trip; KB: columns per launch
__global__ void __launch_bounds__(BLOCK)
k_sptrsm_lvl(int32_t n, const int32_t *__restrict__ ptrp, const int32_t *__restrict__ idxp, const double *__restrict__ valp,
             const int32_t *__restrict__ perm, const double *__restrict__ rhs, int64_t ldr, double *xp, double *__restrict__ out,
             int64_t ldo, int32_t *ticket, int32_t *err)
{
    static_assert(KB >= 1 && KB <= 64 && (KB & (KB - 1)) == 0 && BLOCK % KB == 0, "KB: a power of two that divides the block");
    constexpr int R = BLOCK / KB;                                 // rows of a workgroup
    __shared__ unsigned wg_ticket;
    __shared__ unsigned long long xs[BLOCK];                      // this workgroup's unknowns (row-major R x KB), sentinel = not yet
    if (threadIdx.x == 0) wg_ticket = (unsigned)atomicAdd(ticket, 1);
    xs[threadIdx.x] = kSentinel;
    __syncthreads();
    const int lr = (int)threadIdx.x / KB, u = (int)threadIdx.x % KB;
    const int64_t tb = (int64_t)wg_ticket * R;
    const int64_t t = tb + lr;
    bool active = t < n;
    int j = 0, jend = 0, rn = 0;
    double acc = 0.0, dv = 1.0;
    if (active) {
        const int lo = ptrp[t], hi = ptrp[t + 1];
        rn = perm[t];
        acc = rhs[(int64_t)rn * ldr + u];
        j = lo; jend = hi - 1;
        if (hi > lo) dv = valp[hi - 1];
        else { j = jend = lo; dv = __longlong_as_double((long long)kCanonNaN); }
    }
    const unsigned long long *xpb = reinterpret_cast<const unsigned long long *>(xp);
    volatile unsigned long long *xsv = xs;
    int wc[W];
    double wv[W];
    unsigned long long wb[W];
    int wn = 0, cur = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) { wc[w] = -1; wv[w] = 0.0; wb[w] = kSentinel; }
    unsigned spins = 0;
    for (;;) {
        if (__ballot(active) == 0ull) break;
        bool progressed = false;
        if (active && cur == wn && j != jend) {
            const int left = jend - j;
            wn = left < W ? left : W;
            cur = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) if (w < wn) { wc[w] = idxp[j + w]; wv[w] = valp[j + w]; }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const long lb = (long)wc[w] - (long)tb;
                wb[w] = (w < wn && lb < 0) ? ld_agent_u64(xpb + (int64_t)wc[w] * KB + u) : kSentinel;
            }
            progressed = true;
        } else if (active) {
            // every value of the window that had not arrived is asked for again, all of them in one round trip
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w >= cur && w < wn && wb[w] == kSentinel && (long)wc[w] < (long)tb) wb[w] = ld_agent_u64(xpb + (int64_t)wc[w] * KB + u);
        }
        if (active) {
            // everything of the window that is there, in stored order
            bool stop = false;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (!stop && w >= cur && w < wn) {
                    const long lb = (long)wc[w] - (long)tb;
                    unsigned long long b = wb[w];
                    if (lb >= 0) b = xsv[lb * KB + u];
                    if (b != kSentinel) {
                        const double prod = wv[w] * __longlong_as_double((long long)b);
                        acc = acc - prod;                           // x[k] -= data[j]*x[indices[j]]  (sparse.hpp:4049, :4070)
                        ++j;
                        ++cur;
                        progressed = true;
                    } else {
                        stop = true;
                    }
                }
            }
            if (j == jend) {
                double x = acc / dv;                                // x[k] /= diagonal  (:4051, :4072)
                if (x != x) x = __longlong_as_double((long long)kCanonNaN);   // never store the sentinel
                st_agent_f64(xp + t * KB + u, x);
                xsv[threadIdx.x] = (unsigned long long)__double_as_longlong(x);
                out[(int64_t)rn * ldo + u] = x;
                active = false;
                progressed = true;
            }
        }
        if (__any(progressed)) {
            spins = 0;
        } else {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kLmSpinLimit) {
                if ((threadIdx.x & 63) == 0) atomicExch(err, 1);
                break;
            }
        }
    }
}

// KB columns of a row-major block: rhs (leading dimension ldr) -> out (ldo); xp: n * kb doubles, refilled with sentinels here
int sptrsm_lvl(hipStream_t st, const LevelSweep &ls, int kb, const double *rhs, int64_t ldr, double *out, int64_t ldo, double *xp,
               int32_t *d_ticket, int32_t *d_err)
{
    fill_u64(st, reinterpret_cast<unsigned long long *>(xp), (int64_t)ls.n * kb, kSentinel);
#define LM_LAUNCH(W, B, K)                                                                                                   \
    hipLaunchKernelGGL((k_sptrsm_lvl<W, B, K>), dim3((unsigned)(((int64_t)ls.n + (B) / (K) - 1) / ((B) / (K)))), dim3(B), 0, st,  \
                       ls.n, ls.ptr, ls.idx, ls.val, ls.perm, rhs, ldr, xp, out, ldo, d_ticket, d_err)
#define LM_LAUNCH_W(B, K) do { if (ls.w == 4) LM_LAUNCH(4, B, K); else if (ls.w == 8) LM_LAUNCH(8, B, K); else LM_LAUNCH(16, B, K); } while (0)
#define LM_LAUNCH_K(B)                                                                                                       \
    do {                                                                                                                     \
        switch (kb) {                                                                                                        \
        case 1: LM_LAUNCH_W(B, 1); break;                                                                                    \
        case 2: LM_LAUNCH_W(B, 2); break;                                                                                    \
        case 4: LM_LAUNCH_W(B, 4); break;                                                                                    \
        case 8: LM_LAUNCH_W(B, 8); break;                                                                                    \
        default: LM_LAUNCH_W(B, 16); break;                                                                                  \
        }                                                                                                                    \
    } while (0)
    if (kb != 1 && kb != 2 && kb != 4 && kb != 8 && kb != kSptrsmMaxKB) {
        set_error("internal error: block sweep chunk width not instantiated");
        return ILUPP_ERR_INTERNAL;
    }
    if (ls.block == 256) LM_LAUNCH_K(256);
    else LM_LAUNCH_K(1024);
#undef LM_LAUNCH_K
#undef LM_LAUNCH_W
#undef LM_LAUNCH
    ILUPP_HIP(hipGetLastError());
    return ILUPP_OK;
}

}  // namespace ilupp
