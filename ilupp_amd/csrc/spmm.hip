// ilupp_amd/csrc/spmm.hip -- Y = A X for a CSR matrix resident in HBM and a row-major block X of k columns: the operator of the
// k-column Krylov loops (ilupp_amd/device.py), one pass over A per chunk of columns instead of one per column.
//
// Layout (as k_sptrsm_lvl): KB consecutive lanes per row, lane u of a row owns column c0 + u.  The KB lanes of a row load the row's
// index and value together (one address per row and instruction), so the gather of X[c, c0 : c0 + KB] is one coalesced 8 KB-byte
// access.  Every lane is k_spmv_rows' lane for its column: acc = 0, then acc = acc + val[q] * x[idx[q]] in stored order, the multiply
// and the add separate statements (the library is built with -ffp-contract=off) -- column j of Y is, bit for bit, what
// ilupp_hip_spmv_device gives for column j.  W entries of a row are loaded at a time (indices and values first, then the W gathers,
// all in flight together) and added one after the other in stored order: W = 16 for long rows (more than 8 entries on average: 27-point
// stencils, random matrices with fill), so that their loads do not queue up behind each other on one lane, W = 8 otherwise; a row of at
// most 8 entries takes its indices and values in six 16-byte loads (as k_spmv_rows).  Where X and Y allow 16-byte accesses (aligned
// bases, even leading dimensions), a lane owns two adjacent columns (CPL = 2: KB / 2 lanes per row, one 16-byte gather per entry): half
// the lanes, half the load instructions per row -- the kernel is bound by how many of those a CU issues, not by bytes.  The two
// columns' sums stay separate and in order.  Columns never meet.  X and Y must not overlap.
#include "common.h"

namespace ilupp {

struct __attribute__((aligned(8))) D2s { double v[2]; };
struct __attribute__((aligned(16))) D2v { double v[2]; };

// CPL columns per lane (1, or 2 with 16-byte loads and stores of X and Y): KB / CPL lanes per row
template <int CPL>
__device__ __forceinline__ void spmm_term(double (&acc)[CPL], double v, const double *__restrict__ xp)
{
    if (CPL == 2) {
        const D2v t = *reinterpret_cast<const D2v *>(xp);
        const double p0 = v * t.v[0];
        acc[0] = acc[0] + p0;
        const double p1 = v * t.v[1];
        acc[1] = acc[1] + p1;
    } else {
        const double p = v * xp[0];
        acc[0] = acc[0] + p;
    }
}

template <int KB, int W, int CPL>
__global__ void __launch_bounds__(256)
k_spmm_rows(int32_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, const double *__restrict__ val, int64_t nnz,
            const double *__restrict__ X, int64_t ldx, double *__restrict__ Y, int64_t ldy, int64_t c0)
{
    static_assert(KB >= 1 && KB <= 16 && (KB & (KB - 1)) == 0 && (CPL == 1 || CPL == 2) && KB % CPL == 0, "KB: a power of two up to 16");
    constexpr int L = KB / CPL;                                  // lanes of a row
    constexpr int R = 256 / L;                                   // rows of a workgroup
    const int64_t r = (int64_t)blockIdx.x * R + threadIdx.x / L;
    if (r >= n) return;
    const int64_t col = c0 + (int64_t)blockIdx.y * KB + (threadIdx.x % L) * CPL;
    const int q0 = ptr[r], q1 = ptr[r + 1];
    const double *__restrict__ xc = X + col;
    double acc[CPL];
#pragma unroll
    for (int m = 0; m < CPL; ++m) acc[m] = 0.0;
    if (W == 8 && q1 - q0 <= 8 && (int64_t)q0 + 8 <= nnz) {
        // a short row in one go (as k_spmv_rows): its indices with two 16-byte loads, its values with four
        const Row8 c = load_row8(idx, q0, q1 - q0, nnz);
        double v[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const D2s t = *reinterpret_cast<const D2s *>(val + q0 + 2 * i); v[2 * i] = t.v[0]; v[2 * i + 1] = t.v[1]; }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < q1 - q0) spmm_term<CPL>(acc, v[i], xc + (int64_t)c.c[i] * ldx);
    } else {
        for (int q = q0; q < q1; q += W) {
            int c[W];
            double v[W];
#pragma unroll
            for (int w = 0; w < W; ++w) if (q + w < q1) { c[w] = idx[q + w]; v[w] = val[q + w]; }
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (q + w < q1) spmm_term<CPL>(acc, v[w], xc + (int64_t)c[w] * ldx);
        }
    }
    if (CPL == 2) {
        D2v t;
        t.v[0] = acc[0];
        t.v[1] = acc[CPL - 1];
        *reinterpret_cast<D2v *>(Y + r * ldy + col) = t;
    } else {
        Y[r * ldy + col] = acc[0];
    }
}

// the columns [c0, c0 + chunks * kb) in one launch, chunks of kb columns
static void spmm_launch(hipStream_t st, int kb, bool long_rows, bool pairs, int64_t chunks, int32_t n, const int32_t *ptr, const int32_t *idx,
                        const double *val, int64_t nnz, const double *X, int64_t ldx, double *Y, int64_t ldy, int64_t c0)
{
#define SPMM_LAUNCH(K, W, C)                                                                                                 \
    hipLaunchKernelGGL((k_spmm_rows<K, W, C>), dim3((unsigned)(((int64_t)n + 256 / ((K) / (C)) - 1) / (256 / ((K) / (C)))), (unsigned)chunks), \
                       dim3(256), 0, st, n, ptr, idx, val, nnz, X, ldx, Y, ldy, c0)
#define SPMM_LAUNCH_W(K, C) do { if (long_rows) SPMM_LAUNCH(K, 16, C); else SPMM_LAUNCH(K, 8, C); } while (0)
#define SPMM_LAUNCH_C(K) do { if (pairs) SPMM_LAUNCH_W(K, 2); else SPMM_LAUNCH_W(K, 1); } while (0)
    switch (kb) {
    case 1: SPMM_LAUNCH_W(1, 1); break;
    case 2: SPMM_LAUNCH_C(2); break;
    case 4: SPMM_LAUNCH_C(4); break;
    case 8: SPMM_LAUNCH_C(8); break;
    default: SPMM_LAUNCH_C(16); break;
    }
#undef SPMM_LAUNCH_C
#undef SPMM_LAUNCH_W
#undef SPMM_LAUNCH
}

}  // namespace ilupp

extern "C" int ilupp_hip_spmm_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int64_t nnz,
                                     const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int64_t k, void *hip_stream)
{
    if (!d_data || !d_indices || !d_indptr || !d_X || !d_Y) { ilupp::set_error("spmm: null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0 || nnz < 0) { ilupp::set_error("spmm: n must be positive and nnz non-negative"); return ILUPP_ERR_INVALID; }
    if (k < 0) { ilupp::set_error("spmm: k must not be negative"); return ILUPP_ERR_INVALID; }
    if (ldx < k || ldy < k) { ilupp::set_error("spmm: leading dimension smaller than k"); return ILUPP_ERR_INVALID; }
    if (k == 0) return ILUPP_OK;
    {   // X and Y must not overlap (every lane reads X while others write Y)
        const char *x0 = reinterpret_cast<const char *>(d_X), *x1 = reinterpret_cast<const char *>(d_X + (int64_t)(n - 1) * ldx + k);
        const char *y0 = reinterpret_cast<const char *>(d_Y), *y1 = reinterpret_cast<const char *>(d_Y + (int64_t)(n - 1) * ldy + k);
        if (x0 < y1 && y0 < x1) { ilupp::set_error("spmm: X and Y overlap"); return ILUPP_ERR_INVALID; }
    }
    if (k == 1 && ldx == 1 && ldy == 1) return ilupp_hip_spmv_device(d_data, d_indices, d_indptr, n, nnz, d_X, d_Y, hip_stream);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const bool long_rows = nnz > 8 * (int64_t)n;                  // (ilupp_hip_spmv_device's switch to k_spmv_rows8)
    // two columns per lane where every pair of X and Y is 16-byte aligned (chunk starts are even: 16s first, then 8, 4, 2) -- for long
    // rows only in chunks of 8 and 16 (with fewer lanes per row a long row's loads queue up on too few lanes: 27-point k = 2, 4 slower)
    const bool pairs = (reinterpret_cast<uintptr_t>(d_X) % 16) == 0 && (reinterpret_cast<uintptr_t>(d_Y) % 16) == 0 && ldx % 2 == 0 && ldy % 2 == 0;
    // chunks of 16 columns in one launch, the rest in chunks of 8, 4, 2, 1 (the block apply's chunk widths)
    int64_t c0 = 0;
    for (int64_t full = k / 16; full > 0;) {                       // (gridDim.y <= 65535)
        const int64_t g = full < 65535 ? full : 65535;
        ilupp::spmm_launch(st, 16, long_rows, pairs, g, n, d_indptr, d_indices, d_data, nnz, d_X, ldx, d_Y, ldy, c0);
        c0 += g * 16;
        full -= g;
    }
    for (int kb = 8; kb >= 1; kb >>= 1)
        if (k - c0 >= kb) { ilupp::spmm_launch(st, kb, long_rows, pairs && kb > 1 && (!long_rows || kb >= 8), 1, n, d_indptr, d_indices, d_data, nnz, d_X, ldx, d_Y, ldy, c0); c0 += kb; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ilupp::set_error(hipGetErrorString(e)); return ILUPP_ERR_HIP; }
    return ILUPP_OK;
}
