// ilupp_amd/csrc/block_krylov.hip -- the vector work of the k-column CG / BiCGstab of ilupp_amd/device.py: k column dot products with a
// reduction shape fixed by n alone, and the masked per-column updates.  Blocks are row-major n x k (row i's k values contiguous).
//
// Dot shape (per column, whatever k is): nb = min(1024, ceil(n / 256)) workgroups, each a contiguous chunk of ceil(n / nb) rows; inside
// a workgroup 256 partial sums, partial v adding rows lo + v, lo + v + 256, ... in order (acc = acc + a * b, -ffp-contract=off), then a
// fixed tree over the 256; then one finishing workgroup per column adds the nb partials the same way.  A launch takes CH columns (the
// block apply's chunk widths 1 .. 16): CH consecutive lanes of a row read CH consecutive values, and each lane carries CH of the 256
// partial sums of its column -- the sums and their order are the same for every CH.  So column j of a k-column dot has the bits of the
// same column dotted alone, and the same bits on every run.
//
// Updates: every element's arithmetic is one statement of the 1-D recurrence in device.py and never depends on k; a column whose
// active flag is zero is neither read nor written (frozen columns keep their bits even when their direction holds NaN or Inf).
#include "common.h"

#include <map>
#include <mutex>

namespace ilupp {

namespace {

constexpr int kBdThreads = 256;
constexpr int kBdMaxBlocks = 1024;

template <int CH>
__global__ __launch_bounds__(kBdThreads) void k_bdot_part(int32_t n, int32_t chunk, const double *__restrict__ A, int64_t lda,
                                                          const double *__restrict__ B, int64_t ldb, int64_t c0, double *__restrict__ partial)
{
    constexpr int S = kBdThreads / CH;                           // rows of one sweep of the workgroup's lanes
    __shared__ double sh[kBdThreads * CH];                       // [partial v][column u]
    const int u = threadIdx.x % CH, v0 = threadIdx.x / CH;
    const int64_t col = c0 + (int64_t)blockIdx.y * CH + u;
    const int32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    double acc[CH];
#pragma unroll
    for (int m = 0; m < CH; ++m) acc[m] = 0.0;
    for (int32_t base = lo; base < hi; base += kBdThreads) {
#pragma unroll
        for (int m = 0; m < CH; ++m) {                           // partial v = v0 + m S
            const int32_t i = base + v0 + m * S;
            if (i < hi) { const double p = A[(int64_t)i * lda + col] * B[(int64_t)i * ldb + col]; acc[m] = acc[m] + p; }
        }
    }
#pragma unroll
    for (int m = 0; m < CH; ++m) sh[(v0 + m * S) * CH + u] = acc[m];
    __syncthreads();
#pragma unroll
    for (int s = kBdThreads / 2; s > 0; s >>= 1) {
        for (int w = threadIdx.x; w < s * CH; w += kBdThreads) sh[w] = sh[w] + sh[w + s * CH];
        __syncthreads();
    }
    if (threadIdx.x < CH) partial[(c0 + (int64_t)blockIdx.y * CH + threadIdx.x) * gridDim.x + blockIdx.x] = sh[threadIdx.x];
}

// one workgroup per column: its nb partial sums in order, the same tree
__global__ __launch_bounds__(kBdThreads) void k_bdot_finish(int32_t nb, const double *__restrict__ partial, double *__restrict__ out)
{
    __shared__ double sh[kBdThreads];
    const int t = threadIdx.x;
    const double *pc = partial + (int64_t)blockIdx.x * nb;
    double s0 = 0.0;
    for (int32_t i = t; i < nb; i += kBdThreads) s0 = s0 + pc[i];
    sh[t] = s0;
    __syncthreads();
#pragma unroll
    for (int s = kBdThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = sh[0];
}

static void bdot_launch(hipStream_t st, int ch, int64_t chunks, int nb, int32_t n, int32_t chunk, const double *A, int64_t lda, const double *B,
                        int64_t ldb, int64_t c0, double *partial)
{
#define BD_LAUNCH(C) hipLaunchKernelGGL((k_bdot_part<C>), dim3((unsigned)nb, (unsigned)chunks), dim3(kBdThreads), 0, st, n, chunk, A, lda, B, ldb, c0, partial)
    switch (ch) {
    case 1: BD_LAUNCH(1); break;
    case 2: BD_LAUNCH(2); break;
    case 4: BD_LAUNCH(4); break;
    case 8: BD_LAUNCH(8); break;
    default: BD_LAUNCH(16); break;
    }
#undef BD_LAUNCH
}

// the partial sums' buffer of a (device, stream): calls on one stream are ordered, so one buffer per stream is enough; it only grows
// (after the stream has finished with the old one) and lives as long as the process
struct BdWork { double *p = nullptr; size_t doubles = 0; };
std::mutex g_bd_mu;
std::map<std::pair<int, hipStream_t>, BdWork> g_bd_work;

double *bd_partials(hipStream_t st, size_t doubles)
{
    int dev = 0;
    ILUPP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_bd_mu);
    BdWork &w = g_bd_work[std::make_pair(dev, st)];
    if (w.doubles < doubles) {
        if (w.p) { ILUPP_HIP(hipStreamSynchronize(st)); ILUPP_HIP(hipFree(w.p)); w.p = nullptr; w.doubles = 0; }
        ILUPP_HIP(hipMalloc(reinterpret_cast<void **>(&w.p), sizeof(double) * doubles));
        w.doubles = doubles;
    }
    return w.p;
}

// CG, stage 0: x = x + p alpha; r = r - Ap alpha.  Stage 1: p = z + p beta.  (cg() in device.py)
// BiCGstab, stage 0: s = r - alpha Ap.  Stage 1: y = y + alpha p; y = y + omega s; r = s - omega As.  Stage 2: p = p - omega Ap;
// p = beta p + r.  (bicgstab() in device.py)
// A workgroup owns `rows` consecutive rows (rows * k elements, element e of the block at e); column of element e: e mod k, stepped.
template <int SOLVER>
__global__ __launch_bounds__(256) void k_block_update(int stage, int32_t n, int64_t k, int64_t rows, const uint8_t *__restrict__ active,
                                                      const double *__restrict__ c0, const double *__restrict__ c1, const double *__restrict__ c2,
                                                      double *__restrict__ V0, double *__restrict__ V1, double *__restrict__ V2,
                                                      double *__restrict__ V3, const double *__restrict__ W0, const double *__restrict__ W1)
{
    const int64_t r0 = (int64_t)blockIdx.x * rows;
    const int64_t r1 = r0 + rows < n ? r0 + rows : n;
    const int64_t e0 = r0 * k, e1 = r1 * k;
    const int64_t step = 256 % k;
    int64_t j = threadIdx.x % k;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        if (active[j]) {
            if (SOLVER == 0) {                                   // V0 = x, V1 = r, V2 = p, W0 = Ap or z; c0 = alpha or beta
                if (stage == 0) {
                    const double a = c0[j];
                    const double pa = V2[e] * a;
                    V0[e] = V0[e] + pa;
                    const double apa = W0[e] * a;
                    V1[e] = V1[e] - apa;
                } else {
                    const double pb = V2[e] * c0[j];
                    V2[e] = W0[e] + pb;
                }
            } else {                                             // V0 = y, V1 = r, V2 = p, V3 = s, W0 = Ap, W1 = As; c0, c1, c2 = alpha, omega, beta
                if (stage == 0) {
                    const double aap = c0[j] * W0[e];
                    V3[e] = V1[e] - aap;
                } else if (stage == 1) {
                    const double ap = c0[j] * V2[e];
                    double y = V0[e] + ap;
                    const double os = c1[j] * V3[e];
                    y = y + os;
                    V0[e] = y;
                    const double oas = c1[j] * W1[e];
                    V1[e] = V3[e] - oas;
                } else {
                    const double oap = c1[j] * W0[e];
                    const double p = V2[e] - oap;
                    const double bp = c2[j] * p;
                    V2[e] = bp + V1[e];
                }
            }
        }
        j += step;
        if (j >= k) j -= k;
    }
}

int block_update(int solver, int stage, int32_t n, int64_t k, const uint8_t *active, const double *c0, const double *c1, const double *c2,
                 double *V0, double *V1, double *V2, double *V3, const double *W0, const double *W1, hipStream_t st)
{
    const int64_t rows = k >= 4096 ? 1 : (4096 + k - 1) / k;    // about 4096 elements per workgroup
    const int64_t blocks = ((int64_t)n + rows - 1) / rows;
    if (blocks > 0x7fffffff) { set_error("block update: block too large"); return ILUPP_ERR_INVALID; }
    if (solver == 0)
        hipLaunchKernelGGL(k_block_update<0>, dim3((unsigned)blocks), dim3(256), 0, st, stage, n, k, rows, active, c0, c1, c2, V0, V1, V2, V3, W0, W1);
    else
        hipLaunchKernelGGL(k_block_update<1>, dim3((unsigned)blocks), dim3(256), 0, st, stage, n, k, rows, active, c0, c1, c2, V0, V1, V2, V3, W0, W1);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return ILUPP_ERR_HIP; }
    return ILUPP_OK;
}

}  // namespace

}  // namespace ilupp

extern "C" int ilupp_hip_block_dot_device(int32_t n, int64_t k, const double *d_A, int64_t lda, const double *d_B, int64_t ldb, double *d_out,
                                          void *hip_stream)
{
    if (!d_A || !d_B || !d_out) { ilupp::set_error("block dot: null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0) { ilupp::set_error("block dot: n must be positive"); return ILUPP_ERR_INVALID; }
    if (k < 0) { ilupp::set_error("block dot: k must not be negative"); return ILUPP_ERR_INVALID; }
    if (lda < k || ldb < k) { ilupp::set_error("block dot: leading dimension smaller than k"); return ILUPP_ERR_INVALID; }
    if (k == 0) return ILUPP_OK;
    if (k > 0x7fffffff) { ilupp::set_error("block dot: k too large"); return ILUPP_ERR_INVALID; }
    try {
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        const int nb = std::max(1, std::min(ilupp::kBdMaxBlocks, (n + ilupp::kBdThreads - 1) / ilupp::kBdThreads));
        const int32_t chunk = (int32_t)(((int64_t)n + nb - 1) / nb);
        double *part = ilupp::bd_partials(st, (size_t)k * (size_t)nb);
        int64_t c0 = 0;
        for (int64_t full = k / 16; full > 0;) {
            const int64_t g = full < 65535 ? full : 65535;
            ilupp::bdot_launch(st, 16, g, nb, n, chunk, d_A, lda, d_B, ldb, c0, part);
            c0 += g * 16;
            full -= g;
        }
        for (int ch = 8; ch >= 1; ch >>= 1)
            if (k - c0 >= ch) { ilupp::bdot_launch(st, ch, 1, nb, n, chunk, d_A, lda, d_B, ldb, c0, part); c0 += ch; }
        hipLaunchKernelGGL(ilupp::k_bdot_finish, dim3((unsigned)k), dim3(ilupp::kBdThreads), 0, st, nb, (const double *)part, d_out);
        ILUPP_HIP(hipGetLastError());
    } catch (const ilupp::HipError &e) {
        ilupp::set_error(std::string("block dot: ") + hipGetErrorString(e.code));
        return ILUPP_ERR_HIP;
    }
    return ILUPP_OK;
}

extern "C" int ilupp_hip_cg_block_update_device(int32_t stage, int32_t n, int64_t k, const uint8_t *d_active, const double *d_coef, double *d_X,
                                                double *d_R, double *d_P, const double *d_V, void *hip_stream)
{
    if (stage != 0 && stage != 1) { ilupp::set_error("cg block update: stage must be 0 or 1"); return ILUPP_ERR_INVALID; }
    if (!d_active || !d_coef || !d_P || !d_V || (stage == 0 && (!d_X || !d_R))) { ilupp::set_error("cg block update: null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0 || k < 0) { ilupp::set_error("cg block update: n must be positive and k non-negative"); return ILUPP_ERR_INVALID; }
    if (k == 0) return ILUPP_OK;
    return ilupp::block_update(0, stage, n, k, d_active, d_coef, nullptr, nullptr, d_X, d_R, d_P, nullptr, d_V, nullptr,
                               static_cast<hipStream_t>(hip_stream));
}

extern "C" int ilupp_hip_bicgstab_block_update_device(int32_t stage, int32_t n, int64_t k, const uint8_t *d_active, const double *d_alpha,
                                                      const double *d_omega, const double *d_beta, double *d_Y, double *d_R, double *d_P,
                                                      double *d_S, const double *d_AP, const double *d_AS, void *hip_stream)
{
    if (stage < 0 || stage > 2) { ilupp::set_error("bicgstab block update: stage must be 0, 1 or 2"); return ILUPP_ERR_INVALID; }
    const bool ok = d_active && (stage == 0 ? (d_alpha && d_R && d_S && d_AP)
                                 : stage == 1 ? (d_alpha && d_omega && d_Y && d_R && d_P && d_S && d_AS)
                                              : (d_omega && d_beta && d_R && d_P && d_AP));
    if (!ok) { ilupp::set_error("bicgstab block update: null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0 || k < 0) { ilupp::set_error("bicgstab block update: n must be positive and k non-negative"); return ILUPP_ERR_INVALID; }
    if (k == 0) return ILUPP_OK;
    return ilupp::block_update(1, stage, n, k, d_active, d_alpha, d_omega, d_beta, d_Y, d_R, d_P, d_S, d_AP, d_AS,
                               static_cast<hipStream_t>(hip_stream));
}
