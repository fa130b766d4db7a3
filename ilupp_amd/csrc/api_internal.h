// ilupp_amd/csrc/api_internal.h -- what the translation units of the C ABI's host layer share (api.hip and api_*.hip; host code, included
// by nothing else).  What goes in here: a type, macro or template that more than one of those files uses, and the declaration of every
// plain function that one of them defines and another calls.  Whatever one file alone uses stays in that file, static or in an
// anonymous namespace.  Everything behind the handle types is hidden from the dynamic symbol table (the Makefile sets no
// -fvisibility, so a non-static host function is exported otherwise): the library exports what it exported as one translation unit.
// g_build_mu, which api.hip has always exported, stays exported.  The thread-local state (pool owner, caller stream) is static in
// api.hip and reached through order_after_caller, order_caller_after and read_device_nnz; the last error's text is written through
// set_error alone and read as g_last_error.  What only the two batched files share has a header of its own, api_batch.h.
#pragma once

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <chrono>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "pool.h"
#include "plan_cache.h"

namespace ilupp {
extern std::mutex g_build_mu;      // api.hip
}  // namespace ilupp

using namespace ilupp;

enum { KIND_LU = 0, KIND_LLT = 1, KIND_UTU = 2 };     // UTU (ILUC): two factors whose arrays both read as an upper CSR matrix, diagonal first
enum { NNZ_GENERIC_LU = 0, NNZ_ILUT = 1, NNZ_LLT = 2 };

namespace ilupp {
// an object's queue: streams and events, recycled through a pool of their own (queue_take / queue_give)
struct QueuePack {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [4],[5]: around the factor kernel
    hipEvent_t sev[2] = {nullptr, nullptr};           // ordering against the caller's stream
    hipStream_t side = nullptr;                       // a second stream for work that runs NEXT to the analysis (grid.hip's proof)
    hipEvent_t jev[2] = {nullptr, nullptr};           // fork / join of the side stream
    int device = 0;
};
// what an object is, in its first three words whatever else it is made of: the CPU tests of the batched entries' refusals hand in zeroed
// memory with n in its third word for a handle -- hence a base of its own, in front of the queue pack
struct PrecondHead {
    int kind = KIND_LU;
    int nnz_mode = NNZ_GENERIC_LU;
    int32_t n = 0;
};
}  // namespace ilupp

struct ilupp_precond : ilupp::PrecondHead, ilupp::QueuePack {
    bool input_csc = false;      // factors were computed on the row-major view M = A^T
    // LU: row-major factors of M.  LLT: Lc = the factor in its stored major order, `llt_diag_last`
    DevMat Lc, Uc;
    bool llt_diag_last = true;
    DevMat LcT, UcT;             // transposed storage, built on first use
    bool haveT = false;
    Schedule sA, sL, sU, sUT, sLT;   // factor sweep; fwd(Lc); bwd(Uc); fwd(UcT); bwd(LcT)
    Ilu0Program prog;                // ILU(0) update program for sA (empty -> generic kernel)
    int32_t *prog_f3 = nullptr;      // fixed-size program (short-row matrices): loader/consumer kernel
    bool compact = false;            // descriptors/program usable (block size and grid within the encoding)
    bool no_static_T = false;        // the static form's transposed records were tried and declined
    bool pair_tried = false;         // static sweeps for the stored factor pair (LL^T objects) were tried
    bool chol_static = false;        // IChol(0) was computed by the static-form kernel (st.hip)
    int32_t *dL = nullptr, *dU = nullptr, *dUT = nullptr, *dLT = nullptr;   // solve descriptors
    PackedSweep pkL, pkU;            // level-major packed sweeps of Lc / Uc (short-row factors)
    PackedSweep pkUT, pkLT;          // ... of the transposed storages
    bool pack_tried[4] = {false, false, false, false};   // Lc, Uc, UcT, LcT: packing from the descriptors was attempted
    LevelSweep lvl[4];               // Lc, Uc, UcT, LcT in level order (long-row factors), built on first use
    int32_t *fperm = nullptr;        // ILU(0) of a long-row matrix: its rows in level order (ilu0_lvl.hip), also the forward sweep's order
    int32_t fperm_levels = 0;
    LevelNumbering fperm_how;        // ... and how it was numbered (diagnostics: ilupp_hip_debug_level_order)
    int8_t last_route[4] = {0, 0, 0, 0};   // per slot, the kernel family its last sweep ran on (SweepRoute; diagnostics)
    int8_t last_desc_kernel[4] = {0, 0, 0, 0};   // ... and, where that is SWEPT_DESCRIPTORS, the kernel: 1 k_sptrsv_lc, 2 k_sptrsv_desc (sptrsv())
    FactorLM flm;                    // level-major factor kernel state (then Lc.val / Uc.val are filled on demand)
    bool csr_vals = true;            // Lc.val / Uc.val hold the factor values
    int64_t nnzA = 0;                // stored entries of the factored matrix (same pattern on a numeric re-factorisation; ILU(0), IChol(0))
    int32_t max_row_len = 0;         // longest row of the factored matrix (LU objects) / of L (IChol(0)): what the batched launches route by
    int32_t max_len_T = 0;       // longest major slice of the transposed storages
    double *work = nullptr;      // n, all-sentinel between applies of the record-decoding / CSR sweeps (filled when the first of them runs)
    bool work_clean = false;
    double *xdev = nullptr;      // n, staging for host-vector apply
    int32_t *done = nullptr;     // n
    bool degenerate = false;     // a factor has a major slice without entries (NaN columns of an indefinite ICholT): guarded sweeps only
    int32_t *ctrl = nullptr;     // 16 ints: [0] err, [1] ilu0 ticket (+ its err in [2]) , [4],[5] solve tickets
    ilupp_timings tm = {0, 0, 0, 0, 0, 0};
    bool apply_events_valid = false;
    int max_lanes = 65536;
    bool icholt_grid = false;    // ICholT(0, 0.0): built by the speculative static kernel for box grids (icholt_grid.hip)
    GridDims llt_gd = {0, 0, 0};  // ... and the grid it was (the row-major copy for the sweeps follows from it)
    bool grid_path = false;      // ILU(0): the row blocks came from grid.hip's guess (proven for every row)
    // the plan cache (api.hip: plan_park): the grid this object's tables were made for; plan_ok: they are still what the analysis made and
    // nothing but plain, waited-for applies has happened since (set by the construction, cleared by whatever else touches the object);
    // apply_open: an apply was queued and no finish_apply has yet said that it went well
    GridDims grid_gd = {0, 0, 0};
    bool plan_ok = false, apply_open = false;
    bool no_general_retry = false;   // (ilupp_hip_ilu0_create_device_nnz) a grid guess that fails ends the attempt: the caller reads the head and starts over
    bool verdict_clean = false;  // ctrl[8] (the verdict word of grid.hip's proof) is zero already
    bool ctrl_armed = false;     // the control words are zero and both exchange buffers all-sentinel already (arm_apply): the next plain apply starts with its first sweep
    bool borrowed_queue = false; // stream and events belong to another object (the levels of a multilevel preconditioner share one)
    // block apply (ilupp_hip_apply_block*): buffers kept from one call to the next (grown, never shrunk), the route of the last one
    double *bxp = nullptr, *by = nullptr;   // n x bkb each: the hand-over buffer and the intermediate chunk of the level route
    int bkb = 0;
    double *bcol = nullptr;                 // n: one column of the columns route
    int32_t *btk = nullptr;                 // [0] a column's sweep timed out (columns route), [1 ..] two tickets per chunk (level route)
    int64_t btk_cap = 0;
    const char *block_path = "";
    bool block_events = false;              // the last apply was a block apply: ev[3] .. ev[2] bracket all of it
    hipEvent_t batch_ev = nullptr;          // a batched launch that was not waited for reads the factors (ilupp_hip_apply_batch_device, ilupp_hip_cg_batch_device): what a re-factorisation and the destruction wait for
    // ILU(0) built by the launches of a batched first construction (ilupp_hip_ilu0_create_batch*): Lc, Uc, nnzA and max_row_len, and nothing of
    // the single paths' analysis -- no sA / sU, no program, no packed sweeps, never the static form.  The batched launches take it as it
    // is; the single sweeps' tables (sL, sU, dL, dU) are built from the factors' own patterns on first use (ensure_sweep_tables)
    // IChol(0) built by ilupp_hip_ichol0_create_batch*: Lc, nnzA and max_row_len (the longest row of L) the same way; sL / dL on first use
    // ILUT built by ilupp_hip_ilut_create_batch* (KIND_LU / NNZ_ILUT): Lc and Uc with their values, max_row_len = the longest row of the two
    // (what sweep_tables gives the singly built object), and nothing else; no numeric re-factorisation exists for it, batch-built or not
    bool batch_built = false;
    bool sweeps_ready = false;
};
// (two bases with members: not a standard-layout type, so the order of the bases is the ABI's, not the language's -- checked here)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(ilupp_precond, kind) == 0 && offsetof(ilupp_precond, nnz_mode) == 4 && offsetof(ilupp_precond, n) == 8,
              "kind, nnz_mode and n are a handle's first three words");
#pragma clang diagnostic pop

// (api_pivot.hip's handle, here because the batched code reads its fields: BatchMember in api_batch.h takes obj, perm, tmp, n and batch_ev
// from it)
struct ilupp_ilucp {
    int32_t n = 0;
    bool input_csr = false;
    bool row_kind = false;                 // ILUTP: the factors belong to the ROWS of the view (L by rows, 1 last), the plain solve comes first for ROW input
    ilupp_precond *obj = nullptr;          // L and U' (permuted numbering), the sweeps
    DevMat U;                              // U as the reference stores it (original column indices): what factors() hands out
    int32_t *perm = nullptr;               // device
    double *tmp = nullptr, *xdev = nullptr;
    int32_t zero_pivots = 0;
    float kernel_ms = 0.f;
    hipEvent_t batch_ev = nullptr;         // a batched apply that was not waited for reads this member (and writes tmp): what the member's own stream waits for next
};

// (api_ml.hip's handle, here for the same reason: BatchMember takes n, obj, dev and buf from it.  The set of live ones, which its
// constructor keeps, is api_ml.hip's and hidden; is_live_ml asks it)
#pragma GCC visibility push(hidden)
namespace ilupp {
extern std::mutex g_ml_live_mu;
extern std::set<const void *> g_ml_live;
}  // namespace ilupp
#pragma GCC visibility pop
struct ilupp_ml {
    ilupp_ml() { std::lock_guard<std::mutex> lk(g_ml_live_mu); g_ml_live.insert(this); }
    ~ilupp_ml() { std::lock_guard<std::mutex> lk(g_ml_live_mu); g_ml_live.erase(this); }
    int32_t n = 0;
    std::vector<MlLevelDev> dev;              // per level: scalings, permutations, the middle diagonal (the factors move into `obj`)
    std::vector<ilupp_precond *> obj;         // per level: the sweeps of its two factors
    double *buf = nullptr;                    // n: what a sweep reads
    double *xdev = nullptr;                   // n: staging of host vectors
    float construct_ms = 0.f, kernel_ms = 0.f, last_apply_ms = 0.f;
};

// (from here on hidden: the handle types above keep the visibility they had, and with it their implicit constructors' weak symbols)
#pragma GCC visibility push(hidden)
namespace ilupp {

// one sweep's lane tables: the factor it runs over, its direction, where its schedule and descriptors go
struct SweepSpec { const DevMat *M; bool fwd; Schedule *s; int32_t **desc; };

// One sweep of one object: the stored triangle it walks (slot 0 = Lc, 1 = Uc, 2 = UcT, 3 = LcT: the numbering of pack_tried[] and lvl[])
// and the manner.  Whatever else a sweep needs follows from the slot: sweep_parts.
struct SweepOp { int slot; SweepKind kind; };
struct SweepParts {
    const DevMat &M; const Schedule &sch; const int32_t *desc; int32_t maxlen;      // the triangle, its schedule, descriptors, longest major slice
    PackedSweep *pk; bool *pack_tried;                                               // its level-major or static records
    LevelSweep *lvl;                                                                 // its renumbered copy in level order
};

// The two sweeps of an apply, in the order they run: the one place that knows which factor and which loop of the reference
// (sparse_implementation.h:4040-4087: T1 gather forward, T2 scatter forward, T3 gather backward, T4 scatter backward) every case takes.
// A scatter loop is a gather sweep over the transposed storage, T4 with the off-diagonal entries last-to-first (BWD_FIRST_DESC).
struct ApplyPlan {
    SweepOp first, second;
    // with the level-major factor path (every in-workgroup dependency one step back) the intermediate vector may travel level-major
    // between the two sweeps (first's ybuf, second's ysrc); y then only carries the values other workgroups poll
    bool ylm;
    bool transposed() const { return first.slot >= 2 || second.slot >= 2; }      // reads UcT or LcT
};

// what prepare_apply finds: the plan's sweeps, or one of the two static forms that take their place
enum ApplyRoute { ROUTE_SWEEPS, ROUTE_STATIC_T, ROUTE_STATIC_PAIR };

// ---- api.hip ----
extern thread_local std::string g_last_error;      // (read where a member's message is kept for the batch's report; written by set_error alone)
void order_after_caller(hipStream_t st, hipEvent_t ev);
void order_caller_after(hipStream_t st, hipEvent_t ev);
int32_t read_device_nnz(const int32_t *d_indptr, int32_t n);
int report(const HipError &e);
void queue_give(const QueuePack &q);
void destroy_obj(ilupp_precond *p);
ilupp_precond *new_obj(int32_t n);
int upload(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, bool is_csr, DevMat *A);
DevMat borrow_csr(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int64_t nnz, bool is_csr);
void host_head(const int32_t *indptr, const int32_t *indices, int64_t nnz, int32_t head[10]);
bool sweep_tables(hipStream_t st, const ilupp_precond *p, const SweepSpec &a, const SweepSpec &b, bool joint, int32_t *max_len);
void finish_timing(ilupp_precond *p, float kernel_ms, bool analysis_first = false);
void utu_analyse(ilupp_precond *p);
int apply_dev(ilupp_precond *p, double *x, int transpose);
int finish_apply(ilupp_precond *p);
// (what makes an object ready for its sweeps and the tables an apply reads them from: the multilevel apply and the batched launches'
// describing passes ask what the single apply asks)
void ensure_csr_values(ilupp_precond *p);
void ensure_transposed(ilupp_precond *p);
SweepParts sweep_parts(ilupp_precond *p, SweepOp op);
ApplyPlan apply_plan(int kind, bool transpose, bool input_csc, bool llt_diag_last);
ApplyPlan apply_plan(const ilupp_precond *p, int transpose);
const PackedSweep *packed(ilupp_precond *p, SweepOp op);
int sweep(ilupp_precond *p, SweepOp op, const PackedSweep *ps, double *rhs, double *out, int32_t *ticket, int32_t *err, double *ypk_out = nullptr, const double *ypk_in = nullptr, const int32_t *ysrc = nullptr);
ApplyRoute prepare_apply(ilupp_precond *p, const ApplyPlan &plan, PackedSweep **pf, PackedSweep **pb);
// (the single constructions and re-factorisations that the batched ones run for the members that stay out of their launches)
int ilu0_create_common(const DevMat &A, int is_csr, const int32_t *head, ilupp_precond **out, ilupp_precond *made = nullptr);
int ilu0_create_device_locked(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int is_csr, ilupp_precond **out);
int ilut_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out, ilupp_precond *made = nullptr);
int ichol0_create_common(DevMat &A, int32_t n, ilupp_precond **out, ilupp_precond *made = nullptr);
bool is_ilu0_object(const ilupp_precond *p);
bool is_ichol0_object(const ilupp_precond *p);
int ilu0_refactor_single(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr);
int ichol0_refactor_single(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr);
void drop_old_value_copies(ilupp_precond *p);
void drop_llt_sweep_copies(ilupp_precond *p);
// ---- api_ml.hip (batch_build: the workers of a batched construction, of the multilevel batch first, of the pivoting batches since) ----
bool is_live_ml(const void *h);
int ml_apply_dev(ilupp_ml *m, double *x, int transpose, int part = 0);
int ml_finish_apply(ilupp_ml *m);
int no_batch_stream();
int batch_first_failure(int32_t count, const std::vector<int> &rcs, const std::vector<std::string> &msgs, int32_t *status);
int batch_build(int32_t count, double worst_bytes, int32_t *status, const std::function<int(int32_t)> &build);
// ---- api_batch_build.hip (the launch of the batched re-factorisation with this one member: the single re-factorisation of a batch-built
// object, which has none of the single numeric paths' tables) ----
int refactor_in_launch(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr);
// ---- api_pivot.hip (pivot_apply_dev: the single device apply of a pivoting member, which the batched apply runs for the members it
// does not launch) ----
bool pivot_plain_first(const ilupp_ilucp *m, int transpose);
int pivot_apply_dev(ilupp_ilucp *m, double *x, int transpose);

inline bool schedule_is_compact(const Schedule &s) { return s.B <= 32768 && s.nslots <= kGhostBase; }

// an object under construction: destroyed (its side stream synchronised, its pool blocks given back) when the construction unwinds --
// a HIP error thrown from the middle of a factorisation or an analysis leaves nothing behind
struct ObjGuard {
    ilupp_precond *p;
    explicit ObjGuard(ilupp_precond *q) : p(q) {}
    ~ObjGuard() { if (p) { if (p->side) (void)stream_sync(p->side); destroy_obj(p); } }
    ilupp_precond *release() { ilupp_precond *q = p; p = nullptr; return q; }
    ObjGuard(const ObjGuard &) = delete;
    ObjGuard &operator=(const ObjGuard &) = delete;
};

// a device matrix this scope owns: released when it unwinds (or earlier, by whoever calls m.release())
struct MatGuard {
    DevMat m;
    MatGuard() = default;
    ~MatGuard() { m.release(); }
    MatGuard(const MatGuard &) = delete;
    MatGuard &operator=(const MatGuard &) = delete;
};

}  // namespace ilupp

#define OR_RETURN(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

#define API_TRY try {
// every construction / re-factorisation of the process, one after the other: the memory pool knows nothing of streams -- a block that
// one construction gives back may still be in use on ITS stream when another thread's construction is handed it.  (Every
// construction synchronises its stream before it returns, so the lock costs a concurrent caller what the construction costs.)
#define API_TRY_BUILD try { std::lock_guard<std::mutex> build_lock_(ilupp::g_build_mu);
#define API_CATCH                                                          \
    } catch (const ilupp::HipError &e) { ilupp::d2h_cancel_all(); return ilupp::report(e); }        \
    catch (const std::bad_alloc &) { ilupp::d2h_cancel_all(); ilupp::set_error("out of host memory"); return ILUPP_ERR_MEMORY; }

// ---- what an entry of each shape is made of ----------------------------------------------------------------------------------------
namespace ilupp {

// A construction entry on host arrays: the triple copied to device memory this call owns, then `make(A)`.  args_ok / null_msg: what
// else of the entry's arguments must not be null, and how the refusal reads (the multilevel entries: "null argument").
template <class Handle, class Make>
int create_from_host(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, bool is_csr, Handle **out, Make &&make,
                     bool args_ok = true, const char *null_msg = "null output")
{
    API_TRY_BUILD
    if (!out || !args_ok) { set_error(null_msg); return ILUPP_ERR_INVALID; }
    *out = nullptr;
    MatGuard A;
    OR_RETURN(upload(data, indices, indptr, n, is_csr, &A.m));
    return make(A.m);
    API_CATCH
}

// ... on a matrix that already lives in HBM: the caller's arrays, borrowed for the call; indptr[n] is read back
template <class Handle, class Make>
int create_from_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, bool is_csr, Handle **out, Make &&make,
                       bool args_ok = true, const char *null_msg = "null output")
{
    API_TRY_BUILD
    if (!out || !args_ok) { set_error(null_msg); return ILUPP_ERR_INVALID; }
    *out = nullptr;
    if (n <= 0 || !d_indptr) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
    DevMat A = borrow_csr(d_data, d_indices, d_indptr, n, read_device_nnz(d_indptr, n), is_csr);
    return make(A);
    API_CATCH
}

// the handle and the length of the vector an apply entry is given (n: the handle's, 0 for none)
inline int vector_args(const void *handle, int64_t len, int32_t n)
{
    if (!handle) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
    if (len != n) { set_error("vector has wrong size for preconditioner!"); return ILUPP_ERR_WRONG_SIZE; }   // binding.cpp:241-242
    return ILUPP_OK;
}

// the end of a device apply queued on q: wait for it and say how it went (finish), or hand the result over to the caller's stream
template <class Finish>
int finish_or_hand_over(int sync, const QueuePack &q, Finish &&finish)
{
    if (sync) return finish();
    order_caller_after(q.stream, q.sev[1]);
    return ILUPP_OK;
}

// The apply of a host vector: staged in *slot (n doubles, allocated on first use), sent on the object's stream, apply(staged vector),
// finish(), and a blocking copy back -- from `result` where the apply leaves its result elsewhere than in the staged vector.
template <class Apply, class Finish>
int apply_staged(hipStream_t st, double **slot, int32_t n, double *x, Apply &&apply, Finish &&finish, const double *result = nullptr)
{
    if (!*slot) ILUPP_HIP(pool_malloc(slot, sizeof(double) * (size_t)n));
    ILUPP_HIP(hipMemcpyAsync(*slot, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    OR_RETURN(apply(*slot));
    OR_RETURN(finish());
    ILUPP_HIP(hipMemcpy(x, result ? result : *slot, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return ILUPP_OK;
}

// an optional host array of a handle's copy-out entry
inline void get_host(void *dst, const void *src, size_t bytes)
{
    if (dst && bytes) ILUPP_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
}

}  // namespace ilupp

#pragma GCC visibility pop
