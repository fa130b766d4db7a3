// ilupp_amd/csrc/api.hip -- the C ABI (include/ilupp_hip.h): object lifetime, dispatch of apply() to the sweep kernels, factor egress,
// the constructions of an ilupp_precond, the multilevel preconditioner and the batched tables.  The pivoting preconditioners (ILUCP /
// ILUTP) have a file of their own, api_pivot.hip; api_internal.h holds what the two files share (DESIGN_OTHER_PATHS.md section
// 4h.13).  Mirrors the reference's binding layer (src/binding.cpp) and L2 dispatch (preconditioner_implementation.h:103-111,
// :321-334, :381-394).
#include "api_internal.h"

namespace ilupp {
std::mutex g_build_mu;

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

void DevMat::release()
{
    if (owns) {
        if (ptr) (void)pool_free(ptr);
        if (idx) (void)pool_free(idx);
        if (val) (void)pool_free(val);
    }
    ptr = idx = nullptr; val = nullptr; nnz = 0;
}
void Schedule::release()
{
    if (start) (void)pool_free(start);
    if (slot2blk) (void)pool_free(slot2blk);
    if (blk2slot) (void)pool_free(blk2slot);
    if (sfirst) (void)pool_free(sfirst);
    if (scount) (void)pool_free(scount);
    if (exported) (void)pool_free(exported);
    if (gtab) (void)pool_free(gtab);
    start = slot2blk = blk2slot = sfirst = scount = exported = gtab = nullptr; nb = 0; nslots = 0;
}
void Ilu0Program::release()
{
    if (prow) (void)pool_free(prow);
    if (prog) (void)pool_free(prog);
    prow = prog = nullptr; nwords = 0;
}

// ---- pooled device memory (pool.h) ------------------------------------------------------------
namespace {
int be_alloc(void **p, size_t bytes)
{
    const hipError_t e = ::hipMalloc(p, bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return (int)e;
}
int be_release(void *p) { return (int)::hipFree(p); }
int be_device() { int dev = 0; (void)hipGetDevice(&dev); return dev; }      // a kept block is only ever handed back on the GPU it lives on
size_t default_cache_limit()
{
    // ILUC on a 256^3 mesh keeps 2 x 17 GB of touch records per attempt (with 24 GB they went back to the driver every time, 0.96 s
    // of its 1.25 s); a process that shares the GPU lowers the limit (ilupp_hip_set_cache_limit, ILUPP_CACHE_LIMIT_MB)
    const char *s = getenv("ILUPP_CACHE_LIMIT_MB");
    if (s && *s) return (size_t)strtoull(s, nullptr, 10) << 20;
    return (size_t)48 << 30;
}
BlockPool &pool()
{
    static BlockPool g(PoolBackend{be_alloc, be_release, be_device}, default_cache_limit());
    return g;
}
}  // namespace

// the owner lane of the calling thread (pool.h): 0 except inside a worker of a batched construction
static thread_local int g_pool_owner = 0;
void pool_set_owner(int owner) { g_pool_owner = owner; }
void pool_disown(int owner) { pool().disown(owner); }

hipError_t pool_malloc(void **p, size_t bytes)
{
    const int e = pool().acquire(p, bytes, g_pool_owner);
    return e == 0 ? hipSuccess : (hipError_t)e;
}

hipError_t pool_free(void *p)
{
    const int e = pool().release(p, g_pool_owner);
    if (e == BlockPool::kNotLive) {
        // never ignored: a block freed twice may meanwhile belong to somebody else
        set_error("internal error: a device block was released that the pool had not handed out (double release?)");
        return hipErrorInvalidValue;
    }
    return e == 0 ? hipSuccess : hipErrorUnknown;
}

void pool_trim() { pool().trim(); }
void pool_set_limit(size_t bytes) { pool().set_limit(bytes); }
size_t pool_cached_bytes() { return pool().cached(); }
size_t pool_live_blocks() { return pool().live_blocks(); }

// Ordering against the caller's own HIP stream (device-pointer entry points): when set for this thread, every *_device
// call first makes the object's queue wait for the work already submitted to that stream (the producer of the matrix /
// the vector), and an asynchronous apply makes that stream wait for the result.
static thread_local hipStream_t g_caller_stream = nullptr;
static thread_local bool g_caller_stream_set = false;
void order_after_caller(hipStream_t st, hipEvent_t ev)
{
    if (!g_caller_stream_set) return;
    ILUPP_HIP(hipEventRecord(ev, g_caller_stream));
    ILUPP_HIP(hipStreamWaitEvent(st, ev, 0));
}
void order_caller_after(hipStream_t st, hipEvent_t ev)
{
    if (!g_caller_stream_set) return;
    ILUPP_HIP(hipEventRecord(ev, st));
    ILUPP_HIP(hipStreamWaitEvent(g_caller_stream, ev, 0));
}

// indptr[n] of a device-resident matrix.  Ordered after the work the caller has submitted to its stream when one is set (the
// producer of the arrays: a blocking copy on the null stream does not wait for a non-blocking stream)
int32_t read_device_nnz(const int32_t *d_indptr, int32_t n)
{
    int32_t v = 0;
    if (g_caller_stream_set) {
        ILUPP_HIP(hipMemcpyAsync(&v, d_indptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, g_caller_stream));
        ILUPP_HIP(hipStreamSynchronize(g_caller_stream));
    } else {
        ILUPP_HIP(hipMemcpy(&v, d_indptr + n, sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return v;
}

// indptr[n] plus {indptr[0], indptr[1], indices[0..7]} (-1 where the matrix has no such entry) with ONE read-back
__global__ void k_read_head(const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, int32_t n, int32_t *__restrict__ out,
                            int32_t *__restrict__ zero)
{
    const int t = threadIdx.x;
    const int32_t nnz = ptr[n];
    if (t == 63 && zero) *zero = 0;               // (the verdict word of grid.hip's proof: clean before anything is launched)
    if (t == 0) out[0] = nnz;
    if (t == 1) out[1] = ptr[0];
    if (t == 2) out[2] = ptr[1];
    if (t >= 3 && t < 11) out[t] = (t - 3 < nnz) ? idx[t - 3] : -1;
}
static int32_t read_device_head(const int32_t *d_indptr, const int32_t *d_indices, int32_t n, int32_t *head, int32_t *d_zero = nullptr)
{
    static int32_t *stage = nullptr;         // pinned, mapped: the kernel writes where the host reads
    static int32_t *stage_dev = nullptr;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!stage) {
        ILUPP_HIP(hipHostMalloc(reinterpret_cast<void **>(&stage), 64, hipHostMallocMapped | hipHostMallocPortable));
        ILUPP_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&stage_dev), stage, 0));
    }
    hipStream_t s = g_caller_stream_set ? g_caller_stream : nullptr;
    hipLaunchKernelGGL(k_read_head, dim3(1), dim3(64), 0, s, d_indptr, d_indices, n, stage_dev, d_zero);
    ILUPP_HIP(hipGetLastError());
    ILUPP_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 10; ++i) head[i] = stage[1 + i];
    return stage[0];
}

int report(const HipError &e)
{
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s at %s:%d", (int)e.code, hipGetErrorString(e.code), e.what, e.file, e.line);
    set_error(buf);
    return ILUPP_ERR_HIP;
}

}  // namespace ilupp

namespace {

// streams and events are recycled: creating them costs more than a small kernel
struct QueuePool { std::mutex mu; std::vector<QueuePack> free_list; } g_queues;

// a kept pack of `device` into *q (false: none is kept)
bool queue_take(int device, QueuePack *q)
{
    std::lock_guard<std::mutex> lk(g_queues.mu);
    for (size_t k = 0; k < g_queues.free_list.size(); ++k)
        if (g_queues.free_list[k].device == device) {
            *q = g_queues.free_list[k];
            g_queues.free_list.erase(g_queues.free_list.begin() + (long)k);
            return true;
        }
    return false;
}

// ---- parked plans (plan_cache.h) ----------------------------------------------------------------------------------------------------
// Everything the analysis of a box-grid ILU(0) object makes from the three dimensions alone -- both schedules with their slot tables, the
// lane, chunk, exchange and link tables of both sweeps, the factor kernel's lane records -- is MOVED out of such an object when it is
// destroyed and into the next object of the same (device, n, nnz, nx, ny, nz): a caller that builds the preconditioner of one mesh anew
// every time step runs k_grid_starts / k_grid_lanes / k_grid_scat and their read-back once.  The tables hold slots, offsets and counts,
// no address of a value buffer: records, level-major vectors and exchange buffers go back to the pool as ever and come out of it again
// by the sizes the plan keeps (st.hip: st_alloc_values).  What makes adopted tables valid for the matrix at hand is what makes built ones
// valid: the proof of the pattern, which runs in every construction.
struct GridPlan {
    Schedule sA, sU;
    PackedSweep pkL, pkU;           // (table members and sizes; no records, vectors, exchange buffers)
    FactorLM flm;                   // (xbase, the flags, the predicted and the found sizes)
    int32_t max_row_len = 0;
    bool compact = false;
    int64_t nnzL = 0, nnzU = 0;
};
typedef PlanCache<GridPlan> Plans;
void plan_block_release(void *h) { (void)pool_free(h); }
Plans &plans()
{
    (void)pool();                        // (made first, destroyed last: the plans that are parked when the process ends go back to it)
    static Plans g(plan_block_release, 4);
    return g;
}
// ILUPP_NO_PLAN_CACHE=1: nothing is parked or adopted; nor under a switch that selects an older piece of the analysis
bool plan_cache_on()
{
    static const bool on = []() {
        for (const char *name : {"ILUPP_NO_PLAN_CACHE", "ILUPP_NO_GRID", "ILUPP_NO_SPEC", "ILUPP_NO_WXF", "ILUPP_NO_WR", "ILUPP_SD_VERIFY", "ILUPP_CLASSIC_ANALYSIS"})
            if (getenv(name) != nullptr) return false;
        for (const char *name : {"ILUPP_GRID_TABLES", "ILUPP_GRID_LINK", "ILUPP_GRID_SCAT"}) {
            const char *e = getenv(name);
            if (e && atoi(e) == 0) return false;
        }
        return true;
    }();
    return on;
}
// every pointer of the five structures that is a table of the plan (f: called with a reference to each)
template <class F>
void plan_tables(Schedule &sa, Schedule &su, PackedSweep &pl, PackedSweep &pu, FactorLM &flm, F &&f)
{
    for (Schedule *s : {&sa, &su}) { f(s->start); f(s->slot2blk); f(s->blk2slot); f(s->sfirst); f(s->scount); f(s->exported); f(s->gtab); }
    for (PackedSweep *k : {&pl, &pu}) { f(k->ltab); f(k->skew); f(k->wtab); f(k->flags); f(k->uslot); f(k->ysrc); f(k->xe); f(k->xw); f(k->dump); }
    f(flm.xbase);
}
// An object on the headline path -- grid analysis, static direct feed, the wave-exchange factor kernel with predicted sizes -- whose
// tables are what the analysis made: built (or adopted) by a construction that went well, and since then nothing but plain applies that
// were waited for and went well, and factors() (which turns the records back and forth and makes CSR arrays of the object's own: values,
// and they go to the pool; the record format is a flag the next factor kernel sets).  Everything else is excluded: a re-factorisation, a
// transposed apply, an apply nobody waited for, a batched launch in flight, a call that ended in an error.
bool plan_parkable(const ilupp_precond *p)
{
    if (!plan_cache_on() || !p->plan_ok || p->apply_open || p->batch_ev || p->batch_built || p->borrowed_queue || p->icholt_grid || p->degenerate) return false;
    if (!(p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU && p->grid_path && p->grid_gd.nx > 0 && p->stream)) return false;
    const FactorLM &f = p->flm;
    if (!(f.built && f.stat && f.direct && f.wxf && f.spec && f.xbase) || f.pkA || f.xch || f.xcount) return false;
    if (!(p->pkL.valid && p->pkU.valid && p->pkL.stat && p->pkU.stat) || p->pkL.pkT || p->pkU.pkT || p->pkL.pair || p->pkU.pair) return false;
    return ilu0_numeric_st_is_wx(p->pkL, f);
}
PlanKey plan_key(int device, int32_t n, int64_t nnz, const GridDims &g)
{
    PlanKey k;
    k.device = device; k.n = n; k.nnz = nnz; k.nx = g.nx; k.ny = g.ny; k.nz = g.nz;
    return k;
}
// destroy_obj, behind its wait for the stream: the tables leave the object (which releases the rest as ever) for the cache -- or for the
// pool, where the cache refuses them: the plans' bytes count against the pool's limit, with what the pool keeps
void plan_park(ilupp_precond *p)
{
    Plans::Plan plan;
    plan.key = plan_key(p->device, p->n, p->nnzA, p->grid_gd);
    GridPlan &g = plan.payload;
    g.sA = p->sA; g.sU = p->sU; g.pkL = p->pkL; g.pkU = p->pkU; g.flm = p->flm;
    g.max_row_len = p->max_row_len; g.compact = p->compact; g.nnzL = p->Lc.nnz; g.nnzU = p->Uc.nnz;
    for (PackedSweep *k : {&g.pkL, &g.pkU}) {
        k->pk = nullptr; k->ybuf = nullptr; k->xlm = nullptr; k->xch = nullptr; k->pkT = nullptr;
        k->fmt = k->fmtT = 0; k->xch_armed = false;
    }
    plan_tables(g.sA, g.sU, g.pkL, g.pkU, g.flm, [&](auto *&t) { if (t) plan.blocks.push_back(PlanBlock{t, pool().live_bytes(t)}); });
    plan_tables(p->sA, p->sU, p->pkL, p->pkU, p->flm, [](auto *&t) { t = nullptr; });
    const size_t limit = pool().limit(), kept = pool_cached_bytes();
    (void)plans().park(std::move(plan), limit > kept ? limit - kept : 0);
}
// ilu0_factor, with the dimensions guessed: the parked plan of that shape becomes this object's analysis (false: none is parked)
bool plan_adopt(ilupp_precond *p, const DevMat &A, const GridDims &gd)
{
    if (!plan_cache_on() || p->batch_built || p->borrowed_queue) return false;
    Plans::Plan plan;
    if (!plans().take(plan_key(p->device, A.n, A.nnz, gd), &plan)) return false;
    const GridPlan &g = plan.payload;
    p->pkL.release(); p->pkU.release(); p->flm.release(); p->sA.release(); p->sU.release();
    p->sA = g.sA; p->sU = g.sU; p->pkL = g.pkL; p->pkU = g.pkU; p->flm = g.flm;      // (the object owns the tables from here on, whatever follows)
    p->max_row_len = g.max_row_len; p->compact = g.compact;
    for (DevMat *M : {&p->Lc, &p->Uc}) { M->n = A.n; M->is_csr = true; M->owns = true; }
    p->Lc.nnz = g.nnzL; p->Uc.nnz = g.nnzU;
    st_alloc_values(&p->pkL, &p->pkU);
    return true;
}

}  // namespace

// (what api_pivot.hip and the templates of api_internal.h call, and what goes with it: declared ilupp:: names)
namespace ilupp {

// ... and a pack that nothing uses any more back into the pool
void queue_give(const QueuePack &q)
{
    std::lock_guard<std::mutex> lk(g_queues.mu);
    g_queues.free_list.push_back(q);
}

void destroy_obj(ilupp_precond *p)
{
    if (!p) return;
    if (p->batch_ev && p->stream) (void)hipStreamWaitEvent(p->stream, p->batch_ev, 0);      // (a batched launch may still read the factors)
    const bool idle = p->stream && stream_sync(p->stream) == hipSuccess;   // pooled blocks may be handed out again at once
    if (idle && plan_parkable(p)) plan_park(p);       // (the dimension-derived tables: to the next object of this shape)
    p->Lc.release(); p->Uc.release(); p->LcT.release(); p->UcT.release();
    p->sA.release(); p->sL.release(); p->sU.release(); p->sUT.release(); p->sLT.release();
    p->prog.release();
    p->pkL.release(); p->pkU.release(); p->pkUT.release(); p->pkLT.release(); p->flm.release();
    for (auto &l : p->lvl) l.release();
    if (p->fperm) (void)pool_free(p->fperm);
    if (p->prog_f3) (void)pool_free(p->prog_f3);
    for (int32_t *d : {p->dL, p->dU, p->dUT, p->dLT}) if (d) (void)pool_free(d);
    if (p->work) (void)pool_free(p->work);
    if (p->xdev) (void)pool_free(p->xdev);
    for (void *q : {(void *)p->bxp, (void *)p->by, (void *)p->bcol, (void *)p->btk}) if (q) (void)pool_free(q);
    if (p->done) (void)pool_free(p->done);
    if (p->ctrl) (void)pool_free(p->ctrl);
    // (not a pack new_obj could not finish: jev[1] comes last)
    if (p->stream && !p->borrowed_queue && p->jev[1]) queue_give(*p);
    delete p;
}

ilupp_precond *new_obj(int32_t n)
{
    ObjGuard g(new ilupp_precond());
    ilupp_precond *p = g.p;
    p->n = n;
    ILUPP_HIP(hipGetDevice(&p->device));
    if (!queue_take(p->device, p)) {
        ILUPP_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        for (auto &e : p->ev) ILUPP_HIP(hipEventCreate(&e));
        for (auto &e : p->sev) ILUPP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ILUPP_HIP(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
        for (auto &e : p->jev) ILUPP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    order_after_caller(p->stream, p->sev[0]);        // (the matrix a *_create_device call is about to read)
    ILUPP_HIP(pool_malloc(&p->work, sizeof(double) * (size_t)n));
    ILUPP_HIP(pool_malloc(&p->done, sizeof(int32_t) * (size_t)n));
    ILUPP_HIP(pool_malloc(&p->ctrl, 64));
    // Lanes a schedule may spread over.  NOT the lanes of the chip: every kernel takes its workgroup id from a ticket counter
    // and only waits for rows of lower tickets, which have started by then, so a grid larger than the chip makes progress;
    // what matters is that a lane's block of rows is one dependency chain (a mesh line).  With the chip's 65 536 lanes as the
    // limit, a 288^3 mesh (82 944 lines) got blocks of 365 rows that straddled lines, every lane waited for its predecessor
    // to finish, and the sweeps ran into their spin limits.
    p->max_lanes = 1 << 24;
    return g.release();
}

static int validate(const int32_t *indptr, int32_t n)
{
    if (n <= 0 || indptr == nullptr) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }   // binding.cpp:80-81
    return ILUPP_OK;
}

// a host CSR/CSC triple copied to pooled device memory, into *A (owned by the caller: a MatGuard, the solve's Guard)
int upload(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, bool is_csr, DevMat *A)
{
    const int rc = validate(indptr, n);
    if (rc) return rc;
    const int64_t nnz = indptr[n];
    A->n = n; A->nnz = nnz; A->is_csr = is_csr; A->owns = true;
    ILUPP_HIP(pool_malloc(&A->ptr, sizeof(int32_t) * (size_t)(n + 1)));
    ILUPP_HIP(pool_malloc(&A->idx, sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1)));
    ILUPP_HIP(pool_malloc(&A->val, sizeof(double) * (size_t)(nnz > 0 ? nnz : 1)));
    ILUPP_HIP(hipMemcpy(A->ptr, indptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
    ILUPP_HIP(hipMemcpy(A->idx, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    ILUPP_HIP(hipMemcpy(A->val, data, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
    return ILUPP_OK;
}

// the caller's device arrays, borrowed for the call (never released)
DevMat borrow_csr(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int64_t nnz, bool is_csr)
{
    DevMat A;
    A.n = n; A.nnz = nnz; A.is_csr = is_csr; A.owns = false;
    A.ptr = const_cast<int32_t *>(d_indptr); A.idx = const_cast<int32_t *>(d_indices); A.val = const_cast<double *>(d_data);
    return A;
}

// what read_device_head reads, from host arrays: {indptr[0], indptr[1], indices[0..7]} (-1 where the matrix has no such entry)
void host_head(const int32_t *indptr, const int32_t *indices, int64_t nnz, int32_t head[10])
{
    head[0] = indptr[0]; head[1] = indptr[1];
    for (int i = 0; i < 8; ++i) head[2 + i] = i < nnz ? indices[i] : -1;
}

// the lane tables of one sweep, or of two (b.M != nullptr) stage by stage: cuts and schedules, tilings, slot tables, descriptors.
// Descriptors need a compact schedule: joint = for both sweeps or for neither, else each sweep for itself.  *max_len = the longest
// major slice of the factors; returns whether every schedule is compact.
bool sweep_tables(hipStream_t st, const ilupp_precond *p, const SweepSpec &a, const SweepSpec &b, bool joint, int32_t *max_len)
{
    const SweepSpec *sw[2] = {&a, b.M ? &b : nullptr};
    int32_t m[2] = {0, 0};
    for (int k = 0; k < 2; ++k)
        if (sw[k]) count_cuts_and_schedule(st, p->n, sw[k]->M->ptr, sw[k]->M->idx, p->max_lanes, sw[k]->fwd ? sw[k]->s : nullptr,
                                           sw[k]->fwd ? nullptr : sw[k]->s, &m[k]);
    *max_len = m[0] > m[1] ? m[0] : m[1];
    for (const SweepSpec *w : sw) if (w) choose_tiling(st, p->n, w->M->ptr, w->M->idx, w->s, w->fwd, p->max_lanes / kThreads);
    for (const SweepSpec *w : sw) if (w) build_slot_tables(st, w->s, w->fwd);
    const bool c[2] = {schedule_is_compact(*a.s), !sw[1] || schedule_is_compact(*b.s)};
    for (int k = 0; k < 2; ++k)
        if (sw[k] && (joint ? c[0] && c[1] : c[k])) make_desc(st, *sw[k]->M, *sw[k]->s, sw[k]->desc);
    return c[0] && c[1];
}

// the end of a construction: its last event, the wait for it, the times of its two phases -- [ev[0], ev[1]) is the numeric
// factorisation and [ev[1], ev[2]) the analysis, or the other way round (IChol(0) analyses first)
void finish_timing(ilupp_precond *p, float kernel_ms, bool analysis_first)
{
    ILUPP_HIP(hipEventRecord(p->ev[2], p->stream));
    ILUPP_HIP(stream_sync(p->stream));
    ILUPP_HIP(hipEventElapsedTime(analysis_first ? &p->tm.analysis_ms : &p->tm.numeric_ms, p->ev[0], p->ev[1]));
    ILUPP_HIP(hipEventElapsedTime(analysis_first ? &p->tm.numeric_ms : &p->tm.analysis_ms, p->ev[1], p->ev[2]));
    p->tm.numeric_kernel_ms = kernel_ms;
}

}  // namespace ilupp

namespace {

// What a plain apply of a static ILU(0) object needs before its first sweep -- control words zero, both exchange buffers all-sentinel --
// as ONE launch BEHIND the last wait of the call before (construction, apply): it runs while the host is on its way back to the caller,
// and the next apply is two launches, the sweeps.  (Before: a memset, two fills and their launch gaps inside every apply, 30 us of a 0.7 ms apply.)
__global__ void k_arm_apply(int32_t *__restrict__ ctrl, unsigned long long *__restrict__ a, long long na, unsigned long long *__restrict__ b,
                            long long nb, unsigned long long v)
{
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (i0 < 16) ctrl[i0] = 0;
    for (long long i = i0; i < na; i += stride) a[i] = v;
    for (long long i = i0; i < nb; i += stride) b[i] = v;
}
static void arm_apply(ilupp_precond *p)
{
    static const bool off = getenv("ILUPP_NO_ARM") != nullptr;
    if (off || !(p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU && p->flm.built && p->flm.stat && p->pkL.valid && p->pkU.valid &&
                 p->pkL.fmt >= 1 && p->pkU.fmt == 1 && p->pkL.xch && p->pkU.xch && !p->degenerate)) return;
    hipLaunchKernelGGL(k_arm_apply, dim3(1024), dim3(256), 0, p->stream, p->ctrl, reinterpret_cast<unsigned long long *>(p->pkL.xch),
                       (long long)p->pkL.xch_len, reinterpret_cast<unsigned long long *>(p->pkU.xch), (long long)p->pkU.xch_len, kSentinel);
    if (hipGetLastError() != hipSuccess) return;
    p->ctrl_armed = true; p->pkL.xch_armed = p->pkU.xch_armed = true;
}

// Behind a factor kernel: the control words as a sync() and the next apply expect them.  The wave-exchange objects get the whole apply armed
// (arm_apply).  Every other factor kernel counts its workgroups in ctrl[0], the word the sweeps report a timeout through: a sync() that
// comes before the next apply -- behind device applies or a batched launch that were not waited for -- must not read that count as a
// sweep that gave up.
static void settle_ctrl(ilupp_precond *p)
{
    if (!p->ctrl_armed) arm_apply(p);
    if (!p->ctrl_armed) ILUPP_HIP(hipMemsetAsync(p->ctrl, 0, 16, p->stream));
}

// numeric phase with whatever machinery the analysis could set up; leaves the sweep records' values in place (gp: common.h, GridProof)
static int ilu0_numeric_any(ilupp_precond *p, const DevMat &A, bool have_prog, float *kms, GridProof *gp)
{
    hipStream_t st = p->stream;
    p->ctrl_armed = false; p->pkL.xch_armed = p->pkU.xch_armed = false;      // (the factor kernels use the control words and the forward exchange)
    p->plan_ok = false;                  // (a construction that goes well sets it again: ilu0_factor; a re-factorisation never)
    int rc = ILUPP_ERR_UNSUPPORTED;
    if (p->flm.built) {
        // (flm.built means the static form: round 1's record-decoding level-major FACTOR kernel, which only matrices the static form takes
        // ever reached -- and then only under ILUPP_NO_STATIC --, was removed in round 5)
        rc = ilu0_numeric_st(st, A, &p->pkL, &p->pkU, &p->flm, p->ctrl, kms, p->ev[4], p->ev[5], gp);
        p->csr_vals = false;
        return rc;
    }
    p->csr_vals = true;
    if (p->fperm) {
        rc = ilu0_numeric_lvl(st, A, &p->Lc, &p->Uc, p->fperm, p->ctrl, kms);
    } else if (p->prog_f3) {
        // (letting this kernel scatter the sweep records itself cost more than the separate value pass below)
        rc = ilu0_numeric_lc(st, A, &p->Lc, &p->Uc, p->sA, p->prog_f3, p->ctrl, kms, nullptr, nullptr);
    } else if (have_prog) {
        rc = ilu0_numeric_program(st, A, &p->Lc, &p->Uc, p->sA, p->prog, p->max_row_len, p->ctrl, kms);
    }
    if (rc == ILUPP_ERR_UNSUPPORTED) {
        rc = ilu0_numeric(st, A, &p->Lc, &p->Uc, p->sA, p->max_row_len, p->done, p->ctrl, kms);
    }
    // the level-major sweeps of this object keep their own copy of the values: every one that exists gets the new ones
    // (they are built independently, on first use, so one may exist without the other)
    if (p->pkL.valid && !p->pkL.stat) lm_pack(st, SWEEP_FWD_LAST_ASC, p->Lc, p->sL.start ? p->sL : p->sA, p->dL, &p->pkL, 2);
    if (p->pkU.valid && !p->pkU.stat) lm_pack(st, SWEEP_BWD_FIRST_ASC, p->Uc, p->sU, p->dU, &p->pkU, 2);
    return rc;
}

// The steps of ilu0_factor, in its order.  A grid attempt begins (false: no guess, *gp stays NOT_A_GRID):
// a matrix whose row 0 and entry count are those of a lexicographic box-grid stencil (grid.hip): the row blocks follow from the
// three dimensions, and ONE streaming kernel on the side stream proves the guess for every row while the lane tables are built.
// Its verdict comes home with the construction's last read-back.  (Measured at 256^3: k_grid_lanes only stores and the skew fixpoint
// lives in LDS, so they lose little next to the 4.6 TB/s stream of the proof; DESIGN.md section 4.0.2 has the other placements.)
// (a grid whose factor launch holds one workgroup per CU: that launch proves the pattern itself, on the CUs whose tile has ended --
// st_wave.hip: wa_tail_proof --, and nothing runs on the side stream)
// (*adopted: a plan of that shape was parked -- plan_adopt -- and is this object's analysis now: schedules, slot tables and lane tables are
// there, no launch was made for them; where the factor launch will hold the proof, its preparing launch clears the verdict word as well --
// st_wave.hip: k_wa_prepare --, and nothing at all is queued here)
static bool grid_attempt_begin(ilupp_precond *p, const DevMat &A, const int32_t *head, GridProof *gp, int max_wgs, bool *adopted)
{
    *adopted = false;
    if (head == nullptr || p->side == nullptr || !grid_guess(A.n, A.nnz, head, &gp->g)) return false;
    gp->how = wx_tail_proof_wanted(gp->g.ny, gp->g.nz) ? GridProof::FACTOR_LAUNCH : GridProof::SIDE_STREAM;
    gp->side = p->side; gp->fork_ev = p->jev[0]; gp->join_ev = p->jev[1]; gp->d_verdict = p->ctrl + 8;
    *adopted = plan_adopt(p, A, gp->g);
    if (p->verdict_clean) p->verdict_clean = false;
    else if (!(*adopted && gp->how == GridProof::FACTOR_LAUNCH)) ILUPP_HIP(hipMemsetAsync(gp->d_verdict, 0, sizeof(int32_t), p->stream));
    if (gp->how == GridProof::SIDE_STREAM) gp->queue(p->stream, A);
    if (!*adopted) grid_schedules(p->stream, A, gp->g, &p->Lc, &p->Uc, &p->sA, &p->sU, &p->max_row_len, max_wgs);
    return true;
}
// one pass over A's pattern: row counts of L and U, diagonal check, and the factor-sweep schedules (L shares A's
// forward cuts and U its backward cuts: same strictly-lower / strictly-upper patterns)
static int general_symbolic(ilupp_precond *p, const DevMat &A, int max_wgs)
{
    int32_t missing = -1;
    const int rc = ilu0_symbolic_and_schedule(p->stream, A, &p->Lc, &p->Uc, &missing, p->max_lanes, &p->sA, &p->sU, &p->max_row_len);
    if (rc == ILUPP_ERR_NO_DIAGONAL) set_error("ILU0: structurally missing diagonal entry in row " + std::to_string(missing));
    if (rc) return rc;
    choose_tiling_pair(p->stream, A.ptr, A.idx, &p->sA, &p->sU, max_wgs);
    finish_chains(&p->sA, &p->sU);             // (the read-back ilu0_symbolic_and_schedule queued came with the tiling's wait)
    return ILUPP_OK;
}
// nothing built on a grid guess survives it (forget: nor the shape remembered for this index array); the general pass decides
static void drop_grid_guess(ilupp_precond *p, const GridProof &gp, const char *why, const DevMat *forget)
{
    if (getenv("ILUPP_DEBUG")) fprintf(stderr, "[ilupp] grid guess %d x %d x %d dropped (%s)\n", gp.g.nx, gp.g.ny, gp.g.nz, why);
    p->pkL.release(); p->pkU.release(); p->flm.release();
    p->sA.release(); p->sU.release();
    p->sA = Schedule(); p->sU = Schedule();
    p->grid_path = false; p->plan_ok = false;
    if (forget) grid_shape_forget(forget->n, forget->nnz, forget->idx);
}

// CSR patterns of L and U (ILU0.hpp:85-98).  The level-major kernels never read them (they are for factors() and the
// generic transposed solves).  (Running this pass on a side stream next to the factor kernel cost the kernel more --
// 2.0 -> 2.5 ms -- than the pass takes, 0.28 ms.)  Static form: nothing here; row pointers, column indices and values all
// come out of the records when somebody asks (ensure_csr_values).  lm: the static form took the matrix.
static int csr_and_level_fallbacks(ilupp_precond *p, const DevMat &A, bool lm, bool *have_prog)
{
    hipStream_t st = p->stream;
    if (!p->flm.stat) {
        const int rc = ilu0_csr_ptrs(st, A, &p->Lc, &p->Uc);
        if (rc) return rc;
        ilu0_write_patterns(st, A, &p->Lc, &p->Uc);
    }
    if (!lm) ilu0_unit_diagonal(st, &p->Lc);        // the CSR-streaming factor kernels write the eliminations only
    // rows too long for the level-major forms (9-point, 27-point stencils ...): one wave per row, rows in level order (ilu0_lvl.hip);
    // the sweeps of such factors are the level-ordered ones as well (sptrsv_lvl.hip), nothing below is needed
    // ... and SHORT rows that the static form did not take (a mesh with holes, lines of irregular length): in natural order the
    // CSR-streaming kernels and the generic sweeps run such a matrix's chains one row after the other behind a window of resident rows
    // (the 256^3 mesh with 3 % of its points removed: 111 s, and the sweeps ran into their time limit) -- by level it is hundreds of wide
    // levels.  A matrix whose levels are few and wide anyway (the same mesh randomly permuted: about 30) stays on the streaming kernels.
    static const bool lvl_never = getenv("ILUPP_NO_LVL_SHORT") != nullptr;
    bool by_level = false;
    if (!lm && p->max_row_len <= 64 && A.n >= 1024) {
        const bool longrows = A.nnz > 8 * (int64_t)A.n;
        if ((longrows || !lvl_never) && lvl_order(st, 2, A.n, A.nnz, A.ptr, A.idx, p->sA, &p->fperm, &p->fperm_levels, &p->fperm_how)) {
            // (deep AND wide: a 1-D chain has n levels of one row -- nothing to run side by side, natural order is as good as any)
            by_level = longrows || (p->fperm_levels > 64 && A.n / p->fperm_levels >= 256);
            if (!by_level) { (void)pool_free(p->fperm); p->fperm = nullptr; p->fperm_levels = 0; }
        }
    }
    if (p->compact && !lm && !by_level) {
        // not a short-row matrix (or an irregular one): descriptors, update program and the CSR-streaming kernels
        if (!(A.nnz >= 16 && build_ilu0_program_f3(st, A, p->Uc, p->sA, &p->prog_f3)))
            *have_prog = build_ilu0_program(st, A, p->Uc, p->sA, &p->prog);
        make_desc(st, p->Lc, p->sA, &p->dL);
        make_desc(st, p->Uc, p->sU, &p->dU);
        // the sweeps may still have a level-major form (records from the descriptors, values by a pass after the factor kernel)
        if (lm_prepare(st, SWEEP_FWD_LAST_ASC, p->Lc, p->sA, p->dL, p->max_row_len, &p->pkL) &&
            lm_prepare(st, SWEEP_BWD_FIRST_ASC, p->Uc, p->sU, p->dU, p->max_row_len, &p->pkU)) {
            lm_pack(st, SWEEP_FWD_LAST_ASC, p->Lc, p->sA, p->dL, &p->pkL, 1);
            lm_pack(st, SWEEP_BWD_FIRST_ASC, p->Uc, p->sU, p->dU, &p->pkU, 1);
            lm_finish(st, &p->pkL);
            lm_finish(st, &p->pkU);
        }
        if (!(p->pkL.valid && p->pkU.valid)) { p->pkL.release(); p->pkU.release(); }
    }
    return ILUPP_OK;
}

// The verdict on a grid attempt: 0 = proven, 1 = the pattern differs, 2 = a size was mispredicted.  The factor kernel's own read-back took the verdict word along, or it is
// read here, behind the proof (queued now if the factor kernel that ran was not the one that proves).  waited: for that read-back, already; else for the stream, here.
static int32_t grid_verdict(ilupp_precond *p, const DevMat &A, GridProof *gp, bool waited)
{
    int32_t bad = gp->verdict;
    if (bad < 0) {
        gp->settle(p->stream, A);
        ILUPP_HIP(d2h_async(p->stream, &bad, gp->d_verdict, sizeof(int32_t)));
    }
    if (!waited) ILUPP_HIP(stream_sync(p->stream));
    const FactorLM &f = p->flm;
    if (!f.spec || bad != 0) return bad;
    // the sizes the lane-table kernels were launched with were predicted (st.hip: st_analyse_ilu0); what the device found is here now
    bool same = f.chk_hl[0] == 0 && f.chk_hu[0] == 0 && f.chk_hu[3] == 0 && f.chk_hl[8] == 0 && f.chk_hl[9] == 0 && f.chk_hu[9] == 0 && f.chk_hl[10] == 0;
    same = same && f.chk_hl[1] == f.pred[0] && f.chk_hu[1] == f.pred[0] && f.chk_hl[2] == f.pred[1] && f.chk_hu[2] == f.pred[1];
    same = same && f.chk_xtot[0] == f.pred[2] && f.chk_xtot[2] == f.pred[2] && f.chk_xtot[1] == f.pred[3] && f.chk_xtot[3] == f.pred[3];
    if (!same && getenv("ILUPP_DEBUG"))
        fprintf(stderr, "[ilupp] grid %d x %d x %d: predicted sizes %d %d %d %d, found %d/%d %d/%d %d/%d %d/%d, flags %d %d %d %d %d %d %d: redone\n", gp->g.nx, gp->g.ny, gp->g.nz,
                f.pred[0], f.pred[1], f.pred[2], f.pred[3], f.chk_hl[1], f.chk_hu[1], f.chk_hl[2], f.chk_hu[2], f.chk_xtot[0], f.chk_xtot[2], f.chk_xtot[1], f.chk_xtot[3],
                f.chk_hl[0], f.chk_hu[0], f.chk_hu[3], f.chk_hl[8], f.chk_hl[9], f.chk_hu[9], f.chk_hl[10]);
    return same ? 0 : 2;
}

// The two phases' times; the numeric phase ends at `end`.  kernel_events (a grid whose factor kernel is the wave-exchange one): the proof ends in front of the factor
// kernel, behind the launches that clear its control words, so the analysis phase lasts until the event in front of that kernel, ev[4], not until ev[1].
static void factor_timing(ilupp_precond *p, bool kernel_events, hipEvent_t end, float kms)
{
    hipEvent_t mid = kernel_events ? p->ev[4] : p->ev[1];
    ILUPP_HIP(hipEventElapsedTime(&p->tm.analysis_ms, p->ev[0], mid));
    ILUPP_HIP(hipEventElapsedTime(&p->tm.numeric_ms, mid, end));
    p->tm.numeric_kernel_ms = kms;
}

// ILU(0) of the row-major view held in A (device).  Fills p->Lc/Uc, schedules and timings.
int ilu0_factor(ilupp_precond *p, const DevMat &A, const int32_t *head)
{
    hipStream_t st = p->stream;
    p->nnzA = A.nnz;
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    const int max_wgs = p->max_lanes / kThreads;
    GridProof gp;
    bool adopted = false;
    bool grid = grid_attempt_begin(p, A, head, &gp, max_wgs, &adopted), lm = false;
    for (;;) {
        // (a parked plan of this shape: the three steps below ran for the object that left it)
        if (adopted) { lm = true; break; }
        if (!grid) { const int rc = general_symbolic(p, A, max_wgs); if (rc) return rc; }
        // (a grid's slot tables are filled together with its lane templates: grid.hip, k_grid_lanes; ILUPP_GRID_TABLES=0: by the general kernels)
        static const bool grid_tables = []() { const char *e = getenv("ILUPP_GRID_TABLES"); return !(e && atoi(e) == 0); }();
        build_slot_tables(st, &p->sA, true, !(grid && grid_tables));
        build_slot_tables(st, &p->sU, false, !(grid && grid_tables));
        p->compact = schedule_is_compact(p->sA) && schedule_is_compact(p->sU);
        // static form first (lane tables, values-only records: st.hip; no descriptor words, hence no limit on block size or number
        // of slots), then the record-decoding level-major form
        lm = st_analyse_ilu0(st, A, p->sA, p->sU, &p->pkL, &p->pkU, &p->flm, (grid && grid_tables) ? &gp.g : nullptr);
        if (!grid || (lm && p->flm.stat && p->flm.direct)) break;
        // a grid the static direct-feed form does not take (or not the guessed grid: the lane templates of sampled rows disagree)
        ILUPP_HIP(hipStreamSynchronize(p->side));
        if (p->no_general_retry) return ILUPP_ERR_UNSUPPORTED;
        drop_grid_guess(p, gp, "static analysis declined", nullptr);
        gp = GridProof();
        grid = false;
    }
    p->grid_path = grid;
    bool have_prog = false;
    int rc = csr_and_level_fallbacks(p, A, lm, &have_prog);
    if (rc) return rc;
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    float kms = 0.f;
    // (the factor kernel's own read-back waits for the proof and takes its verdict along: no round trip of its own)
    const bool wx_numeric = p->flm.built && p->flm.stat && ilu0_numeric_st_is_wx(p->pkL, p->flm);
    // (the factor kernel waits for the proof -- it lives on short hand-over latencies and loses more next to the proof's 4.6 TB/s
    // stream than the wait costs --, but what is queued in front of it, the clearing of its control words and exchange, does not;
    // with the lane tables in closed form the proof is what the analysis phase lasts)
    // (... unless that kernel proves the pattern itself, behind its tiles: then it waits for nothing, and the analysis phase is the table chain)
    if (grid && !wx_numeric) gp.settle(st, A);      // (another factor kernel runs: the proof in front of it, here and now if the factor launch was to hold it)
    // (... and queues the arming of the first apply behind that read-back; the speculation's leftovers -- pending read-backs of the lane
    // tables' flags -- lie in front of it too)
    if (wx_numeric && p->jev[0]) { gp.arm = [](void *c) { arm_apply(static_cast<ilupp_precond *>(c)); }; gp.arm_ctx = p; gp.arm_ev = p->jev[0]; }
    rc = ilu0_numeric_any(p, A, have_prog, &kms, &gp);
    // (the wave-exchange factor kernel's own read-back has been waited for -- through an event, so that what it queued behind it, the
    // arming of the first apply, runs on: no wait for the whole stream here then; ev[5] was recorded behind that kernel)
    const bool waited = wx_numeric && gp.verdict >= 0;
    if (!waited) ILUPP_HIP(hipEventRecord(p->ev[2], st));
    const int32_t grid_bad = grid ? grid_verdict(p, A, &gp, waited) : 0;
    if (!grid && !waited) ILUPP_HIP(stream_sync(st));
    if (grid_bad != 0) {
        // the matrix only began like a grid (or a size was mispredicted): the general pass runs
        drop_grid_guess(p, gp, grid_bad == 2 ? "sizes mispredicted" : "pattern differs", &A);
        if (adopted) plans().note_dropped();       // (the tables went to the pool with the guess: the plan is gone, not parked again)
        if (p->no_general_retry) return ILUPP_ERR_UNSUPPORTED;
        return ilu0_factor(p, A, nullptr);
    }
    if (grid && rc == ILUPP_OK) grid_shape_remember(A.n, A.nnz, gp.g, A.idx);
    // (what destroy_obj may park: plan_parkable)
    if (grid && wx_numeric && rc == ILUPP_OK) { p->grid_gd = gp.g; p->plan_ok = true; p->apply_open = false; }
    factor_timing(p, grid && wx_numeric && rc == ILUPP_OK, waited ? p->ev[5] : p->ev[2], kms);
    if (rc == ILUPP_ERR_TIMEOUT) set_error("ILU0: dependency wait timed out (invalid structure?)");
    if (rc == ILUPP_OK) settle_ctrl(p);
    return rc;
}

// the CSR value arrays of the factors, when the level-major factor kernel left them unwritten
void ensure_csr_values(ilupp_precond *p)
{
    if (p->csr_vals) return;
    // (an object its plan can still be parked from -- plan_parkable -- stays one: what follows rewrites records and makes CSR arrays of the
    // object's own, and reads the tables)
    if (p->pkL.stat) {
        // (the passes below read records by template position: st_wave.hip's class-aligned ones are turned back for them)
        const int fmt = p->pkL.fmt;
        wx_convert_records(p->stream, &p->pkL, &p->pkU, 0);
        if (!p->Lc.ptr) (void)st_make_csr(p->stream, p->n, p->pkL, p->pkU, &p->Lc, &p->Uc);      // (throws on a HIP error)
        st_unpack(p->stream, p->Lc, p->pkL);
        st_unpack(p->stream, p->Uc, p->pkU);
        wx_convert_records(p->stream, &p->pkL, &p->pkU, fmt);
    }
    ILUPP_HIP(stream_sync(p->stream));
    p->csr_vals = true;
}

void ensure_transposed(ilupp_precond *p)
{
    if (p->haveT) return;
    ensure_csr_values(p);
    hipStream_t st = p->stream;
    if (p->kind == KIND_LU) {
        transpose_storage(st, p->Uc, &p->UcT);      // lower, diagonal last
        transpose_storage(st, p->Lc, &p->LcT);      // upper, diagonal first
        sweep_tables(st, p, {&p->UcT, true, &p->sUT, &p->dUT}, {&p->LcT, false, &p->sLT, &p->dLT}, true, &p->max_len_T);
    } else if (p->kind == KIND_UTU) {
        // both transposes are row-major lower matrices with the diagonal last: forward sweeps
        transpose_storage(st, p->Lc, &p->LcT);
        transpose_storage(st, p->Uc, &p->UcT);
        sweep_tables(st, p, {&p->LcT, true, &p->sLT, &p->dLT}, {&p->UcT, true, &p->sUT, &p->dUT}, false, &p->max_len_T);
    } else {
        transpose_storage(st, p->Lc, &p->LcT, (p->icholt_grid && !p->llt_diag_last && p->llt_gd.nx > 0) ? &p->llt_gd : nullptr);
        if (min_row_len(st, p->n, p->LcT.ptr, p->LcT.idx, p->llt_diag_last ? 1 : 2) == 0) p->degenerate = true;
        // Lc row-major lower (IChol0): LcT is upper with the diagonal first -> backward sweep;
        // Lc column-major lower (ICholT): LcT is its row-major form with the diagonal last -> forward sweep
        sweep_tables(st, p, {&p->LcT, !p->llt_diag_last, &p->sLT, &p->dLT}, {}, true, &p->max_len_T);
    }
    p->haveT = true;
}

// What the single sweeps of a batch-built ILU(0) object need -- cuts and schedules, tilings, slot tables, descriptors --, on first use and
// from the factors' own patterns: L forward, U backward, as an ILUT object gets its own (ilut_create_common).  max_row_len stays A's
// longest row (no row of L or U is longer): it is what the batched re-factorisation routes by.  A batch-built ILUT object
// (ilupp_hip_ilut_create_batch*) takes the same branch: its max_row_len is the longest row of L or U already, what sweep_tables finds.
void ensure_sweep_tables(ilupp_precond *p)
{
    if (!p->batch_built || p->sweeps_ready) return;
    int32_t longest = 0;
    // (a batch-built IChol(0) object: L forward, as ichol0_create_common builds it; the backward sweep's tables come with LcT)
    if (p->kind == KIND_LLT) p->compact = sweep_tables(p->stream, p, {&p->Lc, true, &p->sL, &p->dL}, {}, true, &longest);
    else p->compact = sweep_tables(p->stream, p, {&p->Lc, true, &p->sL, &p->dL}, {&p->Uc, false, &p->sU, &p->dU}, true, &longest);
    p->sweeps_ready = true;
}

// ---- the sweeps of an apply -----------------------------------------------------------------------------------------------------------
// One sweep of one object: the stored triangle it walks (slot 0 = Lc, 1 = Uc, 2 = UcT, 3 = LcT: the numbering of pack_tried[] and lvl[])
// and the manner.  Whatever else a sweep needs follows from the slot: sweep_parts.
struct SweepOp { int slot; SweepKind kind; };
struct SweepParts {
    const DevMat &M; const Schedule &sch; const int32_t *desc; int32_t maxlen;      // the triangle, its schedule, descriptors, longest major slice
    PackedSweep *pk; bool *pack_tried;                                               // its level-major or static records
    LevelSweep *lvl;                                                                 // its renumbered copy in level order
};
static SweepParts sweep_parts(ilupp_precond *p, SweepOp op)
{
    switch (op.slot) {
    // (an LU object's L has A's strictly-lower pattern, hence A's forward cuts: the factor-sweep schedule serves it)
    case 0: return {p->Lc, (p->kind == KIND_LU && !p->sL.start) ? p->sA : p->sL, p->dL, p->max_row_len, &p->pkL, &p->pack_tried[0], &p->lvl[0]};
    case 1: return {p->Uc, p->sU, p->dU, p->max_row_len, &p->pkU, &p->pack_tried[1], &p->lvl[1]};
    case 2: return {p->UcT, p->sUT, p->dUT, p->max_len_T, &p->pkUT, &p->pack_tried[2], &p->lvl[2]};
    default: return {p->LcT, p->sLT, p->dLT, p->max_len_T, &p->pkLT, &p->pack_tried[3], &p->lvl[3]};
    }
}

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
static ApplyPlan apply_plan(int kind, bool transpose, bool input_csc, bool llt_diag_last)
{
    const SweepKind fwd = SWEEP_FWD_LAST_ASC, bwd = SWEEP_BWD_FIRST_ASC, bwd_desc = SWEEP_BWD_FIRST_DESC;
    if (kind == KIND_LU) {
        // solve with M (= A for CSR input): fwd(Lc) then bwd(Uc)           [CSR/ID, CSC/TRANSPOSE]
        // solve with M^T:                   fwd(Uc^T) then bwd_desc(Lc^T)  [CSR/TRANSPOSE, CSC/ID]
        if (transpose == input_csc) return {{0, fwd}, {1, bwd}, true};
        return {{2, fwd}, {3, bwd_desc}, false};
    }
    if (kind == KIND_UTU) {
        // ILUC (preconditioner_implementation.h:940-958 + :103-111): the left factor is stored column-wise, the right one row-wise,
        // i.e. both array triples read as upper CSR matrices with the diagonal first (F1 = left^T in Lc, F2 = right in Uc).
        //   ID:        T2(left)    = forward sweep over F1^T, then T3(right)  = backward sweep over F2
        //   TRANSPOSE: T2(right^T) = forward sweep over F2^T, then T3(left^T) = backward sweep over F1
        if (!transpose) return {{3, fwd}, {1, bwd}, false};
        return {{2, fwd}, {0, bwd}, false};
    }
    // LL^T: apply == apply_trans (preconditioner_implementation.h:381-394)
    if (llt_diag_last) return {{0, fwd}, {3, bwd_desc}, false};      // IChol0 (Lc row-major): T1(L) then T4(L)
    return {{3, fwd}, {0, bwd}, false};                               // ICholT (Lc column-major): T2(L) then T3(L)
}
static ApplyPlan apply_plan(const ilupp_precond *p, int transpose) { return apply_plan(p->kind, transpose != 0, p->input_csc, p->llt_diag_last); }

// one sweep: the packed kernel when the factor has a verified level-major form, else the CSR kernels.  Either way
// the right-hand side buffer is all-sentinel afterwards (the CSR kernels reset it row by row).
// level-major records of a sweep straight from its CSR arrays and descriptors (any object whose rows are short enough:
// transposed ILU(0) factors, IChol(0)); tried once, on first use
static const PackedSweep *packed(ilupp_precond *p, SweepOp op)
{
    const SweepParts s = sweep_parts(p, op);
    if (!s.pk->valid && !*s.pack_tried && s.desc && !p->degenerate) {
        if (lm_prepare(p->stream, op.kind, s.M, s.sch, s.desc, s.maxlen, s.pk)) {
            lm_pack(p->stream, op.kind, s.M, s.sch, s.desc, s.pk, 3);
            lm_finish(p->stream, s.pk);
        }
    }
    *s.pack_tried = true;
    return s.pk->valid ? s.pk : nullptr;
}

// Rows too long for the level-major records (ILUT factors, ICholT with fill, ILU(0) of a long-row matrix) sweep one lane per row, in
// level order when the factor has one (sptrsv_lvl.hip; renumbered copy of the factor, built at the first sweep and shared by the single
// and the block apply: one level order per factor).  nullptr: the sweep is another kernel (the caller tells which).
static bool long_rows(ilupp_precond *p, SweepOp op)
{
    const DevMat &M = sweep_parts(p, op).M;
    return (M.nnz > 4 * (int64_t)M.n || (p->kind == KIND_LU && p->fperm != nullptr)) && M.n >= 1024;
}
static LevelSweep *level_sweep(ilupp_precond *p, SweepOp op)
{
    const SweepParts s = sweep_parts(p, op);
    if (!s.lvl->tried) {
        if (op.slot < 2) ensure_csr_values(p);
        const bool reuse = op.slot == 0 && p->fperm && op.kind == SWEEP_FWD_LAST_ASC;      // L's rows depend on each other as A's lower part does
        lvl_build(p->stream, op.kind, s.M, s.sch, s.lvl, reuse ? p->fperm : nullptr, reuse ? p->fperm_levels : 0);
    }
    return s.lvl->valid ? s.lvl : nullptr;
}

// the kernel family a sweep ran on, kept per slot in last_route[] (diagnostics: ilupp_hip_debug_level_order's info[6])
enum SweepRoute { SWEPT_NEVER = 0, SWEPT_STATIC = 1, SWEPT_LEVEL_MAJOR = 2, SWEPT_LEVEL_ORDER = 3, SWEPT_ROWS = 4, SWEPT_ROWS_DEGENERATE = 5,
                  SWEPT_DESCRIPTORS = 6, SWEPT_GENERIC = 7 };

static int sweep(ilupp_precond *p, SweepOp op, const PackedSweep *ps, double *rhs, double *out, int32_t *ticket, int32_t *err,
                 double *ypk_out = nullptr, const double *ypk_in = nullptr, const int32_t *ysrc = nullptr)
{
    const SweepParts s = sweep_parts(p, op);
    int8_t &route = p->last_route[op.slot];
    p->last_desc_kernel[op.slot] = 0;
    // every sweep but the static ones hands its unknowns over through `out` (the data is the flag): all-sentinel before it runs.
    // The static sweeps never touch the work vector, so an object that only ever runs them never pays for the fill.
    if (!(ps && ps->valid && ps->stat && !p->degenerate) && !p->work_clean) {
        fill_u64(p->stream, reinterpret_cast<unsigned long long *>(p->work), p->n, kSentinel);
        p->work_clean = true;
    }
    if (p->degenerate) { route = SWEPT_ROWS_DEGENERATE; return sptrsv_rows(p->stream, op.kind, s.M, rhs, out, ticket, err); }
    if (ps && ps->valid) {
        // (the static sweeps exchange through a buffer of their own: `out` needs no sentinels before and `rhs` none after)
        route = ps->stat ? SWEPT_STATIC : SWEPT_LEVEL_MAJOR;
        if (ps->stat) return sptrsv_st(p->stream, *ps, p->n, rhs, out, ticket, err, ypk_out, ypk_in, ysrc);
        OR_RETURN(sptrsv_lm(p->stream, *ps, s.sch, p->n, rhs, out, ticket, err, ypk_out, ypk_in, ysrc));
        fill_u64(p->stream, reinterpret_cast<unsigned long long *>(rhs), p->n, kSentinel);
        return ILUPP_OK;
    }
    // Rows too long for the level-major records (ILUT factors, ICholT with fill): one lane per ROW instead of one lane per
    // block of consecutive rows.  With blocks, a row waits for everything its lane has to do before it, and the factors of
    // a random matrix have no chains that would make blocks pay: BASELINE config C3's apply took 70 + 186 ms, more than the
    // reference needs on one core.
    if (long_rows(p, op)) {
        // ... and the rows in level order: in natural order only the rows inside the window of resident tickets can run, on a mesh a
        // few grid lines
        const LevelSweep *ls = level_sweep(p, op);
        route = ls ? SWEPT_LEVEL_ORDER : SWEPT_ROWS;
        if (ls) return sptrsv_lvl(p->stream, *ls, rhs, out, ticket, err);
        return sptrsv_rows(p->stream, op.kind, s.M, rhs, out, ticket, err);
    }
    route = s.desc ? SWEPT_DESCRIPTORS : SWEPT_GENERIC;
    return sptrsv(p->stream, op.kind, s.M, s.sch, s.desc, s.maxlen, rhs, out, ticket, err, &p->last_desc_kernel[op.slot]);
}
// static form: records of U^T and L^T exist (built on first use; a pattern they cannot express is remembered)
static bool static_transposed_ready(ilupp_precond *p)
{
    if (!(p->flm.stat && p->pkL.stat && p->pkU.stat) || p->no_static_T) return false;
    if (p->pkL.pkT && p->pkU.pkT) return true;
    const int fmt = p->pkL.fmt;
    wx_convert_records(p->stream, &p->pkL, &p->pkU, 0);
    const bool ok = st_build_transposed(p->stream, p->sA, p->n, p->flm, &p->pkL, &p->pkU, p->Lc.nnz - p->n, p->Uc.nnz - p->n);
    wx_convert_records(p->stream, &p->pkL, &p->pkU, fmt);
    // (an object whose own sweeps are the wave-exchange ones gets them for the transposed apply as well)
    if (ok && fmt >= 1) wx_convert_transposed(p->stream, &p->pkL, &p->pkU);
    if (ok) return true;
    p->no_static_T = true;
    return false;
}

// LL^T objects whose factor is stencil-like (IChol0, ICholT without fill on a mesh): the static sweep kernels on the factor's own values,
// analysed on first use.  The pair (forward, backward) when it exists.
static bool llt_static_pair(ilupp_precond *p, PackedSweep **pf_out, PackedSweep **pb_out)
{
    const bool dl = p->llt_diag_last;
    PackedSweep *pf = dl ? &p->pkL : &p->pkLT, *pb = dl ? &p->pkLT : &p->pkL;
    if (!p->pair_tried && !p->degenerate) {
        p->pair_tried = true;
        // IChol0: forward over L (row-major, diagonal last), backward over its transposed copy in DESCENDING column order (T4);
        // ICholT: forward over the row-major copy of L, backward over L's own column-major arrays (T3)
        const bool ok = dl ? st_analyse_pair(p->stream, p->n, p->Lc, p->LcT, p->sL, p->sLT, pf, pb, true)
                           : st_analyse_pair(p->stream, p->n, p->LcT, p->Lc, p->sLT, p->sL, pf, pb, false);
        if (ok) p->pack_tried[0] = p->pack_tried[3] = true;
    }
    *pf_out = pf; *pb_out = pb;
    return pf->valid && pf->pair && pb->valid && pb->pair;
}

// What an apply does before its sweeps, whichever route runs them then: the transposed storages when `plan` reads one, and the two static
// forms that take the place of the plan's sweeps -- LU's transposed records (ROUTE_STATIC_T) and the LL^T pair (ROUTE_STATIC_PAIR: *pf, *pb).
enum ApplyRoute { ROUTE_SWEEPS, ROUTE_STATIC_T, ROUTE_STATIC_PAIR };
static ApplyRoute prepare_apply(ilupp_precond *p, const ApplyPlan &plan, PackedSweep **pf, PackedSweep **pb)
{
    ensure_sweep_tables(p);                          // (a batch-built ILU(0) object's first single sweep)
    if (!plan.transposed()) return ROUTE_SWEEPS;
    p->plan_ok = false;                  // (transposed records or storages are made)
    if (p->kind == KIND_LU) {
        p->pkL.xch_armed = p->pkU.xch_armed = false;
        if (static_transposed_ready(p)) return ROUTE_STATIC_T;
    }
    ensure_transposed(p);
    if (p->kind == KIND_LLT && llt_static_pair(p, pf, pb)) return ROUTE_STATIC_PAIR;
    return ROUTE_SWEEPS;
}

}  // namespace

namespace ilupp {

// apply on a device vector; `transpose` as in apply_preconditioner_only(use, y)
int apply_dev(ilupp_precond *p, double *x, int transpose)
{
    hipStream_t st = p->stream;
    p->apply_open = true;                                // (until a finish_apply has waited for it and found no error)
    order_after_caller(st, p->sev[0]);
    if (p->ctrl_armed) p->ctrl_armed = false;            // (zero already: arm_apply)
    else ILUPP_HIP(hipMemsetAsync(p->ctrl, 0, 64, st));
    int32_t *err = p->ctrl, *t1 = p->ctrl + 4, *t2 = p->ctrl + 5;
    double *y = p->work;
    p->block_events = false;
    const ApplyPlan plan = apply_plan(p, transpose);
    PackedSweep *pf = nullptr, *pb = nullptr;
    const ApplyRoute route = prepare_apply(p, plan, &pf, &pb);
    if (route == ROUTE_STATIC_T) {
        // static form: the same two sweep kernels on records of U^T and L^T
        p->last_route[plan.first.slot] = p->last_route[plan.second.slot] = SWEPT_STATIC;
        p->last_desc_kernel[plan.first.slot] = p->last_desc_kernel[plan.second.slot] = 0;
        ILUPP_HIP(hipEventRecord(p->ev[0], st));
        OR_RETURN(sptrsv_st_T(st, p->pkL, p->n, x, y, t1, err, p->pkL.ybuf, nullptr));
        ILUPP_HIP(hipEventRecord(p->ev[1], st));
        OR_RETURN(sptrsv_st_T(st, p->pkU, p->n, y, x, t2, err, p->pkL.ybuf, p->pkU.ysrc));
    } else if (route == ROUTE_STATIC_PAIR) {
        // stencil-like factors (IChol0, ICholT without fill on a mesh): the static sweep kernels on the factor's own values
        p->last_route[plan.first.slot] = p->last_route[plan.second.slot] = SWEPT_STATIC;
        p->last_desc_kernel[plan.first.slot] = p->last_desc_kernel[plan.second.slot] = 0;
        ILUPP_HIP(hipEventRecord(p->ev[0], st));
        OR_RETURN(sptrsv_st(st, *pf, p->n, x, y, t1, err, pf->ybuf, nullptr, nullptr));
        ILUPP_HIP(hipEventRecord(p->ev[1], st));
        OR_RETURN(sptrsv_st(st, *pb, p->n, y, x, t2, err, nullptr, pf->ybuf, pb->ysrc));
    } else {
        const PackedSweep *pk1 = sweep_parts(p, plan.first).pk, *pk2 = sweep_parts(p, plan.second).pk;
        const bool ylm = plan.ylm && p->flm.built && pk1->valid && pk2->valid && pk1->ybuf && pk2->ysrc;
        const PackedSweep *p1 = packed(p, plan.first);
        const PackedSweep *p2 = packed(p, plan.second);
        ILUPP_HIP(hipEventRecord(p->ev[0], st));
        OR_RETURN(sweep(p, plan.first, p1, x, y, t1, err, ylm ? pk1->ybuf : nullptr));
        ILUPP_HIP(hipEventRecord(p->ev[1], st));
        OR_RETURN(sweep(p, plan.second, p2, y, x, t2, err, nullptr, ylm ? pk1->ybuf : nullptr, ylm ? pk2->ysrc : nullptr));
    }
    ILUPP_HIP(hipEventRecord(p->ev[2], st));
    p->apply_events_valid = true;
    return ILUPP_OK;
}

int finish_apply(ilupp_precond *p)
{
    int32_t err = 0;
    ILUPP_HIP(d2h_async(p->stream, &err, p->ctrl, sizeof(int32_t)));
    bool armed_here = false;
    if (p->jev[0] && !p->borrowed_queue) {
        // (the next apply is armed behind this read-back and in front of the wait for it)
        ILUPP_HIP(hipEventRecord(p->jev[0], p->stream));
        arm_apply(p);
        armed_here = true;
        ILUPP_HIP(event_sync(p->stream, p->jev[0]));
    } else {
        ILUPP_HIP(stream_sync(p->stream));
    }
    if (p->apply_events_valid) {
        ILUPP_HIP(hipEventElapsedTime(&p->tm.lsolve_kernel_ms, p->ev[0], p->ev[1]));
        ILUPP_HIP(hipEventElapsedTime(&p->tm.usolve_kernel_ms, p->ev[1], p->ev[2]));
        ILUPP_HIP(hipEventElapsedTime(&p->tm.last_apply_ms, p->block_events ? p->ev[3] : p->ev[0], p->ev[2]));
    }
    if (err) {
        // a sweep gave up: restore the all-sentinel invariant of the work vector
        fill_u64(p->stream, reinterpret_cast<unsigned long long *>(p->work), p->n, kSentinel);
        ILUPP_HIP(stream_sync(p->stream));
        set_error("triangular solve: dependency wait timed out (factor not triangular?)");
        return ILUPP_ERR_TIMEOUT;
    }
    if (!armed_here) arm_apply(p);
    p->apply_open = false;
    return ILUPP_OK;
}

}  // namespace ilupp

namespace {

// ---- block apply: k right-hand sides, X row-major n x k, in place; every column as apply_dev gives it -----------------------------
// Two routes.  "block:level": both sweeps of the apply are the level-order kernel (sptrsv_lvl.hip) -- the same records walked once per
// chunk of up to kSptrsmMaxKB columns (sptrsm_lvl.hip).  "block:columns": every other object (the static and packed sweeps of box grids,
// factors the level order declines, degenerate ones, n < 1024) and k = 1: each column gathered into a vector, apply_dev, scattered back.
__global__ void k_col_gather(const double *__restrict__ X, int64_t ld, int32_t n, double *__restrict__ col)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) col[i] = X[i * ld];
}
__global__ void k_col_scatter(const double *__restrict__ col, double *__restrict__ X, int64_t ld, int32_t n, const int32_t *__restrict__ err,
                              int32_t *__restrict__ seen)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && *err) *seen = 1;              // (the next column's apply clears the control words)
    if (i < n) X[i * ld] = col[i];
}

// the two sweeps of an apply when both run on the level-order kernel (apply_dev's plan, the same caches)
static bool block_level_plan(ilupp_precond *p, int transpose, LevelSweep **first, LevelSweep **second)
{
    *first = *second = nullptr;
    if (p->degenerate) return false;
    const ApplyPlan plan = apply_plan(p, transpose);
    PackedSweep *pf = nullptr, *pb = nullptr;
    if (prepare_apply(p, plan, &pf, &pb) != ROUTE_SWEEPS) return false;
    auto lvl = [p](SweepOp op) -> LevelSweep * {
        if (packed(p, op)) return nullptr;      // level-major or static records
        return long_rows(p, op) ? level_sweep(p, op) : nullptr;
    };
    *first = lvl(plan.first);
    *second = lvl(plan.second);
    if (!(*first && *second) || p->degenerate) return false;
    // (the caller's chunks are level-order sweeps over these two slots, and they do not pass through sweep())
    p->last_route[plan.first.slot] = p->last_route[plan.second.slot] = SWEPT_LEVEL_ORDER;
    p->last_desc_kernel[plan.first.slot] = p->last_desc_kernel[plan.second.slot] = 0;
    return true;
}

static int chunk_width(int64_t left) { return left >= kSptrsmMaxKB ? kSptrsmMaxKB : left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1; }

// the block buffers for chunks of kb columns and `words` control words (grown only; an earlier asynchronous block apply may still use the
// old ones, and the pool knows nothing of streams)
static void block_buffers(ilupp_precond *p, int kb, int64_t words)
{
    if (kb <= p->bkb && words <= p->btk_cap) return;
    ILUPP_HIP(stream_sync(p->stream));
    if (kb > p->bkb) {
        for (double **q : {&p->bxp, &p->by}) { if (*q) (void)pool_free(*q); *q = nullptr; }
        p->bkb = 0;
        ILUPP_HIP(pool_malloc(&p->bxp, sizeof(double) * (size_t)p->n * (size_t)kb));
        ILUPP_HIP(pool_malloc(&p->by, sizeof(double) * (size_t)p->n * (size_t)kb));
        p->bkb = kb;
    }
    if (words > p->btk_cap) {
        if (p->btk) (void)pool_free(p->btk);
        p->btk = nullptr; p->btk_cap = 0;
        ILUPP_HIP(pool_malloc(&p->btk, sizeof(int32_t) * (size_t)words));
        p->btk_cap = words;
    }
}

int apply_block_dev(ilupp_precond *p, double *X, int64_t k, int transpose)
{
    hipStream_t st = p->stream;
    const int32_t n = p->n;
    order_after_caller(st, p->sev[0]);
    LevelSweep *l1 = nullptr, *l2 = nullptr;
    const bool level = k > 1 && block_level_plan(p, transpose, &l1, &l2);
    p->block_path = level ? "block:level" : "block:columns";
    if (!level && k == 1) {                              // (one column of a row-major block is a contiguous vector)
        ILUPP_HIP(hipEventRecord(p->ev[3], st));
        const int rc = apply_dev(p, X, transpose);
        p->block_events = true;
        return rc;
    }
    if (!level) {
        if (!p->bcol) ILUPP_HIP(pool_malloc(&p->bcol, sizeof(double) * (size_t)n));
        block_buffers(p, 0, 1);
        ILUPP_HIP(hipMemsetAsync(p->btk, 0, sizeof(int32_t), st));
        ILUPP_HIP(hipEventRecord(p->ev[3], st));
        const dim3 g((unsigned)(((int64_t)n + 255) / 256)), b(256);
        for (int64_t j = 0; j < k; ++j) {
            hipLaunchKernelGGL(k_col_gather, g, b, 0, st, X + j, k, n, p->bcol);
            const int rc = apply_dev(p, p->bcol, transpose);
            if (rc) return rc;
            hipLaunchKernelGGL(k_col_scatter, g, b, 0, st, p->bcol, X + j, k, n, p->ctrl, p->btk);
        }
        ILUPP_HIP(hipGetLastError());
        ILUPP_HIP(hipMemcpyAsync(p->ctrl, p->btk, sizeof(int32_t), hipMemcpyDeviceToDevice, st));     // (what finish_apply reads)
        ILUPP_HIP(hipEventRecord(p->ev[2], st));
        p->block_events = true;
        return ILUPP_OK;
    }
    int64_t chunks = 0;
    int kbmax = 0;
    for (int64_t c0 = 0; c0 < k; c0 += chunk_width(k - c0)) { ++chunks; kbmax = chunk_width(k - c0) > kbmax ? chunk_width(k - c0) : kbmax; }
    block_buffers(p, kbmax, 1 + 2 * chunks);
    if (p->ctrl_armed) p->ctrl_armed = false;            // (zero already: arm_apply)
    else ILUPP_HIP(hipMemsetAsync(p->ctrl, 0, 64, st));
    ILUPP_HIP(hipMemsetAsync(p->btk, 0, sizeof(int32_t) * (size_t)(1 + 2 * chunks), st));
    ILUPP_HIP(hipEventRecord(p->ev[3], st));
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    int64_t q = 0;
    for (int64_t c0 = 0; c0 < k; ++q) {
        const int kb = chunk_width(k - c0);
        // X's columns [c0, c0 + kb) -> the intermediate chunk (leading dimension kb) -> back in place
        int rc = sptrsm_lvl(st, *l1, kb, X + c0, k, p->by, kb, p->bxp, p->btk + 1 + 2 * q, p->ctrl);
        if (rc) return rc;
        if (q == 0) ILUPP_HIP(hipEventRecord(p->ev[1], st));
        rc = sptrsm_lvl(st, *l2, kb, p->by, kb, X + c0, k, p->bxp, p->btk + 2 + 2 * q, p->ctrl);
        if (rc) return rc;
        c0 += kb;
    }
    ILUPP_HIP(hipEventRecord(p->ev[2], st));
    p->apply_events_valid = true;
    p->block_events = true;
    return ILUPP_OK;
}

int ilu0_create_common(const DevMat &A, int is_csr, const int32_t *head, ilupp_precond **out, ilupp_precond *made = nullptr)
{
    ObjGuard g(made ? made : new_obj(A.n));
    ilupp_precond *p = g.p;
    p->kind = KIND_LU;
    p->nnz_mode = NNZ_GENERIC_LU;
    p->input_csc = !is_csr;
    const int rc = ilu0_factor(p, A, head);
    if (rc) return rc;
    *out = g.release();
    return ILUPP_OK;
}

// what ilupp_hip_ilu0_create_device does, under the construction lock its caller holds (the batched construction runs it for the members
// that do not go to its launches)
int ilu0_create_device_locked(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int is_csr, ilupp_precond **out)
{
    if (n <= 0 || !d_indptr) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
    // indptr[n], and the head of the matrix for grid.hip's guess: one read-back
    int32_t head[10];
    ObjGuard g(new_obj(n));                        // (first: the read-back below also cleans the object's verdict word)
    const int32_t nnz32 = read_device_head(d_indptr, d_indices, n, head, g.p->ctrl + 8);
    g.p->verdict_clean = true;
    return ilu0_create_common(borrow_csr(d_data, d_indices, d_indptr, n, nnz32, true), is_csr, head, out, g.release());
}

// what ilupp_hip_ilu0_refactor_device does, under the construction lock its caller holds (the batched re-factorisation runs it for the
// members that do not go to its launch)
bool is_ilu0_object(const ilupp_precond *p)
{
    return p && p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU && (p->sA.nb > 0 || p->batch_built);
}

// the launch of the batched re-factorisation with this one member (defined with that launch's host code, below): the single
// re-factorisation of a batch-built object, which has none of the single numeric paths' tables
int refactor_in_launch(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr);

// behind a re-factorisation: every copy of the OLD values goes (the static forms' transposed records, the level-ordered sweeps, the
// transposed storages with their schedules, descriptors and packed sweeps); each is built again on its first use.  The caller has
// waited for whatever still reads them: the pool knows nothing of streams.
void drop_old_value_copies(ilupp_precond *p)
{
    p->apply_events_valid = false;
    st_drop_transposed(&p->pkL, &p->pkU);
    for (auto &l : p->lvl) l.release();
    if (p->haveT) {
        p->LcT.release(); p->UcT.release(); p->sUT.release(); p->sLT.release();
        if (p->dUT) (void)pool_free(p->dUT);
        if (p->dLT) (void)pool_free(p->dLT);
        p->dUT = p->dLT = nullptr; p->haveT = false;
        p->pkUT.release(); p->pkLT.release(); p->pack_tried[2] = p->pack_tried[3] = false;
    }
}

// an IChol(0) object's copies of the factor's values beside Lc and LcT: the packed sweeps of the two (level-major or the static pair)
// and the level-ordered copies; each is built again on its first use.  The caller has waited for whatever still reads them.
void drop_llt_sweep_copies(ilupp_precond *p)
{
    p->apply_events_valid = false;
    for (auto &l : p->lvl) l.release();
    p->pkL.release(); p->pkLT.release();
    p->pack_tried[0] = p->pack_tried[3] = false; p->pair_tried = false;
}

// an IChol(0) object: LL^T with the factor row-major and the diagonal last (ICholT keeps its factor column-major)
bool is_ichol0_object(const ilupp_precond *p)
{
    return p && p->kind == KIND_LLT && p->nnz_mode == NNZ_LLT && p->llt_diag_last && (p->sL.nb > 0 || p->batch_built);
}

// what ilupp_hip_ichol0_refactor_device does, under the construction lock its caller holds: the pattern proved and Lc's values refilled with
// A's lower triangle by two launches around one read-back, then the constructor's numeric path in place on Lc
int ichol0_refactor_single(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr)
{
    if (!is_ichol0_object(p)) { set_error("not an IChol(0) object"); return ILUPP_ERR_INVALID; }
    order_after_caller(p->stream, p->sev[0]);
    if (p->batch_ev) { ILUPP_HIP(hipStreamWaitEvent(p->stream, p->batch_ev, 0)); p->batch_ev = nullptr; }      // (a batched launch still reads the old factor)
    if (p->batch_built) return refactor_in_launch(p, d_data, d_indices, d_indptr);
    hipStream_t st = p->stream;
    {
        int32_t *d_bad = p->ctrl + 2, bad = 1;       // (ctrl[2]: a word no sweep of such an object uses)
        OR_RETURN(ichol0_refill_proof(st, p->n, p->nnzA, d_indptr, d_indices, p->Lc, d_bad));
        ILUPP_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ILUPP_HIP(hipStreamSynchronize(st));
        if (bad) { set_error("IChol0 refactor: the matrix does not have the analysed pattern"); return ILUPP_ERR_INVALID; }
    }
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    OR_RETURN(ichol0_refill(st, p->n, d_indptr, d_indices, d_data, &p->Lc));
    float kms = 0.f;
    int rc = ILUPP_OK;
    if (!(p->chol_static && ichol0_numeric_st(st, &p->Lc, p->sL, p->ctrl, &kms, &rc)))
        rc = ichol0_numeric(st, &p->Lc, p->sL, p->max_row_len, p->done, p->ctrl, &kms);
    ILUPP_HIP(hipEventRecord(p->ev[2], st));
    ILUPP_HIP(stream_sync(st));
    ILUPP_HIP(hipEventElapsedTime(&p->tm.numeric_ms, p->ev[1], p->ev[2]));
    p->tm.numeric_kernel_ms = kms;
    drop_old_value_copies(p);
    drop_llt_sweep_copies(p);
    if (rc == ILUPP_OK) settle_ctrl(p);
    if (rc == ILUPP_ERR_TIMEOUT) set_error("IChol0: dependency wait timed out");
    return rc;
}

int ilu0_refactor_single(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr)
{
    if (!is_ilu0_object(p)) { set_error("not an ILU(0) object"); return ILUPP_ERR_INVALID; }
    order_after_caller(p->stream, p->sev[0]);
    if (p->batch_ev) { ILUPP_HIP(hipStreamWaitEvent(p->stream, p->batch_ev, 0)); p->batch_ev = nullptr; }      // (a batched launch still reads the old factor)
    {
        // same pattern as the analysed one: at least the same number of stored entries
        int32_t nnz32 = -1;
        ILUPP_HIP(hipMemcpyAsync(&nnz32, d_indptr + p->n, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
        ILUPP_HIP(hipStreamSynchronize(p->stream));
        if ((int64_t)nnz32 != p->nnzA) { set_error("ILU0 refactor: the matrix does not have the analysed pattern"); return ILUPP_ERR_INVALID; }
    }
    if (p->batch_built) return refactor_in_launch(p, d_data, d_indices, d_indptr);
    const DevMat A = borrow_csr(d_data, d_indices, d_indptr, p->n, p->nnzA, true);
    hipStream_t st = p->stream;
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    float kms = 0.f;
    int rc = ilu0_numeric_any(p, A, p->prog.prog != nullptr, &kms, nullptr);
    ILUPP_HIP(hipEventRecord(p->ev[2], st));
    ILUPP_HIP(stream_sync(st));
    ILUPP_HIP(hipEventElapsedTime(&p->tm.numeric_ms, p->ev[1], p->ev[2]));
    p->tm.numeric_kernel_ms = kms;
    drop_old_value_copies(p);
    if (rc == ILUPP_OK) settle_ctrl(p);
    if (rc == ILUPP_ERR_TIMEOUT) set_error("ILU0: dependency wait timed out");
    return rc;
}

}  // namespace

extern "C" {

int ilupp_hip_index_size(void) { return (int)sizeof(int32_t); }

const char *ilupp_hip_last_error(void) { return ilupp::g_last_error.c_str(); }

int ilupp_hip_set_device(int device)
{
    API_TRY
    ILUPP_HIP(hipSetDevice(device));
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int ilupp_hip_ilu0_create(const double *data, const int32_t *indices, const int32_t *indptr,
                          int32_t n, int is_csr, ilupp_precond **out)
{
    return create_from_host(data, indices, indptr, n, true, out, [&](DevMat &A) {
        int32_t head[10];
        host_head(indptr, indices, A.nnz, head);
        return ilu0_create_common(A, is_csr, head, out);
    });
}

int ilupp_hip_ilu0_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                 int32_t n, int is_csr, ilupp_precond **out)
{
    API_TRY_BUILD
    if (!out) { set_error("null output"); return ILUPP_ERR_INVALID; }
    *out = nullptr;
    return ilu0_create_device_locked(d_data, d_indices, d_indptr, n, is_csr, out);
    API_CATCH
}

int ilupp_hip_ilu0_create_device_nnz(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                     int32_t n, int64_t nnz, int is_csr, ilupp_precond **out)
{
    {
        API_TRY_BUILD
        if (!out) { set_error("null output"); return ILUPP_ERR_INVALID; }
        *out = nullptr;
        if (n <= 0 || !d_indptr) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
        // the dimensions a matrix of this size had when it last was a box grid: the head a grid of those dimensions has (nothing is read)
        GridDims gd = {0, 0, 0};
        if (nnz > 0 && nnz < (1LL << 31) && grid_shape_recall(n, nnz, &gd, d_indices)) {
            int32_t head[10] = {0, gd.nz > 1 ? 4 : 3, 0, 1, gd.nx, gd.nz > 1 ? gd.nx * gd.ny : -1, -1, -1, -1, -1};
            ObjGuard g(new_obj(n));
            g.p->no_general_retry = true;          // (a failed proof must not run the general pass with an nnz nobody has checked)
            const int rc = ilu0_create_common(borrow_csr(d_data, d_indices, d_indptr, n, nnz, true), is_csr, head, out, g.release());
            if (rc != ILUPP_ERR_UNSUPPORTED) return rc;
        }
        API_CATCH
    }
    // the reading way; the caller's nnz is checked against indptr[n]
    const int rc = ilupp_hip_ilu0_create_device(d_data, d_indices, d_indptr, n, is_csr, out);
    if (rc == ILUPP_OK && *out && (*out)->nnzA != nnz) {
        ilupp_hip_destroy(*out); *out = nullptr;
        set_error("ILU0: the number of stored entries handed in is not indptr[n]");
        return ILUPP_ERR_INVALID;
    }
    return rc;
}

int ilupp_hip_ilu0_refactor_device(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr)
{
    API_TRY_BUILD
    return ilu0_refactor_single(p, d_data, d_indices, d_indptr);
    API_CATCH
}

}  // extern "C"

namespace ilupp {

// ILUC: A = the major-order view (CSR arrays of the input, whatever its orientation: ILUC2 works on dim_along_orientation)
// the sweeps of an object whose two factors both read as upper CSR matrices with the diagonal first (ILUC; a level of the multilevel
// preconditioner): backward schedules and descriptors of the stored arrays (the forward sweeps run on transposed copies, built on first use)
void utu_analyse(ilupp_precond *p)
{
    p->compact = sweep_tables(p->stream, p, {&p->Lc, false, &p->sL, &p->dL}, {&p->Uc, false, &p->sU, &p->dU}, true, &p->max_row_len);
}

}  // namespace ilupp

static int iluc_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    // (guards: an ILUPP_HIP that throws below must leave neither the object nor the factors behind)
    ObjGuard og(new_obj(n));
    ilupp_precond *p = og.p;
    p->kind = KIND_UTU;
    p->nnz_mode = NNZ_GENERIC_LU;
    p->input_csc = !is_csr;
    hipStream_t st = p->stream;
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    int32_t err_row = -1;
    float kms = 0.f;
    MatGuard gl, gu;
    DevMat &Lcol = gl.m, &Urow = gu.m;             // L by columns (unit diagonal first), U by rows (pivot first)
    int rc = iluc_factor(st, A, max_fill_in, threshold, &Lcol, &Urow, &err_row, &kms);
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    A.release();
    if (rc) {
        if (rc == ILUPP_ERR_ZERO_PIVOT) set_error("ILUC2: zero pivot on diagonal, k=" + std::to_string(err_row));               // ILUC.hpp:174-175
        else if (rc == ILUPP_ERR_MEMORY) set_error("append_row_with_prefix: insufficient memory reserved");                       // sparse_implementation.h:3196-3197
        else if (rc == ILUPP_ERR_TIMEOUT) set_error("ILUC: dependency wait timed out");
        return rc;
    }
    // ROW input: left = L (columns), right = U (rows); COLUMN input: ILUC2(A, right, left): left = U of the view, right = L of the
    // view (preconditioner_implementation.h:940-951) -- and iluc() interchanges the same way (binding.cpp:456-457)
    if (is_csr) { p->Lc = Lcol; p->Uc = Urow; } else { p->Lc = Urow; p->Uc = Lcol; }
    Lcol.ptr = Lcol.idx = nullptr; Lcol.val = nullptr; Urow.ptr = Urow.idx = nullptr; Urow.val = nullptr;      // (the object owns them now)
    utu_analyse(p);
    finish_timing(p, kms);
    *out = og.release();
    return ILUPP_OK;
}

static int ilut_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out,
                              ilupp_precond *made = nullptr)
{
    ObjGuard g(made ? made : new_obj(n));
    ilupp_precond *p = g.p;
    p->kind = KIND_LU;
    p->nnz_mode = NNZ_ILUT;
    p->input_csc = !is_csr;      // CSC: factor the row-major view A^T, swap roles on egress (preconditioner_implementation.h:999-1001)
    hipStream_t st = p->stream;
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    int32_t err_row = -1;
    float kms = 0.f;
    const int rc = ilut_factor(st, A, max_fill_in, threshold, &p->Lc, &p->Uc, &err_row, &kms);
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    A.release();
    if (rc) {
        if (rc == ILUPP_ERR_ZERO_PIVOT) set_error("ILUT_heap: encountered zero pivot in row " + std::to_string(err_row));   // ILUT.hpp:269-270
        else if (rc == ILUPP_ERR_TIMEOUT) set_error("ILUT: dependency wait timed out");
        else set_error("ILUT: working row overflow");
        return rc;
    }
    // solve schedules from the factors' own patterns
    p->compact = sweep_tables(st, p, {&p->Lc, true, &p->sL, &p->dL}, {&p->Uc, false, &p->sU, &p->dU}, true, &p->max_row_len);
    finish_timing(p, kms);
    *out = g.release();
    return ILUPP_OK;
}

extern "C" {

int ilupp_hip_ilut_create(const double *data, const int32_t *indices, const int32_t *indptr,
        int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    return create_from_host(data, indices, indptr, n, true, out,
                            [&](DevMat &A) { return ilut_create_common(A, n, is_csr, max_fill_in, threshold, out); });
}

/* the same on a matrix that already lives in HBM (borrowed for the call) */
int ilupp_hip_ilut_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
        int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    return create_from_device(d_data, d_indices, d_indptr, n, true, out,
                              [&](DevMat &A) { return ilut_create_common(A, n, is_csr, max_fill_in, threshold, out); });
}

/* binding.cpp:329-340 ILUCPreconditioner(A, max_fill_in, threshold): Crout ILU (Li, Saad, Chow), ILUC.hpp:112-207 */
int ilupp_hip_iluc_create(const double *data, const int32_t *indices, const int32_t *indptr,
        int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    return create_from_host(data, indices, indptr, n, true, out,
                            [&](DevMat &A) { return iluc_create_common(A, n, is_csr, max_fill_in, threshold, out); });
}

int ilupp_hip_iluc_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
        int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    return create_from_device(d_data, d_indices, d_indptr, n, true, out,
                              [&](DevMat &A) { return iluc_create_common(A, n, is_csr, max_fill_in, threshold, out); });
}

}  // extern "C"

static int ichol0_create_common(DevMat &A, int32_t n, ilupp_precond **out, ilupp_precond *made = nullptr)
{
    ObjGuard g(made ? made : new_obj(n));
    ilupp_precond *p = g.p;
    p->nnzA = A.nnz;
    p->kind = KIND_LLT;
    p->nnz_mode = NNZ_LLT;
    p->llt_diag_last = true;
    hipStream_t st = p->stream;
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    int32_t missing = -1;
    int rc = triangular_part(st, A, true, &p->Lc, &missing);
    ILUPP_HIP(stream_sync(st));
    A.release();
    if (rc == ILUPP_ERR_NO_DIAGONAL) {
        set_error("IChol0: structurally missing diagonal entry in row " + std::to_string(missing));
        return rc;
    }
    p->Lc.is_csr = true;
    p->compact = sweep_tables(st, p, {&p->Lc, true, &p->sL, &p->dL}, {}, true, &p->max_row_len);
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    float kms = 0.f;
    // stencil-like lower triangles whose rows are "simple" (5-/7-point): the static form (st.hip); everything else: the dataflow kernel over chains
    p->chol_static = ichol0_numeric_st(st, &p->Lc, p->sL, p->ctrl, &kms, &rc);
    if (!p->chol_static)
        rc = ichol0_numeric(st, &p->Lc, p->sL, p->max_row_len, p->done, p->ctrl, &kms);
    finish_timing(p, kms, true);
    if (rc) {
        if (rc == ILUPP_ERR_TIMEOUT) set_error("IChol0: dependency wait timed out");
        return rc;
    }
    *out = g.release();
    return ILUPP_OK;
}

extern "C" {

int ilupp_hip_ichol0_create(const double *data, const int32_t *indices, const int32_t *indptr,
        int32_t n, int is_csr, ilupp_precond **out)
{
    (void)is_csr;     // IChol0 keeps idx <= major in either orientation and labels the result ROW (IChol.hpp:63-68)
    return create_from_host(data, indices, indptr, n, true, out,
                            [&](DevMat &A) { return ichol0_create_common(A, n, out); });
}

int ilupp_hip_ichol0_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
        int32_t n, int is_csr, ilupp_precond **out)
{
    return create_from_device(d_data, d_indices, d_indptr, n, true, out,
                              [&](DevMat &A) { return ichol0_create_common(A, n, out); });
}

int ilupp_hip_ichol0_refactor_device(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr)
{
    API_TRY_BUILD
    if (!p || !d_data || !d_indices || !d_indptr) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    return ichol0_refactor_single(p, d_data, d_indices, d_indptr);
    API_CATCH
}
}  // extern "C"

static int icholt_create_common(DevMat &A, int32_t n, int32_t add_fill_in, double threshold, ilupp_precond **out, const int32_t *head)
{
    int rc = ILUPP_OK;
    ObjGuard g(new_obj(n));
    ilupp_precond *p = g.p;
    p->kind = KIND_LLT;
    p->nnz_mode = NNZ_LLT;
    p->llt_diag_last = false;
    hipStream_t st = p->stream;
    ILUPP_HIP(hipEventRecord(p->ev[0], st));
    float kms = 0.f;
    // the schedule of the sweeps: Lc = CSC lower, diagonal first; its arrays read as CSR are L^T (upper, diagonal first): backward sweep
    auto sweep_schedule = [&](hipStream_t q) {
        p->degenerate = min_row_len(q, n, p->Lc.ptr, p->Lc.idx, 1) == 0;      // (column-major lower: diagonal first)
        p->compact = sweep_tables(q, p, {&p->Lc, false, &p->sL, &p->dL}, {}, true, &p->max_row_len);
    };
    // no fill allowed, nothing dropped by size, on a box grid: every column keeps A's entries if they all outweigh the one-step fill --
    // assumed, computed on the wavefront x + 2y + 3z, verified column by column (icholt_grid.hip); anything else: the general way.
    // L's pattern is A's then: the sweeps' schedule is made on the side stream while the kernel runs.
    GridDims gd = {0, 0, 0};
    if (add_fill_in == 0 && threshold == 0.0 && head && grid_guess(A.n, A.nnz, head, &gd)) {
        IcholtGridJob job;
        const auto w0 = std::chrono::steady_clock::now();
        // L's pattern is the grid's: blocks and patches of the sweeps' schedule from the dimensions, no pass over the pattern (env
        // ILUPP_IG_SCHED=general: the general pass; =verify: both, compared)
        static const char *sched_mode = getenv("ILUPP_IG_SCHED");
        const bool sched_verify = sched_mode && !strcmp(sched_mode, "verify");
        bool sched_done = false;
        // (nothing of the closed-form schedule reads L's arrays: it is queued ahead of the kernel that writes them)
        auto schedule_early = [&](hipStream_t q) {
            if (sched_mode) return;
            if (!grid_llt_schedule(q, n, gd, p->max_lanes, &p->sL)) return;
            p->degenerate = false;
            p->max_row_len = 1 + (gd.nx > 1) + (gd.ny > 1) + (gd.nz > 1);
            build_slot_tables(q, &p->sL, false);
            p->compact = schedule_is_compact(p->sL);
            // (the descriptors and the factor's own index arrays in one pass over the columns)
            if (p->compact) { make_desc_llt_grid(q, p->Lc, p->sL, gd, &p->dL, true); job.pattern_written = true; }
            sched_done = true;
        };
        auto schedule_on = [&](hipStream_t q) {
            if (sched_done) return;
            const bool want_general = sched_mode && !strcmp(sched_mode, "general");
            if (!want_general && grid_llt_schedule(q, n, gd, p->max_lanes, &p->sL)) {
                p->degenerate = false;                              // (every column has its diagonal)
                p->max_row_len = 1 + (gd.nx > 1) + (gd.ny > 1) + (gd.nz > 1);
                if (sched_verify) {
                    Schedule ref;
                    int32_t m1 = 0;
                    count_cuts_and_schedule(q, n, p->Lc.ptr, p->Lc.idx, p->max_lanes, nullptr, &ref, &m1);
                    choose_tiling(q, n, p->Lc.ptr, p->Lc.idx, &ref, false, p->max_lanes / kThreads);
                    bool same = ref.nb == p->sL.nb && ref.B == p->sL.B && ref.tile_s2 == p->sL.tile_s2 && ref.tile_ty == p->sL.tile_ty &&
                                ref.tile_tz == p->sL.tile_tz && m1 == p->max_row_len && min_row_len(q, n, p->Lc.ptr, p->Lc.idx, 1) != 0;
                    if (same) {
                        std::vector<int32_t> a((size_t)ref.nb + 1), b((size_t)ref.nb + 1);
                        ILUPP_HIP(hipMemcpyAsync(a.data(), ref.start, sizeof(int32_t) * a.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipMemcpyAsync(b.data(), p->sL.start, sizeof(int32_t) * b.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipStreamSynchronize(q));
                        same = a == b;
                    }
                    ref.release();
                    if (!same) { set_error("ICholT grid path: the schedule from the dimensions differs from the general pass'"); throw HipError{hipErrorUnknown, "ILUPP_IG_SCHED=verify", __FILE__, __LINE__}; }
                }
                build_slot_tables(q, &p->sL, false);
                p->compact = schedule_is_compact(p->sL);
                if (p->compact) {
                    make_desc_llt_grid(q, p->Lc, p->sL, gd, &p->dL);
                    if (sched_verify) {
                        // ... and the descriptors: the general kernel's, word for word (the export marks too)
                        std::vector<int32_t> d1((size_t)p->Lc.nnz), d2((size_t)p->Lc.nnz), e1((size_t)p->sL.nslots), e2((size_t)p->sL.nslots);
                        ILUPP_HIP(hipMemcpyAsync(d1.data(), p->dL, sizeof(int32_t) * d1.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipMemcpyAsync(e1.data(), p->sL.exported, sizeof(int32_t) * e1.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipStreamSynchronize(q));
                        ILUPP_HIP(hipMemsetAsync(p->sL.exported, 0, sizeof(int32_t) * e1.size(), q));
                        int32_t *ref = nullptr;
                        make_desc(q, p->Lc, p->sL, &ref, false);
                        ILUPP_HIP(hipMemcpyAsync(d2.data(), ref, sizeof(int32_t) * d2.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipMemcpyAsync(e2.data(), p->sL.exported, sizeof(int32_t) * e2.size(), hipMemcpyDeviceToHost, q));
                        ILUPP_HIP(hipStreamSynchronize(q));
                        (void)pool_free(ref);
                        if (d1 != d2 || e1 != e2) { set_error("ICholT grid path: the descriptors from the dimensions differ from the general kernel's"); throw HipError{hipErrorUnknown, "ILUPP_IG_SCHED=verify", __FILE__, __LINE__}; }
                    }
                }
            } else {
                sweep_schedule(q);
            }
        };
        if (icholt_grid_launch(st, p->side, A, gd, p->ctrl, &p->Lc, &job, schedule_early, schedule_on)) {
            hipStream_t q = p->side ? p->side : st;
            const auto w1 = std::chrono::steady_clock::now();
            ILUPP_HIP(stream_sync(q));
            const auto w2 = std::chrono::steady_clock::now();
            p->icholt_grid = icholt_grid_finish(st, &job, &kms);
            if (p->icholt_grid) p->llt_gd = gd;
            if (getenv("ILUPP_IG_DEBUG")) {
                const auto w3 = std::chrono::steady_clock::now();
                fprintf(stderr, "icholt_grid host: launch %.3f ms, sweep schedule %.3f ms, wait %.3f ms\n", std::chrono::duration<double, std::milli>(w1 - w0).count(),
                        std::chrono::duration<double, std::milli>(w2 - w1).count(), std::chrono::duration<double, std::milli>(w3 - w2).count());
            }
            if (!p->icholt_grid) {
                p->Lc.release(); p->sL.release();
                if (p->dL) { (void)pool_free(p->dL); p->dL = nullptr; }
            }
        }
    }
    if (!p->icholt_grid) {
        MatGuard T;
        int32_t missing = -1;
        rc = triangular_part(st, A, false, &T.m, &missing);      // natural_triangular_part(false): keep idx >= major
        ILUPP_HIP(stream_sync(st));
        A.release();
        // a missing diagonal is caught by the reference inside the column loop (IChol.hpp:105-107); same error here
        rc = icholt_factor(st, T.m, add_fill_in, threshold, &p->Lc, &kms);
        T.m.release();
    } else {
        A.release();
    }
    ILUPP_HIP(hipEventRecord(p->ev[1], st));
    if (rc) {
        if (rc == ILUPP_ERR_NOT_TRIANGULAR) set_error("ICholT: A must be in triangular form with no zeros on the diagonal");
        else if (rc == ILUPP_ERR_NOT_SPD) set_error("ICholT: the pivot of a column is NaN (the matrix is not positive definite); "
                                                         "the reference returns a NaN-filled factor here");
        else if (rc == ILUPP_ERR_DIAG_DROPPED) set_error("ICholT: the diagonal entry of a column was dropped by the threshold or the fill budget "
                                                              "(threshold too large / budget too small for this matrix); the reference keeps such a "
                                                              "factor and divides by the column's first stored entry, this build does not support it");
        else if (rc == ILUPP_ERR_TIMEOUT) set_error("ICholT: dependency wait timed out");
        else set_error("append_row: insufficient memory reserved (or a working column beyond the kernel's largest capacity class)");
        return rc;
    }
    if (!p->icholt_grid) sweep_schedule(st);
    finish_timing(p, kms);
    *out = g.release();
    return ILUPP_OK;
}

extern "C" {

int ilupp_hip_icholt_create(const double *data, const int32_t *indices, const int32_t *indptr,
        int32_t n, int is_csr, int32_t add_fill_in, double threshold, ilupp_precond **out)
{
    (void)is_csr;     // ICholT keeps idx >= major in either orientation and labels the result COLUMN (IChol.hpp:158-164)
    return create_from_host(data, indices, indptr, n, true, out, [&](DevMat &A) {
        int32_t head[10];
        host_head(indptr, indices, A.nnz, head);
        return icholt_create_common(A, n, add_fill_in, threshold, out, head);
    });
}

int ilupp_hip_icholt_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
        int32_t n, int is_csr, int32_t add_fill_in, double threshold, ilupp_precond **out)
{
    API_TRY_BUILD
    if (!out) { set_error("null output"); return ILUPP_ERR_INVALID; }
    *out = nullptr;
    if (n <= 0 || !d_indptr) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
    int32_t head[10];
    DevMat A = borrow_csr(d_data, d_indices, d_indptr, n, read_device_head(d_indptr, d_indices, n, head), true);
    return icholt_create_common(A, n, add_fill_in, threshold, out, head);
    API_CATCH
}

void ilupp_hip_destroy(ilupp_precond *p) { destroy_obj(p); }

int ilupp_hip_apply_device(ilupp_precond *p, double *d_x, int64_t len, int transpose, int sync)
{
    API_TRY
    OR_RETURN(vector_args(p, len, p ? p->n : 0));
    OR_RETURN(apply_dev(p, d_x, transpose));
    return finish_or_hand_over(sync, *p, [&] { return finish_apply(p); });
    API_CATCH
}

static int block_args(const ilupp_precond *p, int64_t n, int64_t k)
{
    OR_RETURN(vector_args(p, n, p ? p->n : 0));
    if (k < 0) { set_error("number of right-hand sides must not be negative"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

int ilupp_hip_apply_block_device(ilupp_precond *p, double *d_X, int64_t n, int64_t k, int transpose, int sync)
{
    API_TRY
    int rc = block_args(p, n, k);
    if (rc || k == 0) return rc;
    OR_RETURN(apply_block_dev(p, d_X, k, transpose));
    return finish_or_hand_over(sync, *p, [&] { return finish_apply(p); });
    API_CATCH
}

// host X: staged through the device in pieces of at most this many bytes (whole chunks of kSptrsmMaxKB columns where more than one fits)
static constexpr int64_t kBlockStageBytes = (int64_t)256 << 20;

int ilupp_hip_apply_block(ilupp_precond *p, double *X, int64_t n, int64_t k, int transpose)
{
    API_TRY
    int rc = block_args(p, n, k);
    if (rc || k == 0) return rc;
    int64_t cb = kBlockStageBytes / (8 * n);
    if (cb > kSptrsmMaxKB) cb -= cb % kSptrsmMaxKB;
    cb = cb < 1 ? 1 : (cb > k ? k : cb);
    hipStream_t st = p->stream;
    struct Stage { hipStream_t st; double *d = nullptr; ~Stage() { if (d) { (void)stream_sync(st); (void)pool_free(d); } } } stage{st};
    ILUPP_HIP(pool_malloc(&stage.d, sizeof(double) * (size_t)n * (size_t)cb));
    std::vector<double> pack(cb < k ? (size_t)n * (size_t)cb : 0);
    float total_ms = 0.0f;
    for (int64_t c0 = 0; c0 < k; c0 += cb) {
        const int64_t w = k - c0 < cb ? k - c0 : cb;
        const size_t bytes = sizeof(double) * (size_t)n * (size_t)w;
        if (w == k) {
            ILUPP_HIP(hipMemcpyAsync(stage.d, X, bytes, hipMemcpyHostToDevice, st));
        } else {
            for (int64_t i = 0; i < n; ++i) memcpy(&pack[(size_t)(i * w)], X + i * k + c0, sizeof(double) * (size_t)w);
            ILUPP_HIP(hipMemcpyAsync(stage.d, pack.data(), bytes, hipMemcpyHostToDevice, st));
        }
        rc = apply_block_dev(p, stage.d, w, transpose);
        if (rc) return rc;
        rc = finish_apply(p);
        if (rc) return rc;
        total_ms += p->tm.last_apply_ms;
        ILUPP_HIP(hipMemcpyAsync(w == k ? X : pack.data(), stage.d, bytes, hipMemcpyDeviceToHost, st));
        ILUPP_HIP(stream_sync(st));
        if (w != k)
            for (int64_t i = 0; i < n; ++i) memcpy(X + i * k + c0, &pack[(size_t)(i * w)], sizeof(double) * (size_t)w);
    }
    p->tm.last_apply_ms = total_ms;
    return ILUPP_OK;
    API_CATCH
}

const char *ilupp_hip_block_path(const ilupp_precond *p) { return p ? p->block_path : ""; }

int ilupp_hip_set_caller_stream(void *hip_stream, int enable)
{
    g_caller_stream = static_cast<hipStream_t>(hip_stream);
    g_caller_stream_set = enable != 0;
    return ILUPP_OK;
}

const char *ilupp_hip_path(const ilupp_precond *p)
{
    if (!p) return "";
    if (p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU) {
        if (p->batch_built) return "ilu0:batch";
        if (p->flm.built) return p->flm.direct ? "ilu0:static-direct" : "ilu0:static-level-major";
        if (p->fperm) return "ilu0:level-order";
        return p->prog_f3 ? "ilu0:csr-program" : "ilu0:csr";
    }
    if (p->kind == KIND_LU) return p->batch_built ? "ilut:batch" : "ilut";
    if (p->kind == KIND_UTU) return "iluc";
    if (p->llt_diag_last && p->batch_built) return "ichol0:batch";
    return p->llt_diag_last ? (p->chol_static ? "ichol0:static-level-major" : "ichol0") : (p->icholt_grid ? "icholt:grid-static" : "icholt");
}

/* diagnostics: table `which` of a static ILU(0) object as 32-bit words (0 / 1: lane tables of the forward / backward schedule, 2 / 3: chunk
 * tables, 4: backward right-hand-side map, 5: rows-pass records, 6 / 7: export ordinals, 8 / 9: exchange layout, 10: forward -> backward
 * slots, 11 / 12: skews); returns the number of words copied (at most cap), -1 for an object without such a table */
long long ilupp_hip_debug_static_table(ilupp_precond *p, int which, int32_t *out, long long cap)
{
    try {
        if (!p || !(p->flm.built && p->flm.stat) || !out) return -1;
        const long long ns = p->sA.nslots, nwg = ns / kThreads;
        const int32_t *src = nullptr; long long cnt = 0;
        switch (which) {
            case 0: src = p->pkL.ltab; cnt = ns * kStTab; break;
            case 1: src = p->pkU.ltab; cnt = ns * kStTab; break;
            case 2: src = p->pkL.wtab; cnt = nwg * 16; break;
            case 3: src = p->pkU.wtab; cnt = nwg * 16; break;
            case 4: src = p->pkU.ysrc; cnt = ns; break;
            case 5: src = (p->flm.xbase && p->flm.xbase_len >= (int64_t)ns * 33) ? p->flm.xbase + ns : nullptr; cnt = ns * 32; break;
            case 6: src = p->pkL.xe; cnt = ns; break;
            case 7: src = p->pkU.xe; cnt = ns; break;
            case 8: src = p->pkL.xw; cnt = nwg * 4; break;
            case 9: src = p->pkU.xw; cnt = nwg * 4; break;
            case 10: src = p->pkU.uslot; cnt = ns; break;
            case 11: src = p->pkL.skew; cnt = ns; break;
            case 12: src = p->pkU.skew; cnt = ns; break;
            default: return -1;
        }
        if (!src) return -1;
        if (cnt > cap) cnt = cap;
        ILUPP_HIP(stream_sync(p->stream));
        ILUPP_HIP(hipMemcpy(out, src, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost));
        return cnt;
    } catch (...) { return -1; }
}

/* diagnostics: the level order of slot `which` (0 .. 3: lvl[] = Lc, Uc, UcT, LcT; 4: the factor order of an "ilu0:level-order" object) as
 * perm[position] = row, and in info[] {levels, the sweep's w, its block, how it was numbered (0 given, 1 natural pass, 2 relaxation,
 * 3 relaxation given up then natural pass), relaxation batches, W of the natural pass, route of the last sweep over the slot (SweepRoute), its kernel
 * when that route is the descriptor kernels (1 k_sptrsv_lc, 2 k_sptrsv_desc; else 0)}.
 * Builds nothing; -1 where that order does not exist (info[6] and [7] are still the slot's last route and kernel then, the rest zero) */
long long ilupp_hip_debug_level_order(ilupp_precond *p, int which, int32_t *perm_out, long long cap, int32_t info[8])
{
    try {
        if (info) for (int k = 0; k < 8; ++k) info[k] = 0;
        if (!p || !info || which < 0 || which > 4) return -1;
        const int32_t *src = nullptr;
        LevelNumbering how;
        if (which == 4) {
            if (!p->fperm) return -1;
            src = p->fperm; how = p->fperm_how;
            info[0] = p->fperm_levels;
        } else {
            const LevelSweep &ls = p->lvl[which];
            info[6] = p->last_route[which];
            info[7] = p->last_route[which] == SWEPT_DESCRIPTORS ? p->last_desc_kernel[which] : 0;
            if (!ls.valid || !ls.perm) return -1;
            src = ls.perm; how = ls.how;
            info[0] = ls.nlevels; info[1] = ls.w; info[2] = ls.block;
        }
        info[3] = how.route; info[4] = how.batches; info[5] = how.w;
        long long cnt = perm_out ? p->n : 0;
        if (cnt > cap) cnt = cap;
        if (cnt < 0) cnt = 0;
        ILUPP_HIP(stream_sync(p->stream));
        if (cnt > 0) ILUPP_HIP(hipMemcpy(perm_out, src, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost));
        return cnt;
    } catch (...) { return -1; }
}

const char *ilupp_hip_analysis_path(const ilupp_precond *p)
{
    if (!p || !(p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU)) return "";
    return p->grid_path ? "grid" : "general";
}

// which kernels a static ILU(0) object runs: "factor kernel;forward sweep;backward sweep" (measurement hook next to ilupp_hip_path:
// bench.py labels its roofline phases and looks the kernels' counter traffic up by these names); "" for any other object
const char *ilupp_hip_kernel_names(const ilupp_precond *p)
{
    if (p && p->kind == KIND_LLT) {
        // an LL^T object: the factor kernel of its construction and -- once an apply has built them -- the sweeps of its factor pair
        const PackedSweep &pf = p->llt_diag_last ? p->pkL : p->pkLT, &pb = p->llt_diag_last ? p->pkLT : p->pkL;
        const char *fk = p->llt_diag_last ? (p->batch_built ? "k_ichol0_create_batch" : p->chol_static ? "k_ichol0_st" : "k_ichol0") : (p->icholt_grid ? "k_icholt_grid" : "k_icholt_df");
        static thread_local std::string names;
        names = fk;
        if (pf.valid && pf.pair && pb.valid && pb.pair) {
            const bool vec = pf.fmt == 1 && wx_vec_on() && pf.vec_ok && pb.vec_ok;
            if (pf.fmt == 1) names += std::string(vec ? ";k_sptrsv_wv<1, true>;k_sptrsv_wv" : ";k_sptrsv_wx<1, true>;k_sptrsv_wx") + (pb.desc ? "<-1, true, true>" : "<-1, true>");
            else names += std::string(";k_sptrsv_st<1, true>;k_sptrsv_st") + (pb.desc ? "<-1, true>" : "<-1, false>");
        }
        return names.c_str();
    }
    if (!p || !(p->kind == KIND_LU && p->nnz_mode == NNZ_GENERIC_LU && p->flm.built && p->flm.stat)) return "";
    static thread_local std::string lu_names;
    if (p->pkL.fmt >= 1) {
        const bool vec = wx_vec_on() && p->pkL.vec_ok && p->pkU.vec_ok;
        lu_names = std::string(p->flm.wxf ? wx_factor_kernel_name() : "k_ilu0_sd") +
                   (p->pkL.fmt == 2 ? ";k_sptrsv_wv<1, false, false, true>;k_sptrsv_wv<-1, true>"
                    : vec ? ";k_sptrsv_wv<1, false>;k_sptrsv_wv<-1, true>" : ";k_sptrsv_wx<1, false>;k_sptrsv_wx<-1, true>");
        return lu_names.c_str();
    }
    return p->flm.direct ? "k_ilu0_sd;k_sptrsv_st<1, false>;k_sptrsv_st<-1, false>" : "k_ilu0_st;k_sptrsv_st<1, false>;k_sptrsv_st<-1, false>";
}

static int apply_host(ilupp_precond *p, double *x, int64_t len, int transpose)
{
    API_TRY
    OR_RETURN(vector_args(p, len, p ? p->n : 0));
    return apply_staged(p->stream, &p->xdev, p->n, x,
                        [&](double *d) { return apply_dev(p, d, transpose); },
                        [&] { return finish_apply(p); });
    API_CATCH
}

int ilupp_hip_apply(ilupp_precond *p, double *x, int64_t len) { return apply_host(p, x, len, 0); }
int ilupp_hip_apply_trans(ilupp_precond *p, double *x, int64_t len) { return apply_host(p, x, len, 1); }

int64_t ilupp_hip_total_nnz(const ilupp_precond *p)
{
    if (!p) return 0;
    switch (p->nnz_mode) {
    case NNZ_ILUT: return p->Lc.nnz - p->n + p->Uc.nnz;    // preconditioner_implementation.h:1035-1039
    case NNZ_LLT: return p->Lc.nnz;                        // preconditioner.h:246-247
    default: return p->Lc.nnz + p->Uc.nnz;                 // preconditioner.h:208-209
    }
}
double ilupp_hip_memory_used_calculations(const ilupp_precond *) { return 0.0; }        // preconditioner.h:65
double ilupp_hip_memory_allocated_calculations(const ilupp_precond *) { return 0.0; }
double ilupp_hip_memory(const ilupp_precond *) { return 0.0; }                          // preconditioner.h:113
int ilupp_hip_exists(const ilupp_precond *p) { return p ? 1 : 0; }
const char *ilupp_hip_special_info(const ilupp_precond *) { return ""; }
int32_t ilupp_hip_dimension(const ilupp_precond *p) { return p ? p->n : 0; }

int ilupp_hip_num_factors(const ilupp_precond *p) { return p ? (p->kind == KIND_LLT ? 1 : 2) : 0; }

// which factor the caller sees as #which: CSR input -> [L, U] = [Lc, Uc];
// CSC input -> L.interchange(U) + relabel (ILU0.hpp:100-105) -> [Uc as csc, Lc as csc]
static const DevMat *exposed(const ilupp_precond *p, int which, bool *is_csr)
{
    if (!p || which < 0 || which >= ilupp_hip_num_factors(p)) return nullptr;
    if (p->kind == KIND_LLT) { *is_csr = p->Lc.is_csr; return &p->Lc; }
    if (p->kind == KIND_UTU) { *is_csr = which != 0; return which == 0 ? &p->Lc : &p->Uc; }     // binding.cpp:449-460: column-wise, row-wise
    if (!p->input_csc) { *is_csr = true; return which == 0 ? &p->Lc : &p->Uc; }
    *is_csr = false;
    return which == 0 ? &p->Uc : &p->Lc;
}

int ilupp_hip_factor_info(const ilupp_precond *p, int which, int32_t *rows, int32_t *cols, int64_t *nnz, int *is_csr)
{
    bool csr = true;
    const DevMat *M = exposed(p, which, &csr);
    if (!M) { set_error("no such factor"); return ILUPP_ERR_INVALID; }
    if (rows) *rows = p->n;
    if (cols) *cols = p->n;
    if (nnz) *nnz = M->nnz;
    if (is_csr) *is_csr = csr ? 1 : 0;
    return ILUPP_OK;
}

int ilupp_hip_factor_copy(const ilupp_precond *p, int which, double *data, int32_t *indices, int32_t *indptr)
{
    API_TRY
    bool csr = true;
    const DevMat *M = exposed(p, which, &csr);
    if (!M) { set_error("no such factor"); return ILUPP_ERR_INVALID; }
    ensure_csr_values(const_cast<ilupp_precond *>(p));
    ILUPP_HIP(stream_sync(p->stream));
    ILUPP_HIP(hipMemcpy(indptr, M->ptr, sizeof(int32_t) * (size_t)(p->n + 1), hipMemcpyDeviceToHost));
    if (M->nnz > 0) {
        ILUPP_HIP(hipMemcpy(indices, M->idx, sizeof(int32_t) * (size_t)M->nnz, hipMemcpyDeviceToHost));
        ILUPP_HIP(hipMemcpy(data, M->val, sizeof(double) * (size_t)M->nnz, hipMemcpyDeviceToHost));
    }
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_factor_device_ptrs(const ilupp_precond *p, int which, const double **d_data,
                                 const int32_t **d_indices, const int32_t **d_indptr)
{
    bool csr = true;
    const DevMat *M = exposed(p, which, &csr);
    if (!M) { set_error("no such factor"); return ILUPP_ERR_INVALID; }
    try { ensure_csr_values(const_cast<ilupp_precond *>(p)); } catch (const ilupp::HipError &e) { return ilupp::report(e); }
    if (d_data) *d_data = M->val;
    if (d_indices) *d_indices = M->idx;
    if (d_indptr) *d_indptr = M->ptr;
    return ILUPP_OK;
}

void ilupp_hip_print_info(const ilupp_precond *p)
{
    if (!p) return;
    // the reference prints both matrices in full (preconditioner_implementation.h:360-366); we print the summary
    printf("The left matrix of the preconditioner: %d x %d, nnz=%lld\n", p->n, p->n, (long long)p->Lc.nnz);
    if (p->kind != KIND_LLT)
        printf("The right matrix of the preconditioner: %d x %d, nnz=%lld\n", p->n, p->n, (long long)p->Uc.nnz);
}

int ilupp_hip_get_timings(const ilupp_precond *p, ilupp_timings *t)
{
    if (!p || !t) return ILUPP_ERR_INVALID;
    *t = p->tm;
    return ILUPP_OK;
}

int ilupp_hip_release_cached_memory(void)
{
    API_TRY
    plans().drop_all();                  // (first: the plans' blocks go to the pool, the pool's to the driver)
    pool_trim();
    { std::lock_guard<std::mutex> build_lock_(ilupp::g_build_mu); mwm_release_stage(); }
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_set_cache_limit(unsigned long long bytes)
{
    API_TRY
    // (the parked plans count against the limit with the pool's kept blocks; they leave first, the least recently parked first)
    const size_t kept = pool_cached_bytes();
    plans().shrink_to((size_t)bytes > kept ? (size_t)bytes - kept : 0);
    pool_set_limit((size_t)bytes);
    return ILUPP_OK;
    API_CATCH
}
// (a parked plan is cache: its bytes are cached bytes, its blocks -- which the pool has handed out -- are nobody's live blocks)
unsigned long long ilupp_hip_cached_bytes(void) { return (unsigned long long)(pool_cached_bytes() + plans().bytes()); }
unsigned long long ilupp_hip_live_blocks(void)
{
    const size_t live = pool_live_blocks(), parked = plans().blocks();
    return (unsigned long long)(live > parked ? live - parked : 0);
}
int ilupp_hip_plan_cache_stats(unsigned long long out[4])
{
    if (!out) return ILUPP_ERR_INVALID;
    const Plans::Stats s = plans().stats();
    out[0] = s.parked; out[1] = s.taken; out[2] = s.missed; out[3] = s.dropped;
    return ILUPP_OK;
}

int ilupp_hip_sync(ilupp_precond *p)
{
    API_TRY
    if (!p) return ILUPP_ERR_INVALID;
    return finish_apply(p);
    API_CATCH
}

}  // extern "C"

// ================================================================================================================================
// the multilevel ILU++ preconditioner without pivoting (include/ilupp_hip.h: ilupp_hip_ml_*).  Levels from ml.hip /
// piluc_df.hip; every level's two factors are an object of the ILUC kind (left by columns, right by rows, both unit), whose sweep
// kernels the apply borrows one half at a time: preconditioner_implementation.h:441-453 (left: all levels upwards) and :468-486
// (right: all levels downwards), each on the LAST n_level entries of the vector (sparse_implementation.h:4096-4165).
// ================================================================================================================================
// the live multilevel objects: a batched entry that is handed one in place of an ilupp_precond says so instead of reading it as one
static std::mutex g_ml_live_mu;
static std::set<const void *> g_ml_live;
static bool is_live_ml(const void *h) { std::lock_guard<std::mutex> lk(g_ml_live_mu); return g_ml_live.count(h) != 0; }

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

namespace {

void ml_destroy(ilupp_ml *m)
{
    if (!m) return;
    // (the first level owns the stream the others borrow: it goes last)
    for (size_t k = m->obj.size(); k-- > 0;) if (m->obj[k]) destroy_obj(m->obj[k]);
    for (auto &l : m->dev) l.release();
    if (m->buf) (void)pool_free(m->buf);
    if (m->xdev) (void)pool_free(m->xdev);
    delete m;
}

static bool getenv_small_off() { static const bool off = getenv("ILUPP_NO_SMALL_SWEEPS") != nullptr; return off; }

// one half of the ILUC-kind apply (apply_plan, KIND_UTU): forward = the T2 loop (left factor, or right^T), backward = the T3 loop
int utu_half(ilupp_precond *p, bool forward, bool tr, double *rhs, double *out, int32_t *ticket)
{
    ensure_transposed(p);
    int32_t *err = p->ctrl;
    const ApplyPlan plan = apply_plan(KIND_UTU, tr, false, false);
    const SweepOp op = forward ? plan.first : plan.second;
    // small levels (the later, denser ones): one workgroup with the unknowns in LDS instead of a chain of hops through memory
    // (not for a factor with an empty row: p->degenerate objects keep the row-by-row kernel, which reports what it meets)
    // (up to 1 024 rows always; up to kSmallSweepMax = 4 096 when the rows are long -- more than 32 entries on average: there the general
    //  kernels' hop through memory per link of the dependency chain costs most.  Measured, apply of a whole object: 26 levels from n = 2 000,
    //  177 entries per row: 65 against 176 ms; 3 375 rows with 6 entries per row: 0.82 against 0.68 ms -- hence the second condition)
    const DevMat &M = sweep_parts(p, op).M;
    if ((p->n <= 1024 || (p->n <= kSmallSweepMax && M.nnz > 32 * (int64_t)p->n)) && !p->degenerate && !getenv_small_off())
        return sptrsv_small(p->stream, op.kind, M, rhs, out, err);
    return sweep(p, op, packed(p, op), rhs, out, ticket, err);
}

int ml_apply_dev(ilupp_ml *m, double *x, int transpose, int part = 0)       // part: 0 = both passes, 1 = the first only, 2 = the second only
{
    ilupp_precond *p0 = m->obj[0];
    hipStream_t st = p0->stream;
    const int nl = (int)m->obj.size();
    // (a batched launch that was not waited for still reads the levels and writes m->buf: ilupp_hip_ml_apply_batch_device)
    if (p0->batch_ev) {
        ILUPP_HIP(hipStreamWaitEvent(st, p0->batch_ev, 0));
        for (int i = 0; i < nl; ++i) m->obj[(size_t)i]->batch_ev = nullptr;
    }
    order_after_caller(st, p0->sev[0]);
    for (int i = 0; i < nl; ++i) ILUPP_HIP(hipMemsetAsync(m->obj[(size_t)i]->ctrl, 0, 64, st));
    ILUPP_HIP(hipEventRecord(p0->ev[0], st));
    const bool tr = transpose != 0;
    // first pass upwards through the levels, second pass downwards (:103-111 with :441-453, :468-486)
    for (int pass = 0; pass < 2; ++pass) {
        if (part != 0 && part != pass + 1) continue;
        for (int s = 0; s < nl; ++s) {
            const int i = pass == 0 ? s : nl - 1 - s;
            ilupp_precond *p = m->obj[(size_t)i];
            const MlLevelDev &l = m->dev[(size_t)i];
            double *xt = x + (m->n - l.n);
            int rc = ILUPP_OK;
            if (!tr && pass == 0) {            // left, ID: x /= D_l; permute_first(perm_rows); T2(L)
                ml_scale_perm(st, l.n, xt, l.Dl, l.pr, m->buf);
                rc = utu_half(p, true, false, m->buf, p->work, p->ctrl + 4);
                if (!rc) ml_take(st, l.n, p->work, nullptr, xt);
            } else if (!tr) {                  // right, ID: x *= D; T3(U); permute_last(inverse_perm_columns); x /= D_r
                ml_scale(st, l.n, xt, l.D, m->buf);
                rc = utu_half(p, false, false, m->buf, p->work, p->ctrl + 5);
                if (!rc) {
                    ml_perm_scale(st, l.n, p->work, l.ipc, l.Dr, xt);
                    fill_u64(st, reinterpret_cast<unsigned long long *>(p->work), l.n, kSentinel);
                }
            } else if (pass == 0) {            // right, TRANSPOSE: x /= D_r; permute_first(perm_columns); T2(U^T); x *= D
                ml_scale_perm(st, l.n, xt, l.Dr, l.pc, m->buf);
                rc = utu_half(p, true, true, m->buf, p->work, p->ctrl + 4);
                if (!rc) ml_take(st, l.n, p->work, l.D, xt);
            } else {                           // left, TRANSPOSE: T3(L^T); permute_last(inverse_perm_rows); x /= D_l
                ILUPP_HIP(hipMemcpyAsync(m->buf, xt, sizeof(double) * (size_t)l.n, hipMemcpyDeviceToDevice, st));
                rc = utu_half(p, false, true, m->buf, p->work, p->ctrl + 5);
                if (!rc) {
                    ml_perm_scale(st, l.n, p->work, l.ipr, l.Dl, xt);
                    fill_u64(st, reinterpret_cast<unsigned long long *>(p->work), l.n, kSentinel);
                }
            }
            if (rc) return rc;
        }
    }
    ILUPP_HIP(hipEventRecord(p0->ev[2], st));
    return ILUPP_OK;
}

int ml_finish_apply(ilupp_ml *m)
{
    ilupp_precond *p0 = m->obj[0];
    const int nl = (int)m->obj.size();
    std::vector<int32_t> err((size_t)nl, 0);
    for (int i = 0; i < nl; ++i) ILUPP_HIP(hipMemcpyAsync(&err[(size_t)i], m->obj[(size_t)i]->ctrl, sizeof(int32_t), hipMemcpyDeviceToHost, p0->stream));
    ILUPP_HIP(stream_sync(p0->stream));
    ILUPP_HIP(hipEventElapsedTime(&m->last_apply_ms, p0->ev[0], p0->ev[2]));
    for (int i = 0; i < nl; ++i)
        if (err[(size_t)i]) {
            for (int j = 0; j < nl; ++j) fill_u64(p0->stream, reinterpret_cast<unsigned long long *>(m->obj[(size_t)j]->work), m->obj[(size_t)j]->n, kSentinel);
            ILUPP_HIP(stream_sync(p0->stream));
            set_error("triangular solve: dependency wait timed out (factor not triangular?)");
            return ILUPP_ERR_TIMEOUT;
        }
    return ILUPP_OK;
}

int ml_create_common(const DevMat &A, const ilupp_ml_params *ip, ilupp_ml **out)
{
    MlParams P;
    P.threshold = ip->threshold;
    P.n_pre = ip->n_preprocessing;
    if (P.n_pre < 0 || P.n_pre > 8) { set_error("ILU++: at most 8 preprocessing steps"); return ILUPP_ERR_INVALID; }
    for (int i = 0; i < P.n_pre; ++i) P.pre[i] = ip->preprocessing[i];
    P.pq_threshold = ip->pq_threshold; P.max_levels = ip->max_levels; P.min_ml_size = ip->min_ml_size;
    P.pil.small_pivot_terminates = ip->small_pivot_terminates != 0; P.pil.min_pivot = ip->min_pivot; P.pil.min_elim_factor = ip->min_elim_factor;
    P.pil.threshold_shift_schur = ip->threshold_shift_schur; P.vary_threshold_factor = ip->vary_threshold_factor;
    P.use_final_threshold = ip->use_final_threshold != 0; P.final_threshold = ip->final_threshold;
    P.pil.max_fill_in = ip->max_fill_in > 0 ? ip->max_fill_in : 0;
    P.pil.rules = ip->drop_rules; P.pil.combine = ip->combine_factor; P.pil.scale_invdiag = ip->scale_weight_invdiag != 0;
    P.pil.wgt[0] = ip->weight_standard_drop; P.pil.wgt[1] = ip->weight_standard_drop2; P.pil.wgt[2] = ip->weight_err_prop_drop;
    P.pil.wgt[3] = ip->weight_err_prop_drop2; P.pil.wgt[4] = ip->weight_pivot_drop; P.pil.wgt[5] = ip->weight_inverse_drop;
    P.pil.wgt[6] = ip->weight_weighted_drop; P.pil.init_weights_lu = ip->init_weights_lu;
    P.pil.neutral = ip->neutral_element; P.pil.min_weight = ip->min_weight;
    P.pil.piv_tol = ip->piv_tol; P.pil.permute_rows = ip->permute_rows; P.pil.total_piv = ip->total_piv; P.pil.begin_total_piv = ip->begin_total_piv != 0;
    P.pil.final_row_crit = ip->final_row_crit; P.pil.move_level_factor = ip->move_level_factor; P.pil.row_u_max = ip->row_u_max;
    if (P.pil.permute_rows < 0 || P.pil.permute_rows > 3 || P.pil.total_piv < 0 || P.pil.total_piv > 2) { set_error("ILU++: PERMUTE_ROWS / TOTAL_PIV out of range"); return ILUPP_ERR_INVALID; }
    if (P.pil.pivoting() && (P.pil.final_row_crit < -1 || P.pil.final_row_crit > 9)) {
        set_error("ILU++: FINAL_ROW_CRIT " + std::to_string(P.pil.final_row_crit) + " (rows ordered by weights instead of counts) is not built");
        return ILUPP_ERR_UNSUPPORTED;
    }
    if ((P.pil.rules & ~255) != 0) { set_error("ILU++: unknown dropping rule"); return ILUPP_ERR_INVALID; }
    // (inverse-based and weighted dropping -- recurrences over all steps -- run as chains in both factorisations: pilucdp.hip)
    struct MlGuard { ilupp_ml *m; ~MlGuard() { if (m) ml_destroy(m); } } g{new ilupp_ml()};
    ilupp_ml *m = g.m;
    m->n = A.n;
    // the first level's object owns the stream everything runs on
    ilupp_precond *p0 = new_obj(A.n);
    m->obj.push_back(p0);
    hipStream_t st = p0->stream;
    ILUPP_HIP(hipEventRecord(p0->ev[0], st));
    int rc = ml_build(st, A, P, &m->dev, &m->kernel_ms);
    if (rc) return rc;
    ILUPP_HIP(pool_malloc(&m->buf, sizeof(double) * (size_t)A.n));
    for (size_t k = 0; k < m->dev.size(); ++k) {
        MlLevelDev &l = m->dev[k];
        ilupp_precond *p = p0;
        if (k > 0) {
            p = new_obj(l.n);
            m->obj.push_back(p);
            queue_give(*p);                                    // its own queue back to the pool: the level works on the first level's
            static_cast<QueuePack &>(*p) = *p0;
            p->side = nullptr; p->jev[0] = p->jev[1] = nullptr;
            p->borrowed_queue = true;
        }
        p->kind = KIND_UTU; p->nnz_mode = NNZ_GENERIC_LU; p->input_csc = false;
        p->Lc = l.L; p->Uc = l.U;
        l.L = DevMat(); l.U = DevMat();                        // (the object owns the arrays now)
        utu_analyse(p);
    }
    ILUPP_HIP(hipEventRecord(p0->ev[1], st));
    ILUPP_HIP(stream_sync(st));
    ILUPP_HIP(hipEventElapsedTime(&m->construct_ms, p0->ev[0], p0->ev[1]));
    *out = m;
    g.m = nullptr;
    return ILUPP_OK;
}

}  // namespace

namespace ilupp {

// a batched construction that gets no stream to run on
static int no_batch_stream() { set_error("batched construction: no stream"); return ILUPP_ERR_HIP; }

// how a batched construction went, for every kind of batch: the members' codes into the caller's array, if it gave one, and the first
// failure returned and named by its number
static int batch_first_failure(int32_t count, const std::vector<int> &rcs, const std::vector<std::string> &msgs, int32_t *status)
{
    int first = ILUPP_OK;
    for (int32_t i = 0; i < count; ++i) {
        if (status) status[i] = rcs[(size_t)i];
        if (rcs[(size_t)i] && !first) { first = rcs[(size_t)i]; set_error("matrix " + std::to_string(i) + " of the batch: " + msgs[(size_t)i]); }
    }
    return first;
}

// The workers of a batched construction (ilupp_hip_ml_create_batch, ilupp_hip_ilucp_create_batch, ilupp_hip_ilutp_create_batch): `build(i)`
// constructs member i on the calling worker's thread and returns its code; `worst_bytes` is the device memory the largest member holds
// while it is built.  At most 64 workers (ILUPP_BATCH_WORKERS, read per call) and as many as the memory takes: 0.6 of the free bytes, the
// pool's kept blocks counted as free.  Every worker is a member of one ChainBatch, so the sequential chains of the members it builds are
// launched together with the other workers' (pilucdp.hip).  Members are independent: status[i] per member (may be null), the first
// failure is returned and reported as "matrix i of the batch: ...".  The caller holds the build lock.
int batch_build(int32_t count, double worst_bytes, int32_t *status, const std::function<int(int32_t)> &build)
{
    int workers = 64;
    if (const char *e = getenv("ILUPP_BATCH_WORKERS")) { const int v = atoi(e); if (v > 0) workers = v; }
    if (workers > count) workers = count;
    int device = 0;
    ILUPP_HIP(hipGetDevice(&device));
    {
        size_t free_b = 0, total_b = 0;
        ILUPP_HIP(hipMemGetInfo(&free_b, &total_b));
        free_b += pool_cached_bytes();
        if (worst_bytes > 0.0) { const double fit = 0.6 * (double)free_b / worst_bytes; if (fit < (double)workers) workers = fit < 1.0 ? 1 : (int)fit; }
    }
    ChainBatch *cb = chain_batch_create(workers);
    if (!cb) return no_batch_stream();
    // (the batch and its stream go when this call unwinds, whatever throws below)
    struct BatchGuard { ChainBatch *b; ~BatchGuard() { if (b) chain_batch_destroy(b); } } cbg{cb};
    std::vector<int> rcs((size_t)count, ILUPP_OK);
    std::vector<std::string> msgs((size_t)count);
    std::atomic<int32_t> next(0);
    auto work = [&](int w) {
        (void)hipSetDevice(device);
        pool_set_owner(w + 1);
        chain_batch_enter(cb);
        for (;;) {
            const int32_t i = next.fetch_add(1);
            if (i >= count) break;
            int rc;
            try { rc = build(i); }
            catch (const ilupp::HipError &e) { ilupp::d2h_cancel_all(); rc = ilupp::report(e); }
            catch (const std::bad_alloc &) { ilupp::set_error("out of host memory"); rc = ILUPP_ERR_MEMORY; }
            catch (...) { ilupp::set_error("unexpected exception in a batch worker"); rc = ILUPP_ERR_HIP; }     // (a worker must reach chain_batch_leave)
            rcs[(size_t)i] = rc;
            if (rc) msgs[(size_t)i] = ilupp::g_last_error;
        }
        chain_batch_leave(cb);
        (void)hipDeviceSynchronize();                          // (everything this worker queued is done: its kept blocks are everybody's)
        pool_disown(w + 1);
        pool_set_owner(0);
    };
    // Kept blocks of owner 0 may have been given back by calls on other objects' streams (apply temporaries, destroy) without a wait for
    // those streams: nothing of that may still be queued when up to 64 fresh streams start to take such blocks (pool.h).
    ILUPP_HIP(hipDeviceSynchronize());
    {
        // (threads that were started are joined whatever happens -- a joinable std::thread that is destroyed ends the process --, and
        // workers that could not be started are taken out of the batch's count, or the others would wait for their launches for good)
        struct Joiner { std::vector<std::thread> v; ~Joiner() { for (std::thread &t : v) if (t.joinable()) t.join(); } } pool_threads;
        int started = 1;
        try {
            for (int w = 1; w < workers; ++w) { pool_threads.v.emplace_back(work, w); ++started; }
        } catch (...) {
            for (int w = started; w < workers; ++w) { chain_batch_enter(cb); chain_batch_leave(cb); }
        }
        work(0);
    }
    chain_batch_destroy(cbg.b); cbg.b = nullptr;
    return batch_first_failure(count, rcs, msgs, status);
}

}  // namespace ilupp

extern "C" {

void ilupp_hip_ml_default_params(ilupp_ml_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 0.0;
    p->n_preprocessing = 3;
    p->preprocessing[0] = ILUPP_PRE_NORMALIZE_COLUMNS; p->preprocessing[1] = ILUPP_PRE_NORMALIZE_ROWS; p->preprocessing[2] = ILUPP_PRE_PQ_ORDERING;
    p->pq_threshold = 0.0; p->max_levels = 100; p->min_ml_size = 0;
    p->small_pivot_terminates = 1; p->min_pivot = 1e-2; p->min_elim_factor = 0.0; p->threshold_shift_schur = 0.0;
    p->vary_threshold_factor = 1.0; p->use_final_threshold = 0; p->final_threshold = 0.0;
    p->max_fill_in = 0;
    p->drop_rules = ILUPP_DROP_ERR_PROP;
    p->weight_standard_drop = p->weight_standard_drop2 = p->weight_err_prop_drop = p->weight_err_prop_drop2 = p->weight_pivot_drop = 1.0;
    p->weight_inverse_drop = 1.0; p->weight_weighted_drop = 1.0; p->init_weights_lu = 1.0;
    p->combine_factor = 0; p->neutral_element = 0.0; p->min_weight = 1.0; p->scale_weight_invdiag = 0;
    p->piv_tol = 0.0; p->permute_rows = 0; p->total_piv = 0; p->begin_total_piv = 1;        // (init case 10, :927-934)
    p->final_row_crit = -1; p->move_level_factor = 2.0; p->row_u_max = 1.5;
}

int ilupp_hip_ml_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const ilupp_ml_params *params,
                        ilupp_ml **out)
{
    return create_from_host(data, indices, indptr, n, is_csr != 0, out, [&](DevMat &A) { return ml_create_common(A, params, out); },
                            params != nullptr, "null argument");
}

int ilupp_hip_ml_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr, const int32_t *n,
                              int is_csr, const ilupp_ml_params *params, ilupp_ml **out, int32_t *status)
{
    API_TRY_BUILD
    if (count < 0 || !data || !indices || !indptr || !n || !params || !out) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) { out[i] = nullptr; if (status) status[i] = ILUPP_OK; }
    if (count == 0) return ILUPP_OK;
    // a construction with pivoting holds ~116 bytes per entry + 450 per row (two stores with their link arrays, the Schur store, both
    // orientations of the level's matrix, the tables)
    double worst = 0.0;
    for (int32_t i = 0; i < count; ++i)
        if (indptr[i] && n[i] > 0) { const double e = 116.0 * (double)indptr[i][n[i]] + 450.0 * (double)n[i] + (double)(64 << 20); if (e > worst) worst = e; }
    return batch_build(count, worst, status, [&](int32_t i) {
        MatGuard A;
        const int rc = upload(data[i], indices[i], indptr[i], n[i], is_csr != 0, &A.m);
        return rc ? rc : ml_create_common(A.m, params, &out[i]);
    });
    API_CATCH
}

int ilupp_hip_ml_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int is_csr,
                               const ilupp_ml_params *params, ilupp_ml **out)
{
    return create_from_device(d_data, d_indices, d_indptr, n, is_csr != 0, out, [&](DevMat &A) { return ml_create_common(A, params, out); },
                              params != nullptr, "null argument");
}

void ilupp_hip_ml_destroy(ilupp_ml *p)
{
    try { ml_destroy(p); } catch (...) {}
}

int ilupp_hip_ml_apply_device(ilupp_ml *m, double *d_x, int64_t len, int transpose, int sync)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    OR_RETURN(ml_apply_dev(m, d_x, transpose));
    return finish_or_hand_over(sync, *m->obj[0], [&] { return ml_finish_apply(m); });
    API_CATCH
}

int ilupp_hip_ml_apply_part_device(ilupp_ml *m, double *d_x, int64_t len, int transpose, int left, int sync)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    // ID: the left part is the first pass (upwards through the levels), the right part the second; TRANSPOSE: right^T first, then left^T
    const int part = (left != 0) == (transpose == 0) ? 1 : 2;
    OR_RETURN(ml_apply_dev(m, d_x, transpose, part));
    return finish_or_hand_over(sync, *m->obj[0], [&] { return ml_finish_apply(m); });
    API_CATCH
}

int ilupp_hip_ml_apply(ilupp_ml *m, double *x, int64_t len, int transpose)
{
    API_TRY
    OR_RETURN(vector_args(m, len, m ? m->n : 0));
    return apply_staged(m->obj[0]->stream, &m->xdev, m->n, x,
                        [&](double *d) { return ml_apply_dev(m, d, transpose); },
                        [&] { return ml_finish_apply(m); });
    API_CATCH
}

namespace {
// the matrix of a solve in HBM and its preconditioner (the caller holds the construction lock)
int solve_build(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const ilupp_ml_params *params, DevMat *A,
                ilupp_ml **m)
{
    API_TRY
    const int rc = upload(data, indices, indptr, n, is_csr != 0, A);
    if (rc) return rc;
    return ml_create_common(*A, params, m);
    API_CATCH
}
}  // namespace

int ilupp_hip_solve(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const double *rhs, int64_t rhs_len,
                    double rtol, double atol, int32_t max_iter, const ilupp_ml_params *params, double *x, int32_t *iterations, double *rel_reached,
                    double *abs_reached)
{
    if (!data || !indices || !indptr || !rhs || !params || !x) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    if (n <= 0) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
    if (rhs_len != n) { set_error("right-hand side has wrong size!"); return ILUPP_ERR_WRONG_SIZE; }            // binding.cpp:209-210
    // (the whole call under the construction lock: the iteration takes and returns pool blocks on its own stream, and the pool knows nothing
    //  of streams -- see API_TRY_BUILD)
    std::lock_guard<std::mutex> build_lock_(ilupp::g_build_mu);
    struct Guard {
        DevMat A, T; ilupp_ml *m = nullptr;
        ~Guard() { try { if (m) { (void)hipStreamSynchronize(m->obj[0]->stream); ml_destroy(m); } } catch (...) {} A.release(); T.release(); }
    } g;
    { const int rc = solve_build(data, indices, indptr, n, is_csr, params, &g.A, &g.m); if (rc) return rc; }
    API_TRY
    ilupp_ml *m = g.m;
    hipStream_t st = m->obj[0]->stream;
    const DevMat *R = &g.A;                                    // the rows of A, for the products
    if (!g.A.is_csr) { transpose_storage(st, g.A, &g.T); R = &g.T; }
    PoolBlock b_r, b_y, b_t;
    for (PoolBlock *b : {&b_r, &b_y, &b_t}) ILUPP_HIP(b->alloc(sizeof(double) * (size_t)n));
    struct SyncOnExit { hipStream_t st; ~SyncOnExit() { (void)hipStreamSynchronize(st); } } quiesce{st};      // (before the blocks go back)
    double *r = b_r.as<double>(), *y = b_y.as<double>(), *tmp = b_t.as<double>();
    ILUPP_HIP(hipMemcpyAsync(r, rhs, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    { const int rc = ml_apply_dev(m, r, 0, 1); if (rc) return rc; }                                              // r = L' b (preconditioned_rhs)
    auto op = [&](const double *in, double *out) -> int {       // out = L'(A(R' in))
        ILUPP_HIP(hipMemcpyAsync(tmp, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        int rc = ml_apply_dev(m, tmp, 0, 2);
        if (rc) return rc;
        rc = ilupp_hip_spmv_device(R->val, R->idx, R->ptr, n, R->nnz, tmp, out, st);
        if (rc) return rc;
        return ml_apply_dev(m, out, 0, 1);
    };
    int32_t it = 0; double rel = 0.0, res = 0.0;
    { const int rc = bicgstab_split(st, n, op, r, y, 1, max_iter, rtol, atol, &it, &rel, &res); if (rc) return rc; }
    { const int rc = ml_apply_dev(m, y, 0, 2); if (rc) return rc; }                                              // x = R' y (adapt_solution)
    { const int rc = ml_finish_apply(m); if (rc) return rc; }
    ILUPP_HIP(hipMemcpy(x, y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (iterations) *iterations = it;
    if (rel_reached) *rel_reached = rel;
    if (abs_reached) *abs_reached = res;
    if (!(rel < rtol && res < atol)) { set_error("did not converge"); return ILUPP_ERR_NOT_CONVERGED; }         // iterative_solvers_implementation.h:497
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_ml_sync(ilupp_ml *m)
{
    API_TRY
    if (!m) return ILUPP_ERR_INVALID;
    return ml_finish_apply(m);
    API_CATCH
}

int32_t ilupp_hip_ml_levels(const ilupp_ml *m) { return m ? (int32_t)m->obj.size() : 0; }

int64_t ilupp_hip_ml_total_nnz(const ilupp_ml *m)          // preconditioner.h:312 with preconditioner_implementation.h:551-569
{
    if (!m) return 0;
    int64_t sum = 0;
    for (const ilupp_precond *p : m->obj) sum += (p->Lc.nnz - p->n) + (p->Uc.nnz - p->n) + p->n;
    return sum;
}

int ilupp_hip_ml_level_info(const ilupp_ml *m, int32_t level, int32_t *n, int64_t *nnz_left, int64_t *nnz_right)
{
    if (!m || level < 0 || level >= (int32_t)m->obj.size()) { set_error("no such level"); return ILUPP_ERR_INVALID; }
    const ilupp_precond *p = m->obj[(size_t)level];
    if (n) *n = p->n;
    if (nnz_left) *nnz_left = p->Lc.nnz;
    if (nnz_right) *nnz_right = p->Uc.nnz;
    return ILUPP_OK;
}

int ilupp_hip_ml_level_copy(const ilupp_ml *m, int32_t level, double *l_data, int32_t *l_indices, int32_t *l_indptr, double *u_data, int32_t *u_indices,
                            int32_t *u_indptr, double *middle, int32_t *perm_rows, int32_t *perm_cols, int32_t *inv_perm_rows, int32_t *inv_perm_cols,
                            double *d_left, double *d_right)
{
    API_TRY
    if (!m || level < 0 || level >= (int32_t)m->obj.size()) { set_error("no such level"); return ILUPP_ERR_INVALID; }
    const ilupp_precond *p = m->obj[(size_t)level];
    const MlLevelDev &l = m->dev[(size_t)level];
    ILUPP_HIP(stream_sync(p->stream));
    const size_t n = (size_t)p->n;
    get_host(l_data, p->Lc.val, sizeof(double) * (size_t)p->Lc.nnz); get_host(l_indices, p->Lc.idx, sizeof(int32_t) * (size_t)p->Lc.nnz); get_host(l_indptr, p->Lc.ptr, sizeof(int32_t) * (n + 1));
    get_host(u_data, p->Uc.val, sizeof(double) * (size_t)p->Uc.nnz); get_host(u_indices, p->Uc.idx, sizeof(int32_t) * (size_t)p->Uc.nnz); get_host(u_indptr, p->Uc.ptr, sizeof(int32_t) * (n + 1));
    get_host(middle, l.D, sizeof(double) * n);
    get_host(perm_rows, l.pr, sizeof(int32_t) * n); get_host(perm_cols, l.pc, sizeof(int32_t) * n);
    get_host(inv_perm_rows, l.ipr, sizeof(int32_t) * n); get_host(inv_perm_cols, l.ipc, sizeof(int32_t) * n);
    get_host(d_left, l.Dl, sizeof(double) * n); get_host(d_right, l.Dr, sizeof(double) * n);
    return ILUPP_OK;
    API_CATCH
}

int ilupp_hip_ml_timings(const ilupp_ml *m, float *construct_ms, float *kernel_ms, float *last_apply_ms)
{
    if (!m) return ILUPP_ERR_INVALID;
    if (construct_ms) *construct_ms = m->construct_ms;
    if (kernel_ms) *kernel_ms = m->kernel_ms;
    if (last_apply_ms) *last_apply_ms = m->last_apply_ms;
    return ILUPP_OK;
}

}  // extern "C"

// ---- many members applied at once: one launch, one workgroup per member (k_pivot_apply_batch, sptrsv_batch.hip) ----
namespace {

// One array of the batched entries' scratch: `cap` elements on the device (d) and, where the instance is pinned, as many in page-locked
// host memory (h), with the event that says the last upload from there is over (never recorded: over).  It only grows, and is never
// smaller than its floor: the descriptor tables start at 64 entries, the staging blocks take exactly what is asked for.
template <class T>
struct BatchBuf {
    const size_t floor;
    const bool pinned;
    T *d = nullptr, *h = nullptr;
    size_t cap = 0;
    size_t used = 0;              // batch_upload's cache: so many entries of h are on the device as they stand there (0 = none)
    hipEvent_t up = nullptr;
    BatchBuf(size_t floor_, bool pinned_) : floor(floor_), pinned(pinned_) {}
    // Room for `want` elements.  true: the arrays are new ones and what the old ones held is gone.  Work queued on `st` may still read
    // the old ones, hence the wait before they are freed.  A growth that throws leaves cap == 0 and each pointer either null or
    // allocated: nothing is reached through a buffer without capacity, and the next call frees what is there and starts over.
    bool reserve(hipStream_t st, size_t want)
    {
        if (want <= cap) return false;
        if (d) ILUPP_HIP(hipStreamSynchronize(st));
        cap = 0;
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        if (pinned && !up) ILUPP_HIP(hipEventCreateWithFlags(&up, hipEventDisableTiming));
        const size_t n = want < floor ? floor : want;
        ILUPP_HIP(hipMalloc(reinterpret_cast<void **>(&d), sizeof(T) * n));
        if (pinned) ILUPP_HIP(hipHostMalloc(reinterpret_cast<void **>(&h), sizeof(T) * n, hipHostMallocDefault));
        cap = n;
        return true;
    }
};

// `fresh` (at least one entry) into B's pinned copy and from there to the device, on `st`.  cached: nothing is sent when the count and
// the bytes are those the device holds already -- the same members with the same buffers, call after call -- and what is sent is
// remembered.  Not cached: always sent and nothing remembered (a table nobody describes a second time).
template <class T>
void batch_upload(hipStream_t st, BatchBuf<T> &B, const std::vector<T> &fresh, bool cached = true)
{
    const size_t nl = fresh.size(), bytes = sizeof(T) * nl;
    if (B.reserve(st, nl)) B.used = 0;
    if (cached && nl == B.used && memcmp(B.h, fresh.data(), bytes) == 0) return;
    ILUPP_HIP(hipEventSynchronize(B.up));                               // (the upload before this one has read the pinned copy: long over)
    B.used = 0;
    memcpy(B.h, fresh.data(), bytes);
    ILUPP_HIP(hipMemcpyAsync(B.d, B.h, bytes, hipMemcpyHostToDevice, st));
    ILUPP_HIP(hipEventRecord(B.up, st));
    if (cached) B.used = nl;
}

// What the batched entries keep from call to call, one per device: a stream, the events that order it, what the last describing pass
// left, and the arrays that grow with the largest call so far.
struct BatchScratch {
    hipStream_t stream = nullptr;
    hipEvent_t cev[2] = {nullptr, nullptr};       // ordering against the caller's stream
    hipEvent_t in_ev = nullptr, done_ev = nullptr;      // the staged vectors are there; the launch is over
    hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};      // around the two launches of a batched construction (timed; made there)
    std::vector<PivotApplyDesc> fresh;            // the descriptors of the launch
    std::vector<int32_t> launched, route, h_err, status;      // member of workgroup k; per member: route, error word, code
    BatchBuf<PivotApplyDesc> table{64, true};     // the descriptors of an apply or a solve, cached: another member list, direction or vector layout uploads
    BatchBuf<int32_t> err{64, false};             // ... and the error word of each
    BatchBuf<PivotSolveDesc> sys{64, true};       // a solve's second table (the members' matrices), sent with every call
    BatchBuf<double> tmp{0, false};               // the hand-over vectors (`tmp`) of a launch's non-pivoting members, one block: n doubles each
    BatchBuf<double> stage{0, true};              // the host entries' packed block: the vectors of an apply, the matrices of a construction
    // the descriptors of an ILU(0) re-factorisation or construction, cached apart from `table`: the apply's cache still hits after a re-factorisation
    BatchBuf<RefactorDesc> rtable{64, true};
    BatchBuf<CreateInfo> cinfo{64, true};         // a construction's symbolic records, read back through the pinned copy
    BatchBuf<int32_t> cstat{64, false};           // ... and the status words of its create launch
    // a batched ILUT construction: the members' descriptors, the ticket maps of its rows launches (segments, then the member order) and the
    // members' records, read back through the pinned copy
    BatchBuf<IlutBatchDesc> ttable{64, true};
    BatchBuf<int32_t> ttick{512, true};
    BatchBuf<IlutBatchInfo> tinfo{64, true};
    // the two tables of a batched multilevel apply (member records, and the level records of all of them), each cached on its own
    BatchBuf<MlApplyDesc> mltable{64, true};
    BatchBuf<MlLevelDesc> mllevels{64, true};
    std::vector<MlApplyDesc> mfresh;              // the member records of a multilevel apply's launch (S.fresh stays empty there)
    // the level records of a launch's multilevel members (one table, uploaded through mllevels) and, per workgroup of a solve's launch, where
    // its member's records start there (-1: not a multilevel member)
    std::vector<MlLevelDesc> lfresh;
    std::vector<int32_t> ml_first;
};

// One member as the batched kernels see it, whatever class it comes from: the object that holds the two triangles, the pivoting
// permutation (or none) and the side it stands on, and the n doubles the one-array path hands its first sweep's result over in.  A
// pivoting member brings its own tmp and is ordered through its owner's batch_ev; a non-pivoting one (owner == nullptr) gets a slice of
// the scratch's block, which only launches on the scratch's stream ever touch, and is ordered through p->batch_ev.  p == nullptr: a
// member without a preconditioner (the CG solve only).  ml: a multilevel member, of the batched apply or the BiCGstab solve (p stays null:
// its levels are objects of their own, described from what ml_apply_dev reads, ordered through every level's batch_ev, its scratch the
// object's own buf).
struct BatchMember {
    ilupp_precond *p = nullptr;
    ilupp_ilucp *owner = nullptr;
    ilupp_ml *ml = nullptr;
    const int32_t *perm = nullptr;
    bool plain_first = true;
    double *tmp = nullptr;
    int32_t n = 0;
    hipEvent_t *batch_ev() const { return owner ? &owner->batch_ev : p ? &p->batch_ev : nullptr; }
};
BatchMember batch_member(ilupp_ilucp *m, int transpose)
{
    BatchMember v;
    v.p = m->obj; v.owner = m; v.perm = m->perm; v.plain_first = pivot_plain_first(m, transpose); v.tmp = m->tmp; v.n = m->n;
    return v;
}
BatchMember batch_member(ilupp_precond *p, int transpose)
{
    BatchMember v;
    v.p = p; v.plain_first = transpose == 0; v.n = p->n;
    return v;
}
BatchMember batch_member(ilupp_ml *m, int transpose)
{
    BatchMember v;
    v.ml = m; v.plain_first = transpose == 0; v.n = m->n;
    return v;
}
// the object whose stream a member's own work is queued on (a multilevel member: the first level's, which the others borrow)
ilupp_precond *batch_stream_obj(const BatchMember &v) { return v.ml ? v.ml->obj[0] : v.p; }
// a launch that reads the member is recorded in `ev` (nullptr: it has been waited for)
void batch_mark(const BatchMember &v, hipEvent_t ev)
{
    if (v.ml) { for (ilupp_precond *p : v.ml->obj) p->batch_ev = ev; return; }
    if (hipEvent_t *slot = v.batch_ev()) *slot = ev;
}
template <class Handle>
std::vector<BatchMember> batch_members(int32_t count, Handle *const *members, int transpose)
{
    std::vector<BatchMember> v((size_t)count);
    for (int32_t i = 0; i < count; ++i) v[(size_t)i] = batch_member(members[i], transpose);
    return v;
}
std::mutex g_batch_mu;
std::map<int, BatchScratch> g_batch_scratch;

BatchScratch &batch_scratch()
{
    int dev = 0;
    ILUPP_HIP(hipGetDevice(&dev));
    BatchScratch &S = g_batch_scratch[dev];
    if (!S.done_ev) {
        if (!S.stream) ILUPP_HIP(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
        for (hipEvent_t *e : {&S.cev[0], &S.cev[1], &S.in_ev, &S.done_ev})       // (done_ev comes last: a scratch that has it is complete)
            if (!*e) ILUPP_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return S;
}

// ILUPP_BATCH_APPLY_MAX_N lowers the n up to which a member goes to a launch (read per call)
int64_t batch_env_cap(int64_t cap_n)
{
    if (const char *e = getenv("ILUPP_BATCH_APPLY_MAX_N")) { const long long v = atoll(e); if (v >= 0 && v < cap_n) cap_n = v; }
    return cap_n;
}

// n up to which a member goes to the apply's launch: 8 n bytes of LDS must fit
int64_t batch_apply_max_n() { return batch_env_cap((int64_t)(pivot_apply_batch_lds_cap() / 8)); }

// ... a multilevel member to the apply's launch (k_ml_apply_batch): the 8 n bytes of LDS its first level's sweeps take must fit
int64_t ml_apply_batch_cap_n() { return batch_env_cap((int64_t)(ml_apply_batch_lds_cap() / 8)); }

// ... to a solver's launch: the cap of the apply's launch, lowered by what the dot scratch takes
// (ml: the launch of k_bicgstab_batch<true>, which a batch with a multilevel member runs: that instantiation's own cap)
int64_t solve_batch_cap_n(BatchSolver solver, bool ml = false)
{
    const int64_t a = batch_apply_max_n(), b = solve_batch_max_n(solver, ml);
    return a < b ? a : b;
}

// ... to the re-factorisation's and the construction's launches: one flag word per row of LDS
int64_t refactor_batch_max_n() { return batch_env_cap(ilu0_refactor_batch_max_n()); }

// the scratch's stream behind whatever is still queued on a member's own stream (a single apply or factors() that was not waited for,
// the transposed storages of a first use)
void batch_join(hipStream_t bs, ilupp_precond *p)
{
    if (!p || hipStreamQuery(p->stream) == hipSuccess) return;
    (void)hipGetLastError();
    ILUPP_HIP(hipEventRecord(p->sev[1], p->stream));
    ILUPP_HIP(hipStreamWaitEvent(bs, p->sev[1], 0));
}

// the routes of a call into the caller's array, if it gave one
void routes_out(const std::vector<int32_t> &from, int32_t *route)
{
    if (route) std::copy(from.begin(), from.end(), route);
}

// One record per level of a multilevel member, appended to `out`, from what ml_apply_dev reads: apply_plan(KIND_UTU, ...) and
// sweep_parts on the level's object for the two halves (the caller has run ensure_transposed on every level, as utu_half does), the
// level's diagonals and the two index arrays of the direction.
void ml_level_records(ilupp_ml *m, bool tr, std::vector<MlLevelDesc> *out)
{
    const ApplyPlan plan = apply_plan(KIND_UTU, tr, false, false);
    for (size_t k = 0; k < m->obj.size(); ++k) {
        const MlLevelDev &l = m->dev[k];
        const DevMat &M1 = sweep_parts(m->obj[k], plan.first).M, &M2 = sweep_parts(m->obj[k], plan.second).M;
        MlLevelDesc e;
        memset(&e, 0, sizeof(e));
        e.n = l.n; e.kind1 = plan.first.kind; e.kind2 = plan.second.kind;
        e.ptr1 = M1.ptr; e.idx1 = M1.idx; e.val1 = M1.val;
        e.ptr2 = M2.ptr; e.idx2 = M2.idx; e.val2 = M2.val;
        e.D = l.D; e.Dl = l.Dl; e.Dr = l.Dr;
        e.gather = tr ? l.pc : l.pr; e.take = tr ? l.ipr : l.ipc;
        out->push_back(e);
    }
}

// ... of a member whose levels are made ready first (ensure_transposed on every level, as utu_half does); false, and nothing appended,
// when a level object is degenerate
bool ml_member_records(ilupp_ml *m, bool tr, std::vector<MlLevelDesc> *out)
{
    bool degenerate = false;
    for (ilupp_precond *p : m->obj) { ensure_transposed(p); degenerate = degenerate || p->degenerate; }
    if (degenerate) return false;
    ml_level_records(m, tr, out);
    return true;
}

// Route and describe the members of a batched launch: route 0 = the launch (n <= cap_n, object not degenerate), 1 = too large, 2 = degenerate.
// S.fresh / S.launched receive the descriptors and member numbers of route 0, from the tables the single apply uses (apply_plan,
// sweep_parts); xoff = offsets[i].  A pivoting member is prepared as its single apply prepares it (prepare_apply).  A non-pivoting one
// needs only the two CSR triangles with their values (ensure_csr_values: a static-form ILU(0) leaves them unwritten; ensure_transposed
// when the plan reads slot 2 or 3): one whose single apply would take a static form goes to the launch all the same -- every route has
// the reference's bits -- and no static analysis runs merely to describe it.  Its tmp is a slice of the scratch's block (batch_tmp).
// take_ml == false: the launch is one without multilevel members -- they stay out of it whatever their n (route 1; the caller knows better).
void batch_describe(BatchScratch &S, int32_t count, const BatchMember *members, const int64_t *offsets, int64_t cap_n, bool take_ml = true)
{
    S.route.assign((size_t)count, 0); S.status.assign((size_t)count, ILUPP_OK); S.h_err.assign((size_t)count, 0);
    S.launched.clear(); S.fresh.clear(); S.lfresh.clear(); S.ml_first.clear();
    for (int32_t i = 0; i < count; ++i) {
        const BatchMember &v = members[i];
        ilupp_precond *p = v.p;
        if (v.n > cap_n || (v.ml && !take_ml)) { S.route[(size_t)i] = 1; continue; }
        PivotApplyDesc d;
        memset(&d, 0, sizeof(d));
        d.n = v.n; d.xoff = offsets[i];
        int32_t ml_first = -1;
        if (v.ml) {
            // a multilevel member (k_bicgstab_batch<true>): plain_first == 2, kind1 levels from ptr1 (set by batch_stage, when the level
            // table's place on the device is known), kind2 the direction, tmp the object's own scratch
            ml_first = (int32_t)S.lfresh.size();
            if (!ml_member_records(v.ml, !v.plain_first, &S.lfresh)) { S.route[(size_t)i] = 2; continue; }
            d.plain_first = 2; d.kind1 = (int32_t)v.ml->obj.size(); d.kind2 = v.plain_first ? 0 : 1; d.tmp = v.ml->buf;
        } else if (p) {
            const ApplyPlan plan = apply_plan(p, v.plain_first ? 0 : 1);
            if (v.owner) {
                PackedSweep *pf = nullptr, *pb = nullptr;
                if (prepare_apply(p, plan, &pf, &pb) != ROUTE_SWEEPS || p->degenerate) { S.route[(size_t)i] = 2; continue; }
            } else {
                ensure_csr_values(p);
                if (plan.transposed()) ensure_transposed(p);
                if (p->degenerate) { S.route[(size_t)i] = 2; continue; }
            }
            const DevMat &M1 = sweep_parts(p, plan.first).M, &M2 = sweep_parts(p, plan.second).M;
            d.kind1 = plan.first.kind; d.kind2 = plan.second.kind; d.plain_first = v.plain_first ? 1 : 0;
            d.ptr1 = M1.ptr; d.idx1 = M1.idx; d.val1 = M1.val;
            d.ptr2 = M2.ptr; d.idx2 = M2.idx; d.val2 = M2.val;
            d.perm = v.perm; d.tmp = v.tmp;
        }
        S.fresh.push_back(d);
        S.launched.push_back(i);
        S.ml_first.push_back(ml_first);
    }
}

// the hand-over vectors of the launch's non-pivoting members: slices of one block of the scratch, in the order of the launch
void batch_tmp(BatchScratch &S, const BatchMember *members)
{
    size_t total = 0;
    for (int32_t i : S.launched) if (members[i].p && !members[i].owner) total += (size_t)members[i].n;
    S.tmp.reserve(S.stream, total);
    size_t at = 0;
    for (size_t k = 0; k < S.launched.size(); ++k) {
        const BatchMember &v = members[S.launched[k]];
        if (v.p && !v.owner) { S.fresh[k].tmp = S.tmp.d + at; at += (size_t)v.n; }
    }
}

// The described members (at least one) made ready for their launch on the scratch's stream: the bytes of LDS the sweeps of the launch take
// (returned), the error words, the descriptor table on the device (uploaded again only when a descriptor differs), and the stream behind
// whatever is still queued on a member's own stream.
size_t batch_stage(BatchScratch &S, const BatchMember *members, int64_t cap_n)
{
    hipStream_t bs = S.stream;
    batch_tmp(S, members);
    // both arrays in LDS where 16 n bytes fit under the cap, else one: the launch takes what its largest member needs
    size_t lds = 0;
    const size_t cap_bytes = (size_t)cap_n * 8;
    for (const PivotApplyDesc &d : S.fresh) {
        const size_t two = (size_t)16 * (size_t)d.n, want = two <= cap_bytes ? two : (size_t)8 * (size_t)d.n;
        if (want > lds) lds = want;
    }
    // (the kernel makes the same choice per member from the launch's size: 16 n <= lds exactly when 16 n <= the cap)
    S.err.reserve(bs, S.fresh.size());
    for (size_t k = 0; k < S.fresh.size(); ++k) S.fresh[k].err = S.err.d + k;
    if (!S.lfresh.empty()) {
        // (the level table first: a multilevel member's descriptor points into it)
        if (S.mllevels.reserve(bs, S.lfresh.size())) S.mllevels.used = 0;
        for (size_t k = 0; k < S.fresh.size(); ++k)
            if (S.ml_first[k] >= 0) S.fresh[k].ptr1 = reinterpret_cast<const int32_t *>(S.mllevels.d + S.ml_first[k]);
        batch_upload(bs, S.mllevels, S.lfresh);
    }
    batch_upload(bs, S.table, S.fresh);
    for (int32_t i : S.launched) batch_join(bs, batch_stream_obj(members[i]));
    return lds;
}

// behind the launch: what touches a member's tmp or rewrites its factors comes after it (a pivoting member's later single apply, any
// member's re-factorisation and destruction)
void batch_launched(BatchScratch &S, const BatchMember *members)
{
    ILUPP_HIP(hipEventRecord(S.done_ev, S.stream));
    for (int32_t i : S.launched) batch_mark(members[i], S.done_ev);
}

// The second table of a batched solve on the device: for every launched member (at least one) its matrix, its own words of the per-member
// outputs and where its `wf` vectors of n start in the workspace -- member i's behind those of the members before it, launched or not.
void batch_systems(BatchScratch &S, int32_t count, const BatchMember *members, int64_t wf, const double *const *d_data,
                   const int32_t *const *d_indices, const int32_t *const *d_indptr)
{
    std::vector<int64_t> woff((size_t)count);
    int64_t total = 0;
    for (int32_t i = 0; i < count; ++i) { woff[(size_t)i] = wf * total; total += members[i].n; }
    std::vector<PivotSolveDesc> fresh;
    fresh.reserve(S.launched.size());
    for (int32_t i : S.launched) {
        PivotSolveDesc e;
        e.aval = d_data[i]; e.aidx = d_indices[i]; e.aptr = d_indptr[i];
        e.woff = woff[(size_t)i]; e.member = i; e.pad = 0;
        fresh.push_back(e);
    }
    batch_upload(S.stream, S.sys, fresh, false);
}

// Route and describe the members of a batched MULTILEVEL apply (k_ml_apply_batch), as batch_describe does for the other classes: route 0 =
// the launch (n <= cap_n, no level object degenerate), 1 = too large, 2 = degenerate.  S.mfresh / S.lfresh / S.launched receive a member's
// record, one record per level (ml_member_records) and the member numbers of route 0; a member's scratch is the object's own buf.
void ml_apply_describe(BatchScratch &S, int32_t count, const BatchMember *members, const int64_t *offsets, int64_t cap_n)
{
    S.route.assign((size_t)count, 0); S.status.assign((size_t)count, ILUPP_OK); S.h_err.assign((size_t)count, 0);
    S.launched.clear(); S.fresh.clear(); S.mfresh.clear(); S.lfresh.clear();
    for (int32_t i = 0; i < count; ++i) {
        ilupp_ml *m = members[i].ml;
        if (m->n > cap_n) { S.route[(size_t)i] = 1; continue; }
        const bool tr = !members[i].plain_first;
        MlApplyDesc d;
        memset(&d, 0, sizeof(d));
        d.n = m->n; d.levels = (int32_t)m->obj.size(); d.first = (int32_t)S.lfresh.size(); d.transpose = tr ? 1 : 0;
        d.xoff = offsets[i]; d.tmp = m->buf;
        if (!ml_member_records(m, tr, &S.lfresh)) { S.route[(size_t)i] = 2; continue; }
        S.mfresh.push_back(d);
        S.launched.push_back(i);
    }
}

// ... made ready for their launch, as batch_stage does: the bytes of LDS (8 n of the largest member, returned), the error words, the two
// tables (each uploaded again only when a record of it differs), and the stream behind whatever is still queued on a member's own stream
size_t ml_apply_stage(BatchScratch &S, const BatchMember *members)
{
    hipStream_t bs = S.stream;
    size_t lds = 0;
    for (const MlApplyDesc &d : S.mfresh) if ((size_t)8 * (size_t)d.n > lds) lds = (size_t)8 * (size_t)d.n;
    S.err.reserve(bs, S.mfresh.size());
    for (size_t k = 0; k < S.mfresh.size(); ++k) S.mfresh[k].err = S.err.d + k;
    batch_upload(bs, S.mltable, S.mfresh);
    batch_upload(bs, S.mllevels, S.lfresh);
    // (the levels of a member share the first one's stream: one join per member)
    for (int32_t i : S.launched) batch_join(bs, batch_stream_obj(members[i]));
    return lds;
}

// the single apply of a member on its own stream, and what waits for it
int batch_single_apply(const BatchMember &v, double *x, int transpose)
{
    return v.ml ? ml_apply_dev(v.ml, x, transpose) : v.owner ? pivot_apply_dev(v.owner, x, transpose) : apply_dev(v.p, x, transpose);
}
int batch_single_finish(const BatchMember &v) { return v.ml ? ml_finish_apply(v.ml) : finish_apply(v.p); }

// Queue the applies of all members (all of one class): route 0 = the launch (n within the LDS cap, object not degenerate), 1 = too large (for
// the LDS, or for a launch it would have to itself) and 2 = degenerate through the single apply on the member's own stream.  Multilevel
// members have a launch, a cap and tables of their own (ml_apply_describe); everything else is one path.  Everything is joined on the
// scratch's stream when this returns; nothing is waited for.
// staged: the vectors were put there by work on the scratch's stream (the host entry), not by the caller's stream.
int apply_batch_run(BatchScratch &S, int32_t count, const BatchMember *members, double *d_x, const int64_t *offsets, int transpose, bool staged)
{
    hipStream_t bs = S.stream;
    if (!staged) order_after_caller(bs, S.cev[0]);
    else ILUPP_HIP(hipEventRecord(S.in_ev, bs));
    const bool ml = members[0].ml != nullptr;
    const int64_t cap_n = ml ? ml_apply_batch_cap_n() : batch_apply_max_n();
    if (ml) ml_apply_describe(S, count, members, offsets, cap_n);
    else batch_describe(S, count, members, offsets, cap_n);
    // ONE member in the launch is one workgroup of 256 lanes walking all its rows, 0.06 ms + 0.015 ms per 1 000 rows, where the general sweeps
    // of the single apply take 0.11 - 0.12 ms whatever n is: past n = 4 096 the member alone is faster on the single apply (n = 4 000: 0.92 -
    // 1.18 x, 6 000: 1.2 - 1.5 x, 12 000: 1.9 - 2.5 x; two members of n = 12 000 break even, four take half the loop's time:
    // profiles/r10_pivot_apply_batch.txt)
    if (S.launched.size() == 1 && members[S.launched[0]].n > kSmallSweepMax) {
        S.route[(size_t)S.launched[0]] = 1;
        S.launched.clear(); S.fresh.clear(); S.mfresh.clear(); S.lfresh.clear();
    }
    if (!S.launched.empty()) {
        const int32_t nl = (int32_t)S.launched.size();
        if (ml) {
            const size_t lds = ml_apply_stage(S, members);
            OR_RETURN(ml_apply_batch_launch(bs, nl, S.mltable.d, S.mllevels.d, d_x, lds));
        } else {
            const size_t lds = batch_stage(S, members, cap_n);
            OR_RETURN(pivot_apply_batch_launch(bs, nl, S.table.d, d_x, lds));
        }
        batch_launched(S, members);
    }
    for (int32_t i = 0; i < count; ++i) {
        if (S.route[(size_t)i] == 0) continue;
        ilupp_precond *q = batch_stream_obj(members[i]);
        if (staged) ILUPP_HIP(hipStreamWaitEvent(q->stream, S.in_ev, 0));
        OR_RETURN(batch_single_apply(members[i], d_x + offsets[i], transpose));
        ILUPP_HIP(hipEventRecord(q->sev[1], q->stream));
        ILUPP_HIP(hipStreamWaitEvent(bs, q->sev[1], 0));
    }
    return ILUPP_OK;
}

// wait for a batch that apply_batch_run queued and say how it went: status per member, the first failure returned and named by its number
// (singles: the members of routes 1 and 2 went through their single applies -- not so behind the batched solve, which leaves them alone)
int apply_batch_finish(BatchScratch &S, int32_t count, const BatchMember *members, bool singles = true)
{
    const int32_t nl = (int32_t)S.launched.size();
    std::vector<std::string> msgs((size_t)count);
    for (int32_t i = 0; i < count; ++i)
        if (singles && S.route[(size_t)i] != 0) {
            S.status[(size_t)i] = batch_single_finish(members[i]);
            if (S.status[(size_t)i]) msgs[(size_t)i] = g_last_error;
        }
    std::vector<int32_t> err((size_t)(nl > 0 ? nl : 1), 0);
    if (nl > 0) ILUPP_HIP(d2h_async(S.stream, err.data(), S.err.d, sizeof(int32_t) * (size_t)nl));
    ILUPP_HIP(stream_sync(S.stream));
    for (int32_t k = 0; k < nl; ++k) {
        const int32_t i = S.launched[(size_t)k];
        batch_mark(members[i], nullptr);
        S.h_err[(size_t)i] = err[(size_t)k];
        if (err[(size_t)k]) { S.status[(size_t)i] = ILUPP_ERR_TIMEOUT; msgs[(size_t)i] = "triangular solve: dependency wait timed out (factor not triangular?)"; }
    }
    for (int32_t i = 0; i < count; ++i)
        if (S.status[(size_t)i]) { set_error("member " + std::to_string(i) + " of the batch: " + msgs[(size_t)i]); return S.status[(size_t)i]; }
    return ILUPP_OK;
}

// What both device entries of the batched apply do once their arguments are checked and their members named (count > 0): queue the
// applies, hand the routes out, and either wait for them (sync) or order the caller's stream behind them.
int apply_batch_device(int32_t count, const std::vector<BatchMember> &mv, double *d_x, const int64_t *offsets, int transpose, int sync,
                       int32_t *route)
{
    std::lock_guard<std::mutex> lk(g_batch_mu);
    BatchScratch &S = batch_scratch();
    const int rc = apply_batch_run(S, count, mv.data(), d_x, offsets, transpose, false);
    routes_out(S.route, route);
    if (rc) return rc;
    if (sync) return apply_batch_finish(S, count, mv.data());
    order_caller_after(S.stream, S.cev[1]);
    return ILUPP_OK;
}

// What both host entries of the batched apply do once their arguments are checked and their members named (at least one): x[i], len[i]
// doubles, is member i's vector, replaced by its apply.  The call has waited for everything when it returns.
int apply_batch_host(const std::vector<BatchMember> &mv, double *const *x, const int64_t *len, int transpose, int32_t *route)
{
    const int32_t count = (int32_t)mv.size();
    std::lock_guard<std::mutex> lk(g_batch_mu);
    BatchScratch &S = batch_scratch();
    // all vectors through ONE device buffer: one packed upload, one download
    std::vector<int64_t> off((size_t)count);
    size_t total = 0;
    for (int32_t i = 0; i < count; ++i) { off[(size_t)i] = (int64_t)total; total += (size_t)len[i]; }
    S.stage.reserve(S.stream, total);
    for (int32_t i = 0; i < count; ++i) memcpy(S.stage.h + off[(size_t)i], x[i], sizeof(double) * (size_t)len[i]);
    ILUPP_HIP(hipMemcpyAsync(S.stage.d, S.stage.h, sizeof(double) * total, hipMemcpyHostToDevice, S.stream));
    int rc = apply_batch_run(S, count, mv.data(), S.stage.d, off.data(), transpose, true);
    routes_out(S.route, route);
    if (rc) { (void)hipStreamSynchronize(S.stream); return rc; }
    ILUPP_HIP(hipMemcpyAsync(S.stage.h, S.stage.d, sizeof(double) * total, hipMemcpyDeviceToHost, S.stream));
    rc = apply_batch_finish(S, count, mv.data());
    // (a member that failed keeps its vector as it was; the others have theirs)
    for (int32_t i = 0; i < count; ++i)
        if (S.status[(size_t)i] == ILUPP_OK) memcpy(x[i], S.stage.h + off[(size_t)i], sizeof(double) * (size_t)len[i]);
    return rc;
}

// ---- the argument checks the entries share, each entry in its own order: all before any device call ----
// the host vectors of a batched apply: every one there, and as long as its member
template <class Handle>
int batch_vector_args(int32_t count, Handle *const *members, double *const *x, const int64_t *len)
{
    for (int32_t i = 0; i < count; ++i) {
        if (!x[i]) { set_error("null argument"); return ILUPP_ERR_INVALID; }
        if (len[i] != members[i]->n) { set_error("vector has wrong size for preconditioner!"); return ILUPP_ERR_WRONG_SIZE; }
    }
    return ILUPP_OK;
}

// a handle that stands twice in `seen` (a member's scratch vector and its factors serve one launch at a time)
int batch_no_duplicates(std::vector<const void *> &seen)
{
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { set_error("a preconditioner appears twice in the batch"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

// the three arrays of member i's matrix
int batch_matrix_arrays(const double *const *d_data, const int32_t *const *d_indices, const int32_t *const *d_indptr, int32_t i)
{
    if (!d_data[i] || !d_indices[i] || !d_indptr[i]) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

int batch_iteration_args(int32_t maxiter, int32_t check_every)
{
    if (maxiter < 0 || check_every < 0) { set_error("maxiter and check_every must not be negative"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

// the workspace of a solve over `total` unknowns
int batch_workspace(BatchSolver solver, int64_t work_doubles, int64_t total)
{
    const int64_t wf = solve_batch_work_factor(solver);
    if (work_doubles < wf * total) { set_error("workspace too small: " + std::to_string(wf) + " doubles per unknown of the batch"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

// null arguments, a negative count, a null member, a member named twice
int pivot_batch_args(int32_t count, ilupp_ilucp *const *members, const void *a, const void *b)
{
    if (count < 0 || !members || !a || !b) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) if (!members[i]) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
    std::vector<const void *> seen(members, members + count);
    return batch_no_duplicates(seen);
}

// the same for a list of non-pivoting objects; null_ok: a null handle is a member without a preconditioner (the CG solve), any number of them.
// A multilevel object handed in as a member is named before anything reads it as an ilupp_precond.
int plain_batch_args(int32_t count, ilupp_precond *const *members, bool null_ok, const void *a, const void *b)
{
    if (count < 0 || !members || !a || !b) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    std::vector<const void *> seen;
    for (int32_t i = 0; i < count; ++i) {
        if (!members[i]) { if (null_ok) continue; set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
        if (is_live_ml(members[i])) { set_error("a multilevel preconditioner cannot be a member of a batch"); return ILUPP_ERR_INVALID; }
        seen.push_back(members[i]);
    }
    return batch_no_duplicates(seen);
}

// What the three batched solves do once their arguments are checked and their members named (count > 0): the members routed and
// described, those of route 0 solved in ONE launch of `solver`'s kernel on the scratch's stream behind the caller's, and either waited
// for (sync) or the caller's stream ordered behind them.  Members of routes 1 and 2 are left alone.
int solve_batch_run(BatchSolver solver, int32_t count, const std::vector<BatchMember> &mv, const double *const *d_data,
                    const int32_t *const *d_indices, const int32_t *const *d_indptr, const double *d_b, const double *d_x0, double *d_x,
                    const int64_t *offsets, double *d_work, int32_t maxiter, double rtol, int32_t check_every, int64_t *d_iterations,
                    int32_t *d_flags, double *d_rr, double *d_last, int sync, int32_t *route)
{
    std::lock_guard<std::mutex> lk(g_batch_mu);
    BatchScratch &S = batch_scratch();
    hipStream_t bs = S.stream;
    order_after_caller(bs, S.cev[0]);
    // The launch with a multilevel member is another instantiation of the kernel with a cap of its own: the members are routed by the
    // cap of the instantiation that is launched -- and where no multilevel member takes route 0 after all, by the other one's again, for
    // the launch they have always had.
    bool ml = std::any_of(mv.begin(), mv.end(), [](const BatchMember &v) { return v.ml != nullptr; });
    int64_t cap_n = solve_batch_cap_n(solver, ml);
    batch_describe(S, count, mv.data(), offsets, cap_n);
    if (ml && S.lfresh.empty()) {
        const std::vector<int32_t> routed = S.route;
        ml = false;
        cap_n = solve_batch_cap_n(solver, false);
        batch_describe(S, count, mv.data(), offsets, cap_n, false);
        for (int32_t i = 0; i < count; ++i) if (mv[(size_t)i].ml) S.route[(size_t)i] = routed[(size_t)i];
    }
    routes_out(S.route, route);
    const int32_t nl = (int32_t)S.launched.size();
    if (nl == 0) return ILUPP_OK;
    const size_t lds = batch_stage(S, mv.data(), cap_n);
    batch_systems(S, count, mv.data(), solve_batch_work_factor(solver), d_data, d_indices, d_indptr);
    OR_RETURN(solve_batch_launch(solver, bs, nl, S.table.d, S.sys.d, d_b, d_x0, d_x, d_work, lds, maxiter, rtol, check_every, d_iterations,
                                 d_flags, d_rr, d_last, ml));
    batch_launched(S, mv.data());
    if (sync) return apply_batch_finish(S, count, mv.data(), false);
    order_caller_after(bs, S.cev[1]);
    return ILUPP_OK;
}

// ---- many MULTILEVEL members applied at once: one launch, one workgroup per member (k_ml_apply_batch, sptrsv_batch.hip) ----
// null arguments, a negative count, a null member, a member named twice
int ml_batch_args(int32_t count, ilupp_ml *const *members, const void *a, const void *b)
{
    if (count < 0 || !members || !a || !b) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) {
        if (!members[i]) { set_error("null preconditioner"); return ILUPP_ERR_INVALID; }
        if (!is_live_ml(members[i])) { set_error("member " + std::to_string(i) + " of the batch is not a multilevel preconditioner"); return ILUPP_ERR_INVALID; }
    }
    std::vector<const void *> seen(members, members + count);
    return batch_no_duplicates(seen);
}

}  // namespace

extern "C" {

int ilupp_hip_apply_batch_device(int32_t count, ilupp_precond *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                 int32_t *route)
{
    API_TRY
    const int rc0 = plain_batch_args(count, members, false, d_x, offsets);
    if (rc0 || count == 0) return rc0;
    return apply_batch_device(count, batch_members(count, members, transpose), d_x, offsets, transpose, sync, route);
    API_CATCH
}

int ilupp_hip_cg_batch_device(int32_t count, ilupp_precond *const *members, const int64_t *n, const double *const *d_data,
                              const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b,
                              const double *d_x0, double *d_x, const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter,
                              double rtol, int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_bnorm, int sync,
                              int32_t *route)
{
    API_TRY
    OR_RETURN(plain_batch_args(count, members, true, d_x, offsets));
    if (!n || !d_data || !d_indices || !d_indptr || !nnz || !d_b || !d_work || !d_iterations || !d_flags || !d_rr || !d_bnorm) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    OR_RETURN(batch_iteration_args(maxiter, check_every));
    int64_t total = 0;
    for (int32_t i = 0; i < count; ++i) {
        OR_RETURN(batch_matrix_arrays(d_data, d_indices, d_indptr, i));
        if (n[i] <= 0 || n[i] > INT32_MAX) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
        if (members[i] && members[i]->n != n[i]) { set_error("matrix has wrong size for preconditioner!"); return ILUPP_ERR_WRONG_SIZE; }
        total += n[i];
    }
    OR_RETURN(batch_workspace(BATCH_CG, work_doubles, total));
    if (count == 0) return ILUPP_OK;
    std::vector<BatchMember> mv((size_t)count);
    for (int32_t i = 0; i < count; ++i) { if (members[i]) mv[(size_t)i] = batch_member(members[i], 0); mv[(size_t)i].n = (int32_t)n[i]; }
    return solve_batch_run(BATCH_CG, count, mv, d_data, d_indices, d_indptr, d_b, d_x0, d_x, offsets, d_work, maxiter, rtol, check_every,
                           d_iterations, d_flags, d_rr, d_bnorm, sync, route);
    API_CATCH
}

int64_t ilupp_hip_cg_batch_max_n(void)
{
    API_TRY
    return solve_batch_cap_n(BATCH_CG);
    API_CATCH
}

int ilupp_hip_pivot_apply_batch_device(int32_t count, ilupp_ilucp *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                       int32_t *route)
{
    API_TRY
    const int rc0 = pivot_batch_args(count, members, d_x, offsets);
    if (rc0 || count == 0) return rc0;
    return apply_batch_device(count, batch_members(count, members, transpose), d_x, offsets, transpose, sync, route);
    API_CATCH
}

int ilupp_hip_pivot_apply_batch(int32_t count, ilupp_ilucp *const *members, double *const *x, const int64_t *len, int transpose, int32_t *route)
{
    API_TRY
    OR_RETURN(pivot_batch_args(count, members, x, len));
    OR_RETURN(batch_vector_args(count, members, x, len));
    if (count == 0) return ILUPP_OK;
    return apply_batch_host(batch_members(count, members, transpose), x, len, transpose, route);
    API_CATCH
}

int ilupp_hip_pivot_bicgstab_batch_device(int32_t count, ilupp_ilucp *const *members, const double *const *d_data, const int32_t *const *d_indices,
                                          const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x,
                                          const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter, double rtol,
                                          int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync,
                                          int32_t *route)
{
    API_TRY
    OR_RETURN(pivot_batch_args(count, members, d_x, offsets));
    if (!d_data || !d_indices || !d_indptr || !nnz || !d_b || !d_work || !d_iterations || !d_flags || !d_rr || !d_init) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    OR_RETURN(batch_iteration_args(maxiter, check_every));
    int64_t total = 0;
    for (int32_t i = 0; i < count; ++i) {
        OR_RETURN(batch_matrix_arrays(d_data, d_indices, d_indptr, i));
        total += members[i]->n;
    }
    OR_RETURN(batch_workspace(BATCH_BICGSTAB, work_doubles, total));
    if (count == 0) return ILUPP_OK;
    return solve_batch_run(BATCH_BICGSTAB, count, batch_members(count, members, 0), d_data, d_indices, d_indptr, d_b, d_x0, d_x, offsets,
                           d_work, maxiter, rtol, check_every, d_iterations, d_flags, d_rr, d_init, sync, route);
    API_CATCH
}

// what ilupp_hip_bicgstab_batch_device and ilupp_hip_bicgstab_batch_ml_device do (the first without a list of multilevel members)
static int bicgstab_batch_entry(int32_t count, ilupp_precond *const *plain, ilupp_ilucp *const *pivoted, ilupp_ml *const *multilevel, const int64_t *n,
                                const double *const *d_data, const int32_t *const *d_indices, const int32_t *const *d_indptr,
                                const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x, const int64_t *offsets,
                                double *d_work, int64_t work_doubles, int32_t maxiter, double rtol, int32_t check_every,
                                int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync, int32_t *route)
{
    if (count < 0 || !d_x || !offsets || !n || !d_data || !d_indices || !d_indptr || !nnz || !d_b || !d_work || !d_iterations || !d_flags ||
        !d_rr || !d_init) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    OR_RETURN(batch_iteration_args(maxiter, check_every));
    // member i: pivoted[i], or plain[i], or multilevel[i], or none of them (no preconditioner); a multilevel object among `plain` is
    // named before anything reads it as an ilupp_precond, and a member of `multilevel` must be a live one
    std::vector<const void *> seen_plain, seen_pivoted, seen_ml;
    int64_t total = 0;
    for (int32_t i = 0; i < count; ++i) {
        ilupp_precond *p = plain ? plain[i] : nullptr;
        ilupp_ilucp *m = pivoted ? pivoted[i] : nullptr;
        ilupp_ml *q = multilevel ? multilevel[i] : nullptr;
        if (p && m) { set_error("member " + std::to_string(i) + " of the batch: both a pivoting and a non-pivoting preconditioner"); return ILUPP_ERR_INVALID; }
        if (q && (p || m)) { set_error("member " + std::to_string(i) + " of the batch: both a multilevel and another preconditioner"); return ILUPP_ERR_INVALID; }
        if (p && is_live_ml(p)) { set_error("a multilevel preconditioner cannot be a member of a batch"); return ILUPP_ERR_INVALID; }
        if (q && !is_live_ml(q)) { set_error("member " + std::to_string(i) + " of the batch is not a multilevel preconditioner"); return ILUPP_ERR_INVALID; }
        OR_RETURN(batch_matrix_arrays(d_data, d_indices, d_indptr, i));
        if (n[i] <= 0 || n[i] > INT32_MAX) { set_error("matrix has size 0!"); return ILUPP_ERR_INVALID; }
        if ((p && p->n != n[i]) || (m && m->n != n[i]) || (q && q->n != n[i])) { set_error("matrix has wrong size for preconditioner!"); return ILUPP_ERR_WRONG_SIZE; }
        if (p) seen_plain.push_back(p);
        if (m) seen_pivoted.push_back(m);
        if (q) seen_ml.push_back(q);
        total += n[i];
    }
    OR_RETURN(batch_no_duplicates(seen_plain));
    OR_RETURN(batch_no_duplicates(seen_pivoted));
    OR_RETURN(batch_no_duplicates(seen_ml));
    OR_RETURN(batch_workspace(BATCH_BICGSTAB, work_doubles, total));
    if (count == 0) return ILUPP_OK;
    std::vector<BatchMember> mv((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        if (pivoted && pivoted[i]) mv[(size_t)i] = batch_member(pivoted[i], 0);
        else if (plain && plain[i]) mv[(size_t)i] = batch_member(plain[i], 0);
        else if (multilevel && multilevel[i]) mv[(size_t)i] = batch_member(multilevel[i], 0);
        mv[(size_t)i].n = (int32_t)n[i];
    }
    return solve_batch_run(BATCH_BICGSTAB, count, mv, d_data, d_indices, d_indptr, d_b, d_x0, d_x, offsets, d_work, maxiter, rtol,
                           check_every, d_iterations, d_flags, d_rr, d_init, sync, route);
}

int ilupp_hip_bicgstab_batch_device(int32_t count, ilupp_precond *const *plain, ilupp_ilucp *const *pivoted, const int64_t *n,
                                    const double *const *d_data, const int32_t *const *d_indices, const int32_t *const *d_indptr,
                                    const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x, const int64_t *offsets,
                                    double *d_work, int64_t work_doubles, int32_t maxiter, double rtol, int32_t check_every,
                                    int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync, int32_t *route)
{
    API_TRY
    return bicgstab_batch_entry(count, plain, pivoted, nullptr, n, d_data, d_indices, d_indptr, nnz, d_b, d_x0, d_x, offsets, d_work, work_doubles,
                                maxiter, rtol, check_every, d_iterations, d_flags, d_rr, d_init, sync, route);
    API_CATCH
}

int ilupp_hip_bicgstab_batch_ml_device(int32_t count, ilupp_precond *const *plain, ilupp_ilucp *const *pivoted, ilupp_ml *const *multilevel,
                                       const int64_t *n, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x,
                                       const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter, double rtol,
                                       int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync,
                                       int32_t *route)
{
    API_TRY
    return bicgstab_batch_entry(count, plain, pivoted, multilevel, n, d_data, d_indices, d_indptr, nnz, d_b, d_x0, d_x, offsets, d_work,
                                work_doubles, maxiter, rtol, check_every, d_iterations, d_flags, d_rr, d_init, sync, route);
    API_CATCH
}

int64_t ilupp_hip_bicgstab_batch_ml_max_n(void)
{
    API_TRY
    return solve_batch_cap_n(BATCH_BICGSTAB, true);
    API_CATCH
}

int64_t ilupp_hip_bicgstab_batch_max_n(void)
{
    API_TRY
    return solve_batch_cap_n(BATCH_BICGSTAB);
    API_CATCH
}

int64_t ilupp_hip_pivot_apply_batch_max_n(void)
{
    API_TRY
    return batch_apply_max_n();
    API_CATCH
}

int ilupp_hip_ml_apply_batch_device(int32_t count, ilupp_ml *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                    int32_t *route)
{
    API_TRY
    const int rc0 = ml_batch_args(count, members, d_x, offsets);
    if (rc0 || count == 0) return rc0;
    return apply_batch_device(count, batch_members(count, members, transpose), d_x, offsets, transpose, sync, route);
    API_CATCH
}

int ilupp_hip_ml_apply_batch(int32_t count, ilupp_ml *const *members, double *const *x, const int64_t *len, int transpose, int32_t *route)
{
    API_TRY
    OR_RETURN(ml_batch_args(count, members, x, len));
    OR_RETURN(batch_vector_args(count, members, x, len));
    if (count == 0) return ILUPP_OK;
    return apply_batch_host(batch_members(count, members, transpose), x, len, transpose, route);
    API_CATCH
}

int64_t ilupp_hip_ml_apply_batch_max_n(void)
{
    API_TRY
    return ml_apply_batch_cap_n();
    API_CATCH
}

}  // extern "C"

namespace {

// What the batched re-factorisation and the batched first construction of ILU(0) and of IChol(0) differ in; everything else of the two
// host scaffolds below is one copy.
struct CreateMember;
struct FactorBatchKind {
    const char *name, *object;                       // in messages: "ILU0", "an ILU(0) object"
    bool llt;                                        // one factor Lc (and its transposed copy, kept current) instead of Lc and Uc
    int32_t alone_min;                               // rows from which a member that would have the launch to itself takes the single path
    bool (*is_object)(const ilupp_precond *);
    bool (*is_static)(const ilupp_precond *);        // the values live elsewhere than in the CSR factor(s), or the single path is the static form's
    size_t (*fits)(int32_t n, int32_t max_row_len);
    int64_t (*max_n)();
    int (*refactor_launch)(hipStream_t, int32_t, const RefactorDesc *, int32_t *, size_t);
    int (*symbolic_launch)(hipStream_t, int32_t, const RefactorDesc *, CreateInfo *);
    int (*create_launch)(hipStream_t, int32_t, const RefactorDesc *, int32_t *, size_t);
    int (*refactor_single)(ilupp_precond *, const double *, const int32_t *, const int32_t *);
    // the single constructor inside a batched construction (staged: the matrix was uploaded on the scratch's stream, in_ev behind it)
    int (*create_single)(const CreateMember &, int is_csr, bool staged, hipEvent_t in_ev, ilupp_precond **out);
};
int ilu0_create_single(const CreateMember &m, int is_csr, bool staged, hipEvent_t in_ev, ilupp_precond **out);
int ichol0_create_single(const CreateMember &m, int is_csr, bool staged, hipEvent_t in_ev, ilupp_precond **out);
// ONE member in the launch is one workgroup walking all its rows where the single path's factor kernels spread them over the chip, and
// the launch then saves no host wait that matters.  ILU(0) alone: n = 1 000 takes 0.447 ms in the launch against 0.202 ms on the single
// path, n = 4 000 0.858 against 0.167 ms (profiles/r13_refactor_batch.txt, "alone in the launch"; smaller n not measured: it stays in
// the launch).  IChol(0) alone: n = 250 0.461 ms in the launch against 0.636 ms, n = 1 000 1.423 against 0.738 ms, n = 4 000 3.354 against
// 0.843 ms (profiles/r16_ichol0_batch.txt, "alone in the launch"): the single path wins from the same 1 000 rows on.
const FactorBatchKind kIlu0Batch = {"ILU0", "an ILU(0) object", false, 1000, is_ilu0_object,
                                    [](const ilupp_precond *p) { return p->flm.built; }, ilu0_refactor_batch_fits, ilu0_refactor_batch_max_n,
                                    ilu0_refactor_batch_launch, ilu0_symbolic_batch_launch, ilu0_create_batch_launch, ilu0_refactor_single,
                                    ilu0_create_single};
const FactorBatchKind kIchol0Batch = {"IChol0", "an IChol(0) object", true, 1000, is_ichol0_object,
                                      [](const ilupp_precond *p) { return p->chol_static; }, ichol0_refactor_batch_fits, ichol0_refactor_batch_max_n,
                                      ichol0_refactor_batch_launch, ichol0_symbolic_batch_launch, ichol0_create_batch_launch, ichol0_refactor_single,
                                      ichol0_create_single};

}  // namespace

extern "C" {

// one member of the launches: the matrix and the two triangles of p -- Lc and Uc, for IChol(0) Lc and its transposed copy LcT when the
// object has one (at the symbolic launch the index and value arrays are not there yet: null) --, the number of stored entries the matrix
// is to have, and the member's number in the call
static RefactorDesc refactor_desc(const FactorBatchKind &K, const ilupp_precond *p, const double *aval, const int32_t *aidx, const int32_t *aptr,
                                  int64_t nnzA, int32_t member)
{
    RefactorDesc d;
    memset(&d, 0, sizeof(d));
    d.aptr = aptr; d.aidx = aidx; d.aval = aval;
    d.lptr = p->Lc.ptr; d.lidx = p->Lc.idx; d.lval = p->Lc.val;
    if (!K.llt) { d.uptr = p->Uc.ptr; d.uidx = p->Uc.idx; d.uval = p->Uc.val; }
    else if (p->haveT) { d.uptr = p->LcT.ptr; d.uidx = p->LcT.idx; d.uval = p->LcT.val; }
    d.nnzA = nnzA; d.n = p->n; d.member = member;
    return d;
}

// what ilupp_hip_ilu0_refactor_batch_device and ilupp_hip_ichol0_refactor_batch_device do, under the construction lock its caller holds (the construction lock first, then the
// batch lock: pool blocks are freed below; no path takes the two in the other order)
static int refactor_batch_locked(const FactorBatchKind &K, int32_t count, ilupp_precond *const *members, const double *const *d_data,
                                 const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz,
                                 int32_t *d_status, int sync, int32_t *route)
{
    OR_RETURN(plain_batch_args(count, members, false, d_data, nnz));
    if (!d_indices || !d_indptr || !d_status) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) {
        OR_RETURN(batch_matrix_arrays(d_data, d_indices, d_indptr, i));
        if (!K.is_object(members[i])) { set_error("member " + std::to_string(i) + " of the batch: not " + K.object); return ILUPP_ERR_INVALID; }
        if (nnz[i] != members[i]->nnzA) {
            set_error("member " + std::to_string(i) + " of the batch: the matrix does not have the analysed pattern");
            return ILUPP_ERR_INVALID;
        }
    }
    if (count == 0) return ILUPP_OK;
    std::lock_guard<std::mutex> lk(g_batch_mu);
    BatchScratch &S = batch_scratch();
    hipStream_t bs = S.stream;
    order_after_caller(bs, S.cev[0]);
    // routes: 0 = the launch, 1 = n above the cap or a row above the row cap (K.fits), 2 = static form (ILU(0): its values live in
    // lane-table records; IChol(0): its single path is the static kernel)
    const int64_t cap_n = batch_env_cap(K.max_n());
    S.route.assign((size_t)count, 0); S.launched.clear();
    size_t lds = 0;                                                     // what the launch's most demanding member asks for
    for (int32_t i = 0; i < count; ++i) {
        const ilupp_precond *p = members[i];
        if (K.is_static(p)) { S.route[(size_t)i] = 2; continue; }
        // (a member the batched construction built has no single numeric path, and fits by construction: the launch, whatever the cap says)
        if (p->n > cap_n && !p->batch_built) { S.route[(size_t)i] = 1; continue; }
        const size_t want = K.fits(p->n, p->max_row_len);
        if (want == 0) { S.route[(size_t)i] = 1; continue; }
        S.launched.push_back(i);
        if (want > lds) lds = want;
    }
    // From K.alone_min rows on, a member that would have the launch to itself takes the single path (the measurements: at the kinds' table).
    // ILUPP_REFACTOR_ALONE_MIN moves the threshold (read per call; the measurement sets it above n to time the launch of one member).
    long long alone_min = K.alone_min;
    if (const char *e = getenv("ILUPP_REFACTOR_ALONE_MIN")) { const long long v = atoll(e); if (v > 0) alone_min = v; }
    if (S.launched.size() == 1 && members[S.launched[0]]->n >= alone_min && !members[S.launched[0]]->batch_built) { S.route[(size_t)S.launched[0]] = 1; S.launched.clear(); }
    routes_out(S.route, route);
    const int32_t nl = (int32_t)S.launched.size();
    if (nl > 0) {
        // (uploaded again only when a descriptor differs: the same members with their matrices in the same buffers, step after step, upload nothing)
        std::vector<RefactorDesc> fresh;
        fresh.reserve((size_t)nl);
        for (int32_t i : S.launched) fresh.push_back(refactor_desc(K, members[i], d_data[i], d_indices[i], d_indptr[i], members[i]->nnzA, i));
        batch_upload(bs, S.rtable, fresh);
        // the launch behind whatever is still queued on a member's own stream; what earlier batched launches read of the factors lies on
        // the scratch's stream itself
        bool stale = false;
        for (int32_t i : S.launched) {
            ilupp_precond *p = members[i];
            // (IChol(0): the launch writes the transposed copy too, which therefore stays; what goes are the packed sweeps of the two)
            if (K.llt) stale = stale || p->pkL.built || p->pkL.valid || p->pkLT.built || p->pkLT.valid;
            else stale = stale || p->pkL.valid || p->pkU.valid || p->pkL.pkT || p->pkU.pkT || p->haveT;
            for (const auto &l : p->lvl) stale = stale || l.tried;
            batch_join(bs, p);
        }
        OR_RETURN(K.refactor_launch(bs, nl, S.rtable.d, d_status, lds));
        const std::vector<BatchMember> mv = batch_members(count, members, 0);
        batch_launched(S, mv.data());
        // this launch WRITES the factors: whatever a member's own stream does next (a single apply, factors(), ensure_*) comes after it
        for (int32_t i : S.launched) ILUPP_HIP(hipStreamWaitEvent(members[i]->stream, S.done_ev, 0));
        // copies of the old values go (as in the single path; the non-static packed sweeps too: they are rebuilt at the next single apply,
        // not re-packed per member here).  The pool knows nothing of streams: ONE wait for the whole call before the first free, and none
        // when no member holds such a copy -- the steady state of refactor -> cg_batch -> refactor.
        if (stale) ILUPP_HIP(hipStreamSynchronize(bs));
        for (int32_t i : S.launched) {
            ilupp_precond *p = members[i];
            p->csr_vals = true;
            if (K.llt) { drop_llt_sweep_copies(p); continue; }      // (Lc and LcT, with LcT's schedule and descriptors, hold the new values)
            drop_old_value_copies(p);
            if (p->pkL.valid) { p->pkL.release(); p->pack_tried[0] = false; }
            if (p->pkU.valid) { p->pkU.release(); p->pack_tried[1] = false; }
        }
    }
    // routes 1 and 2: the single path on the member's own stream (it waits for its stream itself); the status word by the host afterwards
    for (int32_t i = 0; i < count; ++i) {
        if (S.route[(size_t)i] == 0) continue;
        const int rc = K.refactor_single(members[i], d_data[i], d_indices[i], d_indptr[i]);
        if (rc != ILUPP_OK && rc != ILUPP_ERR_INVALID && rc != ILUPP_ERR_TIMEOUT) return rc;
        ILUPP_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_status + i), rc == ILUPP_OK ? 0 : rc == ILUPP_ERR_INVALID ? 1 : 2, 1, bs));
    }
    if (sync) {
        std::vector<int32_t> st((size_t)count, 0);
        ILUPP_HIP(d2h_async(bs, st.data(), d_status, sizeof(int32_t) * (size_t)count));
        ILUPP_HIP(stream_sync(bs));
        for (int32_t i : S.launched) members[i]->batch_ev = nullptr;
        for (int32_t i = 0; i < count; ++i) {
            if (st[(size_t)i] == 1) { set_error("member " + std::to_string(i) + " of the batch: the matrix does not have the analysed pattern"); return ILUPP_ERR_INVALID; }
            if (st[(size_t)i] != 0) { set_error("member " + std::to_string(i) + " of the batch: " + K.name + ": dependency wait timed out"); return ILUPP_ERR_TIMEOUT; }
        }
        return ILUPP_OK;
    }
    order_caller_after(bs, S.cev[1]);
    return ILUPP_OK;
}

int ilupp_hip_ilu0_refactor_batch_device(int32_t count, ilupp_precond *const *members, const double *const *d_data,
                                         const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz,
                                         int32_t *d_status, int sync, int32_t *route)
{
    API_TRY_BUILD
    return refactor_batch_locked(kIlu0Batch, count, members, d_data, d_indices, d_indptr, nnz, d_status, sync, route);
    API_CATCH
}

int64_t ilupp_hip_ilu0_refactor_batch_max_n(void)
{
    API_TRY
    return refactor_batch_max_n();
    API_CATCH
}

int ilupp_hip_ichol0_refactor_batch_device(int32_t count, ilupp_precond *const *members, const double *const *d_data,
                                           const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz,
                                           int32_t *d_status, int sync, int32_t *route)
{
    API_TRY_BUILD
    return refactor_batch_locked(kIchol0Batch, count, members, d_data, d_indices, d_indptr, nnz, d_status, sync, route);
    API_CATCH
}

int64_t ilupp_hip_ichol0_refactor_batch_max_n(void)
{
    API_TRY
    return batch_env_cap(ichol0_refactor_batch_max_n());
    API_CATCH
}

}  // extern "C"

// ---- many ILU(0) or IChol(0) objects built at once: a symbolic launch, one read-back, a create launch (ilu0_batch.hip, ichol0_batch.hip) ----
namespace {

int refactor_in_launch(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr)
{
    // (never reached from the batched re-factorisation, which holds the batch lock and sends such a member to its launch)
    ilupp_precond *const one[1] = {p};
    const double *const dd[1] = {d_data};
    const int32_t *const di[1] = {d_indices}, *const dp[1] = {d_indptr};
    const int64_t nz[1] = {p->nnzA};
    const int rc = refactor_batch_locked(p->kind == KIND_LLT ? kIchol0Batch : kIlu0Batch, 1, one, dd, di, dp, nz, p->ctrl + 2, 1, nullptr);      // (ctrl[2]: a word no sweep of such an object uses)
    if (rc) {
        const std::string prefix = "member 0 of the batch: ", msg = g_last_error;
        if (msg.compare(0, prefix.size(), prefix) == 0) set_error(msg.substr(prefix.size()));
    }
    return rc;
}

// one matrix of a batched construction: device CSR arrays (the caller's, or slices of the scratch's staging block), and for the host
// entry the host arrays they were copied from
struct CreateMember {
    const double *data = nullptr; const int32_t *indices = nullptr, *indptr = nullptr;
    int32_t n = 0; int64_t nnz = 0;
    const int32_t *h_indices = nullptr, *h_indptr = nullptr;
};

// the objects of a call until it has succeeded: whatever makes it unwind destroys them all
struct CreatedObjects {
    std::vector<ilupp_precond *> v;
    ~CreatedObjects() { for (ilupp_precond *p : v) if (p) { if (p->side) (void)stream_sync(p->side); destroy_obj(p); } }
};

// What the batched constructions share around their own launches, for one call: per member its code, its message, its route and its
// object.  The first failing member is reported as "matrix i of the batch: ...", status[i] says which failed, and no object of the call
// survives a failure (batch_build's convention).
struct CreateShell {
    const int32_t count;
    const CreateMember *const m;
    std::vector<int> rcs;
    std::vector<std::string> msgs;
    std::vector<int32_t> rt;
    CreatedObjects objs;
    bool failed = false;
    CreateShell(BatchScratch &S, int32_t count_, const CreateMember *m_) : count(count_), m(m_), rcs((size_t)count_, ILUPP_OK), msgs((size_t)count_), rt((size_t)count_, 0)
    {
        for (hipEvent_t &e : S.tev) if (!e) ILUPP_HIP(hipEventCreate(&e));
        objs.v.assign((size_t)count, nullptr);
    }
    void fail(int32_t i, int rc, const std::string &msg) { rcs[(size_t)i] = rc; msgs[(size_t)i] = msg; failed = true; }
    // a member no construction of `name`'s kind takes
    bool refused(int32_t i, const char *name)
    {
        if (m[i].n <= 0 || !m[i].indptr) { fail(i, ILUPP_ERR_INVALID, "matrix has size 0!"); return true; }
        if (m[i].nnz < 0 || m[i].nnz + (int64_t)m[i].n > INT32_MAX) { fail(i, ILUPP_ERR_INVALID, std::string(name) + ": too many stored entries for 32-bit indices"); return true; }
        return false;
    }
    // route 1: single(i, &object), the single constructor, on the member's own stream, next to the launches (it waits for its stream
    // itself); nothing more is built once a member has failed
    template <class Single>
    void singles(Single &&single)
    {
        for (int32_t i = 0; i < count && !failed; ++i) {
            if (rt[(size_t)i] != 1) continue;
            if (objs.v[(size_t)i]) { destroy_obj(objs.v[(size_t)i]); objs.v[(size_t)i] = nullptr; }      // (it only held the two row-pointer arrays)
            const int rc = single(i, &objs.v[(size_t)i]);
            if (rc) fail(i, rc, g_last_error);
        }
    }
    // the routes and the codes into the caller's arrays, then the first failure, or the objects handed out
    int report(ilupp_precond **out, int32_t *status, int32_t *route)
    {
        routes_out(rt, route);
        const int first = batch_first_failure(count, rcs, msgs, status);
        if (first) return first;                     // (objs goes, and every object of the call with it)
        for (int32_t i = 0; i < count; ++i) { out[i] = objs.v[(size_t)i]; objs.v[(size_t)i] = nullptr; }
        return ILUPP_OK;
    }
};

// What the entries of the batched ILU(0) and IChol(0) constructions do once the matrices are in device memory (count > 0; the caller holds the
// construction lock and the batch lock).  staged: the matrices were uploaded on the scratch's stream (S.in_ev behind the upload), not
// produced on the caller's.  Routes: 0 = built by the two launches; 1 = built by the single constructor inside this call (n above the cap
// of the re-factorisation's launch, a longest row above its row cap, a matrix whose rows are not sorted or whose indices are out of
// range -- whatever the single constructor does with it, it does here --, or a batch of one: a user who builds one object wants the
// fully analysed one).  Failures as CreateShell reports them.
int factor_create_batch_run(const FactorBatchKind &K, BatchScratch &S, int32_t count, const CreateMember *m, int is_csr, bool staged, ilupp_precond **out, int32_t *status,
                          int32_t *route)
{
    hipStream_t bs = S.stream;
    CreateShell C(S, count, m);
    std::vector<int32_t> &rt = C.rt;
    std::vector<ilupp_precond *> &objs = C.objs.v;
    const int64_t cap_n = batch_env_cap(K.max_n());
    std::vector<int32_t> cand;                       // the members of the symbolic launch
    for (int32_t i = 0; i < count; ++i) {
        if (C.refused(i, K.name)) continue;
        if (count == 1 || m[i].n > cap_n) { rt[(size_t)i] = 1; continue; }
        cand.push_back(i);
    }
    if (!staged) order_after_caller(bs, S.cev[0]);
    const int32_t nc = (int32_t)cand.size();
    std::vector<int32_t> launched;                   // the members of the create launch
    std::vector<RefactorDesc> fresh;
    float sym_ms = 0.f, create_ms = 0.f;
    if (nc > 0) {
        S.cinfo.reserve(bs, (size_t)count);
        S.cstat.reserve(bs, (size_t)count);
        // the objects, and the n + 1 row pointers of L and of U the symbolic launch writes
        for (int32_t i : cand) {
            ilupp_precond *p = objs[(size_t)i] = new_obj(m[i].n);
            if (K.llt) { p->kind = KIND_LLT; p->nnz_mode = NNZ_LLT; p->llt_diag_last = true; }
            else { p->kind = KIND_LU; p->nnz_mode = NNZ_GENERIC_LU; p->input_csc = !is_csr; }
            for (DevMat *M : {&p->Lc, &p->Uc}) {
                if (K.llt && M == &p->Uc) continue;
                M->n = m[i].n; M->is_csr = true; M->owns = true;
                ILUPP_HIP(pool_malloc(&M->ptr, sizeof(int32_t) * (size_t)(m[i].n + 1)));
            }
            fresh.push_back(refactor_desc(K, p, m[i].data, m[i].indices, m[i].indptr, m[i].nnz, i));
        }
        // (sent whatever the table holds, and the re-factorisation's cached table is gone: these descriptors are half filled)
        batch_upload(bs, S.rtable, fresh, false);
        ILUPP_HIP(hipEventRecord(S.tev[0], bs));
        OR_RETURN(K.symbolic_launch(bs, nc, S.rtable.d, S.cinfo.d));
        ILUPP_HIP(hipEventRecord(S.tev[1], bs));
        // the call's one host wait in front of the numeric launch: all result records with one read-back
        ILUPP_HIP(hipMemcpyAsync(S.cinfo.h, S.cinfo.d, sizeof(CreateInfo) * (size_t)nc, hipMemcpyDeviceToHost, bs));
        ILUPP_HIP(stream_sync(bs));
        ILUPP_HIP(hipEventElapsedTime(&sym_ms, S.tev[0], S.tev[1]));
        for (int32_t k = 0; k < nc; ++k) {
            const int32_t i = cand[(size_t)k];
            const CreateInfo &o = S.cinfo.h[k];
            ilupp_precond *p = objs[(size_t)i];
            if (o.flags & kCreateNnzDiffers) {
                C.fail(i, ILUPP_ERR_INVALID, std::string(K.name) + ": the number of stored entries handed in is not indptr[n]");
            } else if (o.flags & kCreateUnsorted) {
                rt[(size_t)i] = 1;
            } else if (o.missing >= 0) {
                C.fail(i, ILUPP_ERR_NO_DIAGONAL, std::string(K.name) + ": structurally missing diagonal entry in row " + std::to_string(o.missing));
            } else {
                if (K.fits(m[i].n, o.max_row_len) == 0) { rt[(size_t)i] = 1; continue; }
                // exact index and value arrays, and what the object records of the factored matrix
                p->Lc.nnz = o.nnz_l; p->Uc.nnz = o.nnz_u;
                for (DevMat *M : {&p->Lc, &p->Uc}) {
                    if (K.llt && M == &p->Uc) continue;
                    ILUPP_HIP(pool_malloc(&M->idx, sizeof(int32_t) * (size_t)M->nnz));
                    ILUPP_HIP(pool_malloc(&M->val, sizeof(double) * (size_t)M->nnz));
                }
                p->nnzA = m[i].nnz; p->max_row_len = o.max_row_len; p->csr_vals = true; p->batch_built = true;
                launched.push_back(i);
            }
        }
    }
    const int32_t nl = C.failed ? 0 : (int32_t)launched.size();
    if (nl > 0) {
        // (this table is what the batched re-factorisation of the same members from the same buffers describes: its cache may hit)
        fresh.clear();
        size_t lds = 0;
        for (int32_t i : launched) {
            const ilupp_precond *p = objs[(size_t)i];
            fresh.push_back(refactor_desc(K, p, m[i].data, m[i].indices, m[i].indptr, p->nnzA, i));
            const size_t want = K.fits(m[i].n, p->max_row_len);
            if (want > lds) lds = want;
        }
        batch_upload(bs, S.rtable, fresh);
        ILUPP_HIP(hipEventRecord(S.tev[2], bs));
        OR_RETURN(K.create_launch(bs, nl, S.rtable.d, S.cstat.d, lds));
        ILUPP_HIP(hipEventRecord(S.tev[3], bs));
        // whatever a member's own stream does next (an apply, factors(), ensure_*) comes after the launch that writes its factors
        ILUPP_HIP(hipEventRecord(S.done_ev, bs));
        for (int32_t i : launched) ILUPP_HIP(hipStreamWaitEvent(objs[(size_t)i]->stream, S.done_ev, 0));
    }
    C.singles([&](int32_t i, ilupp_precond **made) { return K.create_single(m[i], is_csr, staged, S.in_ev, made); });
    if (nl > 0) {
        // a construction synchronises: the launch is over when the call returns
        std::vector<int32_t> st((size_t)count, 0);
        ILUPP_HIP(d2h_async(bs, st.data(), S.cstat.d, sizeof(int32_t) * (size_t)count));
        ILUPP_HIP(stream_sync(bs));
        ILUPP_HIP(hipEventElapsedTime(&create_ms, S.tev[2], S.tev[3]));
        for (int32_t i : launched) {
            ilupp_precond *p = objs[(size_t)i];
            if (st[(size_t)i] == 2) C.fail(i, ILUPP_ERR_TIMEOUT, std::string(K.name) + ": dependency wait timed out (invalid structure?)");
            else if (st[(size_t)i] != 0) C.fail(i, ILUPP_ERR_INVALID, std::string(K.name) + ": the matrix changed while it was factored");
            // (the two launches' times, shared by the call's members)
            p->tm.analysis_ms = sym_ms; p->tm.numeric_ms = create_ms; p->tm.numeric_kernel_ms = create_ms;
        }
    }
    return C.report(out, status, route);
}

// the object a single constructor inside a batched construction fills, its stream behind the upload of a staged matrix (nullptr: no stream)
ilupp_precond *single_obj(const CreateMember &m, bool staged, hipEvent_t in_ev)
{
    ilupp_precond *made = new_obj(m.n);
    if (staged && hipStreamWaitEvent(made->stream, in_ev, 0) != hipSuccess) { destroy_obj(made); (void)no_batch_stream(); return nullptr; }
    return made;
}

int ilu0_create_single(const CreateMember &m, int is_csr, bool staged, hipEvent_t in_ev, ilupp_precond **out)
{
    if (staged) {
        int32_t head[10];
        host_head(m.h_indptr, m.h_indices, m.nnz, head);
        ilupp_precond *made = single_obj(m, true, in_ev);
        if (!made) return ILUPP_ERR_HIP;
        return ilu0_create_common(borrow_csr(m.data, m.indices, m.indptr, m.n, m.nnz, true), is_csr, head, out, made);
    }
    const int rc = ilu0_create_device_locked(m.data, m.indices, m.indptr, m.n, is_csr, out);
    if (rc == ILUPP_OK && (*out)->nnzA != m.nnz) { set_error("ILU0: the number of stored entries handed in is not indptr[n]"); return ILUPP_ERR_INVALID; }
    return rc;
}

// the single constructor of `name`'s kind on a borrowed matrix: the count of stored entries checked where nothing staged it, then
// common(A, made)
template <class Common>
int borrowed_create_single(const char *name, const CreateMember &m, bool staged, hipEvent_t in_ev, Common &&common)
{
    if (!staged && (int64_t)read_device_nnz(m.indptr, m.n) != m.nnz) {
        set_error(std::string(name) + ": the number of stored entries handed in is not indptr[n]");
        return ILUPP_ERR_INVALID;
    }
    ilupp_precond *made = single_obj(m, staged, in_ev);
    if (!made) return ILUPP_ERR_HIP;
    DevMat A = borrow_csr(m.data, m.indices, m.indptr, m.n, m.nnz, true);
    return common(A, made);
}

int ichol0_create_single(const CreateMember &m, int is_csr, bool staged, hipEvent_t in_ev, ilupp_precond **out)
{
    (void)is_csr;                                    // (as ilupp_hip_ichol0_create)
    return borrowed_create_single("IChol0", m, staged, in_ev, [&](DevMat &A, ilupp_precond *made) { return ichol0_create_common(A, m.n, out, made); });
}

// the arguments of the *_create_batch_device entries, then the run: run(scratch, count, members, is_csr, staged, out, status, route)
template <class Run>
int factor_create_batch_device(Run &&run, int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                               const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, ilupp_precond **out,
                               int32_t *status, int32_t *route)
{
    if (count < 0 || !d_data || !d_indices || !d_indptr || !n || !nnz || !out) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) { out[i] = nullptr; if (status) status[i] = ILUPP_OK; if (route) route[i] = 0; }
    std::vector<CreateMember> m((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        if (n[i] > 0) OR_RETURN(batch_matrix_arrays(d_data, d_indices, d_indptr, i));
        m[(size_t)i].data = d_data[i]; m[(size_t)i].indices = d_indices[i]; m[(size_t)i].indptr = d_indptr[i];
        m[(size_t)i].n = n[i]; m[(size_t)i].nnz = nnz[i];
    }
    if (count == 0) return ILUPP_OK;
    std::lock_guard<std::mutex> lk(g_batch_mu);
    return run(batch_scratch(), count, m.data(), is_csr, false, out, status, route);
}

// ... of the host-array entries: all members through ONE packed block, one upload
template <class Run>
int factor_create_batch_host(Run &&run, int32_t count, const double *const *data, const int32_t *const *indices,
                             const int32_t *const *indptr, const int32_t *n, int is_csr, ilupp_precond **out, int32_t *status, int32_t *route)
{
    if (count < 0 || !data || !indices || !indptr || !n || !out) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    for (int32_t i = 0; i < count; ++i) { out[i] = nullptr; if (status) status[i] = ILUPP_OK; if (route) route[i] = 0; }
    for (int32_t i = 0; i < count; ++i)
        if (n[i] > 0) OR_RETURN(batch_matrix_arrays(data, indices, indptr, i));
    if (count == 0) return ILUPP_OK;
    std::lock_guard<std::mutex> lk(g_batch_mu);
    BatchScratch &S = batch_scratch();
    // all members through ONE packed block, one upload: per member its values, then its indices and its row pointers (each padded to 8 bytes)
    std::vector<CreateMember> m((size_t)count);
    std::vector<size_t> at((size_t)count);
    size_t total = 0;
    auto words = [](int64_t ints) { return (size_t)((ints + 1) / 2); };
    for (int32_t i = 0; i < count; ++i) {
        m[(size_t)i].n = n[i];
        if (n[i] <= 0) continue;
        const int64_t nz = indptr[i][n[i]];
        m[(size_t)i].nnz = nz;
        if (nz < 0 || nz + (int64_t)n[i] > INT32_MAX) continue;      // (refused per member below; nothing of it is staged)
        at[(size_t)i] = total;
        total += (size_t)nz + words(nz) + words((int64_t)n[i] + 1);
    }
    S.stage.reserve(S.stream, total > 0 ? total : 1);
    for (int32_t i = 0; i < count; ++i) {
        CreateMember &c = m[(size_t)i];
        if (c.n <= 0 || c.nnz < 0 || c.nnz + (int64_t)c.n > INT32_MAX) continue;
        const size_t nz = (size_t)c.nnz, o_idx = at[(size_t)i] + nz, o_ptr = o_idx + words(c.nnz);
        memcpy(S.stage.h + at[(size_t)i], data[i], sizeof(double) * nz);
        memcpy(S.stage.h + o_idx, indices[i], sizeof(int32_t) * nz);
        memcpy(S.stage.h + o_ptr, indptr[i], sizeof(int32_t) * ((size_t)c.n + 1));
        c.data = S.stage.d + at[(size_t)i];
        c.indices = reinterpret_cast<const int32_t *>(S.stage.d + o_idx);
        c.indptr = reinterpret_cast<const int32_t *>(S.stage.d + o_ptr);
        c.h_indices = indices[i]; c.h_indptr = indptr[i];
    }
    if (total > 0) ILUPP_HIP(hipMemcpyAsync(S.stage.d, S.stage.h, sizeof(double) * total, hipMemcpyHostToDevice, S.stream));
    ILUPP_HIP(hipEventRecord(S.in_ev, S.stream));
    const int rc = run(S, count, m.data(), is_csr, true, out, status, route);
    // (the staged matrices are read by nothing once the call is over: every member's construction has been waited for)
    if (rc) (void)hipStreamSynchronize(S.stream);
    return rc;
}

// the run of an ILU(0) or IChol(0) construction, as the two entry shapes above take it
auto factor_run(const FactorBatchKind &K)
{
    return [&K](BatchScratch &S, int32_t count, const CreateMember *m, int is_csr, bool staged, ilupp_precond **out, int32_t *status, int32_t *route) {
        return factor_create_batch_run(K, S, count, m, is_csr, staged, out, status, route);
    };
}

// ---- many ILUT objects built at once: the rows of all members in one launch per LDS class (k_ilut_rows_batch, ilut_wp.hip), one read-back,
// one fill launch (ilut.hip) ----

// the single constructor inside a batched ILUT construction (route 1)
int ilut_create_single(const CreateMember &m, int is_csr, bool staged, hipEvent_t in_ev, int32_t max_fill_in, double threshold, ilupp_precond **out)
{
    return borrowed_create_single("ILUT", m, staged, in_ev,
                                  [&](DevMat &A, ilupp_precond *made) { return ilut_create_common(A, m.n, is_csr, max_fill_in, threshold, out, made); });
}

// the stream is idle when the scope ends, however it ends: the pool blocks declared before it go back only then
struct StreamIdle {
    hipStream_t s;
    ~StreamIdle() { (void)hipStreamSynchronize(s); }
};

// What the two entries of the batched ILUT construction do once the matrices are in device memory (count > 0; the caller holds the
// construction lock and the batch lock; staged as for factor_create_batch_run).  Steady state, on the scratch's stream: the descriptors and
// the ticket maps (two small uploads), the record initialisation of all members, the rows launch (two when the members' clamped budgets
// fall into both LDS classes), the count-and-scan launch, ONE read-back of the members' records, the index and value arrays from the pool,
// the fill launch.  Routes: 0 = built by the launches; 1 = built by ilut_create_single inside this call -- a batch of one, a clamped budget
// of the largest capacity class, a member whose record says status 3 (a row that fits no tier of the launch), or a call whose slabs would
// not fit the memory budget.  Failures as CreateShell reports them.
int ilut_create_batch_run(BatchScratch &S, int32_t count, const CreateMember *m, int is_csr, bool staged, int32_t max_fill_in, double threshold,
                          ilupp_precond **out, int32_t *status, int32_t *route)
{
    hipStream_t bs = S.stream;
    CreateShell C(S, count, m);
    std::vector<int32_t> &rt = C.rt;
    std::vector<ilupp_precond *> &objs = C.objs.v;
    std::vector<int32_t> cand;                       // the members of the launches
    std::vector<int32_t> pm((size_t)count, 1);       // the clamped budgets (ILUT.hpp:211-212)
    size_t slab_bytes = 0;
    int64_t rows = 0;
    auto rec_bytes = [](int32_t p) { return ((((size_t)4 + 4 * (size_t)p + 7) & ~(size_t)7) + 8 * (size_t)p + 127) & ~(size_t)127; };
    for (int32_t i = 0; i < count; ++i) {
        if (C.refused(i, "ILUT")) continue;
        const int32_t p = pm[(size_t)i] = std::min(std::max(max_fill_in, 1), m[i].n);
        if (count == 1 || ilut_batch_class(p) < 0 || cand.size() >= 65535) { rt[(size_t)i] = 1; continue; }
        cand.push_back(i);
        slab_bytes += (size_t)m[i].n * ((size_t)p * 12 + 4 + rec_bytes(p));
        rows += m[i].n;
    }
    // (the slabs of a call are held together: a call that asks for more than the single path's working arrays do takes the single path
    // member by member; the tickets of a launch are counted in 32 bits)
    if (slab_bytes > ((size_t)16 << 30) || rows > (int64_t)1 << 30) { for (int32_t i : cand) rt[(size_t)i] = 1; cand.clear(); }
    if (!staged) order_after_caller(bs, S.cev[0]);
    const int32_t nc = (int32_t)cand.size();
    const bool debug = getenv("ILUPP_DEBUG") != nullptr;
    if (nc > 0 && !C.failed) {
        PoolBlock b_Lri, b_Lrv, b_Llen, b_Urec, b_ctrl;
        IlutBatchWork work;
        StreamIdle idle{bs};                         // (declared last: the wait comes before the blocks above are given back)
        // the slabs of all members, one block per array; the control blocks behind one block of the launches' own (its words 0 and 1: the ticket counters)
        std::vector<size_t> oL((size_t)nc), oN((size_t)nc), oU((size_t)nc);
        size_t tL = 0, tN = 0, tU = 0;
        for (int32_t k = 0; k < nc; ++k) {
            const int32_t i = cand[(size_t)k];
            oL[(size_t)k] = tL; oN[(size_t)k] = tN; oU[(size_t)k] = tU;
            tL += (size_t)m[i].n * (size_t)pm[(size_t)i]; tN += (size_t)m[i].n; tU += (size_t)m[i].n * rec_bytes(pm[(size_t)i]);
        }
        ILUPP_HIP(b_Lri.alloc(sizeof(int32_t) * tL));
        ILUPP_HIP(b_Lrv.alloc(sizeof(double) * tL));
        ILUPP_HIP(b_Llen.alloc(sizeof(int32_t) * tN));
        ILUPP_HIP(b_Urec.alloc(tU));
        ILUPP_HIP(b_ctrl.alloc(128 * ((size_t)nc + 1)));
        std::vector<IlutBatchDesc> fresh((size_t)nc);
        std::vector<int32_t> nk((size_t)nc), cls[2];
        int64_t max_words = 0;
        int32_t max_n = 0;
        for (int32_t k = 0; k < nc; ++k) {
            const int32_t i = cand[(size_t)k], n = m[i].n, p = pm[(size_t)i];
            ilupp_precond *q = objs[(size_t)i] = new_obj(n);
            q->kind = KIND_LU; q->nnz_mode = NNZ_ILUT; q->input_csc = !is_csr;
            for (DevMat *M : {&q->Lc, &q->Uc}) {
                M->n = n; M->is_csr = true; M->owns = true;
                ILUPP_HIP(pool_malloc(&M->ptr, sizeof(int32_t) * (size_t)(n + 1)));
            }
            const size_t voff = ((size_t)4 + 4 * (size_t)p + 7) & ~(size_t)7, rec = rec_bytes(p);
            unsigned char *urec = b_Urec.as<unsigned char>() + oU[(size_t)k];
            IlutBatchDesc &d = fresh[(size_t)k];
            memset(&d, 0, sizeof(d));
            d.aptr = m[i].indptr; d.aidx = m[i].indices; d.aval = m[i].data;
            d.Lri = b_Lri.as<int32_t>() + oL[(size_t)k]; d.Lrv = b_Lrv.as<double>() + oL[(size_t)k]; d.Llen = b_Llen.as<int32_t>() + oN[(size_t)k];
            d.Ulen = reinterpret_cast<int32_t *>(urec); d.Uri = reinterpret_cast<int32_t *>(urec + 4); d.Urv = reinterpret_cast<double *>(urec + voff);
            d.ctrl = b_ctrl.as<int32_t>() + 32 * ((size_t)k + 1);
            d.lptr = q->Lc.ptr; d.uptr = q->Uc.ptr;
            d.ul = {(int32_t)(rec / 4), (int32_t)(rec / 8), (int32_t)(rec / 4)};
            d.n = n; d.p = p; d.vw = (int32_t)(voff / 8);
            nk[(size_t)k] = n;
            cls[ilut_batch_class(p)].push_back(k);
            max_words = std::max(max_words, (int64_t)n * d.ul.sv);
            max_n = std::max(max_n, n);
        }
        // the ticket maps of the (at most two) rows launches: round-robin over the members that still have rows.  ILUPP_ILUT_BATCH_ORDER=member
        // is the measurement's other order (profiles/r26_ilut_batch.txt): one member after the other.
        const char *order_env = getenv("ILUPP_ILUT_BATCH_ORDER");
        const bool member_major = order_env && strcmp(order_env, "member") == 0;
        std::vector<IlutBatchSeg> seg;
        std::vector<int32_t> order;
        int32_t seg0[3] = {0, 0, 0};
        int64_t tickets[2] = {0, 0};
        for (int c = 0; c < 2; ++c) {
            if (!cls[c].empty()) tickets[c] = ilut_batch_tickets(cls[c], nk, member_major, &seg, &order);
            seg0[c + 1] = (int32_t)seg.size();
        }
        std::vector<int32_t> tick(4 * seg.size() + order.size());
        memcpy(tick.data(), seg.data(), sizeof(IlutBatchSeg) * seg.size());
        memcpy(tick.data() + 4 * seg.size(), order.data(), sizeof(int32_t) * order.size());
        batch_upload(bs, S.ttable, fresh, false);
        batch_upload(bs, S.ttick, tick, false);
        S.tinfo.reserve(bs, (size_t)nc);
        int32_t *d_counters = b_ctrl.as<int32_t>();
        OR_RETURN(ilut_batch_init_launch(bs, nc, S.ttable.d, max_words, d_counters));
        OR_RETURN(ilut_batch_work(bs, tickets[0], tickets[1], &work));
        ILUPP_HIP(hipEventRecord(S.tev[0], bs));
        for (int c = 0; c < 2; ++c)
            OR_RETURN(ilut_rows_batch_launch(bs, c, S.ttable.d, reinterpret_cast<const IlutBatchSeg *>(S.ttick.d) + seg0[c], seg0[c + 1] - seg0[c],
                                             S.ttick.d + 4 * seg.size(), (int32_t)tickets[c], d_counters + c, threshold, work));
        ILUPP_HIP(hipEventRecord(S.tev[1], bs));
        // (queued unconditionally behind the rows: a member that failed has lengths within its slabs like every other)
        OR_RETURN(ilut_batch_count_launch(bs, nc, S.ttable.d, S.tinfo.d));
        // the call's one read-back
        ILUPP_HIP(hipMemcpyAsync(S.tinfo.h, S.tinfo.d, sizeof(IlutBatchInfo) * (size_t)nc, hipMemcpyDeviceToHost, bs));
        ILUPP_HIP(stream_sync(bs));
        float rows_ms = 0.f;
        ILUPP_HIP(hipEventElapsedTime(&rows_ms, S.tev[0], S.tev[1]));
        std::vector<int32_t> launched;
        for (int32_t k = 0; k < nc; ++k) {
            const int32_t i = cand[(size_t)k];
            const IlutBatchInfo &o = S.tinfo.h[k];
            ilupp_precond *q = objs[(size_t)i];
            if (debug)
                fprintf(stderr, "[ilupp] ilut_batch: member %d: %d of %d rows outgrew LDS (pool %d, U slots %d, kept %d), %d of them the pool-in-LDS tier too, status %d, rows launches %.3f ms\n",
                        i, o.outgrew, m[i].n, o.pool, o.uslots, o.kept, o.left_tier2, o.status, rows_ms);
            if (o.status == 3) { rt[(size_t)i] = 1; continue; }
            if (o.status != 0) { C.fail(i, ILUPP_ERR_TIMEOUT, "ILUT: dependency wait timed out"); continue; }
            if (o.zero_row >= 0) { C.fail(i, ILUPP_ERR_ZERO_PIVOT, "ILUT_heap: encountered zero pivot in row " + std::to_string(o.zero_row)); continue; }      // ILUT.hpp:269-270
            q->Lc.nnz = o.nnz_l; q->Uc.nnz = o.nnz_u;
            for (DevMat *M : {&q->Lc, &q->Uc}) {
                ILUPP_HIP(pool_malloc(&M->idx, sizeof(int32_t) * (size_t)(M->nnz > 0 ? M->nnz : 1)));
                ILUPP_HIP(pool_malloc(&M->val, sizeof(double) * (size_t)(M->nnz > 0 ? M->nnz : 1)));
            }
            q->max_row_len = o.max_row_len; q->csr_vals = true; q->batch_built = true;
            q->tm.numeric_ms = rows_ms; q->tm.numeric_kernel_ms = rows_ms;      // (the rows launches' time, shared by the call's members)
            IlutBatchDesc &d = fresh[(size_t)k];
            d.lidx = q->Lc.idx; d.lval = q->Lc.val; d.uidx = q->Uc.idx; d.uval = q->Uc.val;
            launched.push_back(i);
        }
        if (!C.failed && !launched.empty()) {
            batch_upload(bs, S.ttable, fresh, false);
            OR_RETURN(ilut_batch_fill_launch(bs, nc, S.ttable.d, max_n));
            // whatever a member's own stream does next (an apply, factors(), ensure_*) comes after the launch that writes its factors
            ILUPP_HIP(hipEventRecord(S.done_ev, bs));
            for (int32_t i : launched) ILUPP_HIP(hipStreamWaitEvent(objs[(size_t)i]->stream, S.done_ev, 0));
            // a construction synchronises: the launches are over when the call returns
            ILUPP_HIP(stream_sync(bs));
        }
    }
    C.singles([&](int32_t i, ilupp_precond **made) { return ilut_create_single(m[i], is_csr, staged, S.in_ev, max_fill_in, threshold, made); });
    return C.report(out, status, route);
}

auto ilut_run(int32_t max_fill_in, double threshold)
{
    return [=](BatchScratch &S, int32_t count, const CreateMember *m, int is_csr, bool staged, ilupp_precond **out, int32_t *status, int32_t *route) {
        return ilut_create_batch_run(S, count, m, is_csr, staged, max_fill_in, threshold, out, status, route);
    };
}

}  // namespace

extern "C" {

int ilupp_hip_ilu0_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, ilupp_precond **out,
                                       int32_t *status, int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_device(factor_run(kIlu0Batch), count, d_data, d_indices, d_indptr, n, nnz, is_csr, out, status, route);
    API_CATCH
}

int ilupp_hip_ilu0_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                const int32_t *n, int is_csr, ilupp_precond **out, int32_t *status, int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_host(factor_run(kIlu0Batch), count, data, indices, indptr, n, is_csr, out, status, route);
    API_CATCH
}

int ilupp_hip_ichol0_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                         const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, ilupp_precond **out,
                                         int32_t *status, int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_device(factor_run(kIchol0Batch), count, d_data, d_indices, d_indptr, n, nnz, is_csr, out, status, route);
    API_CATCH
}

int ilupp_hip_ichol0_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                  const int32_t *n, int is_csr, ilupp_precond **out, int32_t *status, int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_host(factor_run(kIchol0Batch), count, data, indices, indptr, n, is_csr, out, status, route);
    API_CATCH
}

int ilupp_hip_ilut_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, int32_t max_fill_in,
                                       double threshold, ilupp_precond **out, int32_t *status, int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_device(ilut_run(max_fill_in, threshold), count, d_data, d_indices, d_indptr, n, nnz, is_csr, out, status, route);
    API_CATCH
}

int ilupp_hip_ilut_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out, int32_t *status,
                                int32_t *route)
{
    API_TRY_BUILD
    return factor_create_batch_host(ilut_run(max_fill_in, threshold), count, data, indices, indptr, n, is_csr, out, status, route);
    API_CATCH
}

}  // extern "C"
