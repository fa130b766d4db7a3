// ilupp_amd/csrc/api.hip -- the C ABI (include/ilupp_hip.h): object lifetime, dispatch of apply() to the sweep kernels, factor egress,
// the constructions of an ilupp_precond, the entries of no handle.  The other handle families have files of their own: api_pivot.hip
// (ILUCP / ILUTP), api_ml.hip (the multilevel preconditioner), api_batch.hip (batched apply and solves) and api_batch_build.hip (batched
// re-factorisation and construction); api_internal.h holds what the files share (DESIGN_OTHER_PATHS.md section 4h.13).  Mirrors the reference's binding layer (src/binding.cpp) and L2 dispatch (preconditioner_implementation.h:103-111,
// :321-334, :381-394).
#include "api_internal.h"

namespace ilupp {
std::mutex g_build_mu;

thread_local std::string g_last_error;
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

}  // namespace

// (the sweeps of an apply and what makes an object ready for them: what api_ml.hip and the batched files call is declared in
// api_internal.h, the rest is static)
namespace ilupp {

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
static void ensure_sweep_tables(ilupp_precond *p)
{
    if (!p->batch_built || p->sweeps_ready) return;
    int32_t longest = 0;
    // (a batch-built IChol(0) object: L forward, as ichol0_create_common builds it; the backward sweep's tables come with LcT)
    if (p->kind == KIND_LLT) p->compact = sweep_tables(p->stream, p, {&p->Lc, true, &p->sL, &p->dL}, {}, true, &longest);
    else p->compact = sweep_tables(p->stream, p, {&p->Lc, true, &p->sL, &p->dL}, {&p->Uc, false, &p->sU, &p->dU}, true, &longest);
    p->sweeps_ready = true;
}

// ---- the sweeps of an apply -----------------------------------------------------------------------------------------------------------
// (SweepOp, SweepParts, ApplyPlan: api_internal.h)
SweepParts sweep_parts(ilupp_precond *p, SweepOp op)
{
    switch (op.slot) {
    // (an LU object's L has A's strictly-lower pattern, hence A's forward cuts: the factor-sweep schedule serves it)
    case 0: return {p->Lc, (p->kind == KIND_LU && !p->sL.start) ? p->sA : p->sL, p->dL, p->max_row_len, &p->pkL, &p->pack_tried[0], &p->lvl[0]};
    case 1: return {p->Uc, p->sU, p->dU, p->max_row_len, &p->pkU, &p->pack_tried[1], &p->lvl[1]};
    case 2: return {p->UcT, p->sUT, p->dUT, p->max_len_T, &p->pkUT, &p->pack_tried[2], &p->lvl[2]};
    default: return {p->LcT, p->sLT, p->dLT, p->max_len_T, &p->pkLT, &p->pack_tried[3], &p->lvl[3]};
    }
}

ApplyPlan apply_plan(int kind, bool transpose, bool input_csc, bool llt_diag_last)
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
ApplyPlan apply_plan(const ilupp_precond *p, int transpose) { return apply_plan(p->kind, transpose != 0, p->input_csc, p->llt_diag_last); }

// one sweep: the packed kernel when the factor has a verified level-major form, else the CSR kernels.  Either way
// the right-hand side buffer is all-sentinel afterwards (the CSR kernels reset it row by row).
// level-major records of a sweep straight from its CSR arrays and descriptors (any object whose rows are short enough:
// transposed ILU(0) factors, IChol(0)); tried once, on first use
const PackedSweep *packed(ilupp_precond *p, SweepOp op)
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

int sweep(ilupp_precond *p, SweepOp op, const PackedSweep *ps, double *rhs, double *out, int32_t *ticket, int32_t *err,
                 double *ypk_out, const double *ypk_in, const int32_t *ysrc)
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
ApplyRoute prepare_apply(ilupp_precond *p, const ApplyPlan &plan, PackedSweep **pf, PackedSweep **pb)
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

}  // namespace

// (the single ILU(0) / IChol(0) constructions and re-factorisations: api_batch_build.hip runs them for the members that stay out of its
// launches)
namespace ilupp {

int ilu0_create_common(const DevMat &A, int is_csr, const int32_t *head, ilupp_precond **out, ilupp_precond *made)
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

}  // namespace ilupp

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

int ilut_create_common(DevMat &A, int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out,
                              ilupp_precond *made)
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

}  // namespace ilupp

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

namespace ilupp {

int ichol0_create_common(DevMat &A, int32_t n, ilupp_precond **out, ilupp_precond *made)
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

}  // namespace ilupp

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
