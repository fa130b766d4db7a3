// ilupp_amd/csrc/api_batch.hip -- the batched apply and the batched solves of the C ABI: members of every handle type applied or solved
// in one launch (sptrsv_batch.hip), the describing passes that make the launches' tables, the argument checks and the entries.  The
// scratch, BatchMember and what api_batch_build.hip uses too: api_batch.h.  (Host layer: api.hip; DESIGN_OTHER_PATHS.md 4h.13.)
#include "api_batch.h"

// (what api_batch_build.hip calls too: declared in api_batch.h)
namespace ilupp {

std::mutex g_batch_mu;
static std::map<int, BatchScratch> g_batch_scratch;

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

// behind the launch: what touches a member's tmp or rewrites its factors comes after it (a pivoting member's later single apply, any
// member's re-factorisation and destruction)
void batch_launched(BatchScratch &S, const BatchMember *members)
{
    ILUPP_HIP(hipEventRecord(S.done_ev, S.stream));
    for (int32_t i : S.launched) batch_mark(members[i], S.done_ev);
}

}  // namespace ilupp

// ---- many members applied at once: one launch, one workgroup per member (k_pivot_apply_batch, sptrsv_batch.hip) ----
namespace {

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
