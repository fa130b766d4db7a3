// ilupp_amd/csrc/api_batch_build.hip -- the batched re-factorisation of ILU(0) and IChol(0) objects and the batched first constructions
// of ILU(0), IChol(0) and ILUT objects (ilu0_batch.hip, ichol0_batch.hip, ilut_wp.hip, ilut.hip): the launches' host scaffolds, the single
// constructors they run for the members that stay out of the launches, and the entries.  The scratch and what api_batch.hip uses too:
// api_batch.h.  (Host layer: api.hip; DESIGN_OTHER_PATHS.md 4h.13.)
#include "api_batch.h"

namespace {

// n up to which a member goes to the re-factorisation's and the construction's launches: one flag word per row of LDS
int64_t refactor_batch_max_n() { return batch_env_cap(ilu0_refactor_batch_max_n()); }

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

// the launch of the batched re-factorisation with this one member: the single re-factorisation of a batch-built object (api.hip:
// ilu0_refactor_single, ichol0_refactor_single), which has none of the single numeric paths' tables
namespace ilupp {

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

}  // namespace ilupp

// ---- many ILU(0) or IChol(0) objects built at once: a symbolic launch, one read-back, a create launch (ilu0_batch.hip, ichol0_batch.hip) ----
namespace {

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
