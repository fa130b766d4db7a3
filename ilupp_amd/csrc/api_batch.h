// ilupp_amd/csrc/api_batch.h -- what the two batched translation units of the host layer share and nothing else uses: api_batch.hip (the
// batched apply and the batched solves) and api_batch_build.hip (the batched re-factorisation and the batched first constructions).
// The scratch the batched entries keep per device with its growable arrays, a member as the batched kernels see it, the lock and the
// few steps both files take, the argument checks both run.  What crosses handle families goes in api_internal.h instead; everything
// here is hidden from the dynamic symbol table the same way (DESIGN_OTHER_PATHS.md section 4h.13).
#pragma once

#include "api_internal.h"

#pragma GCC visibility push(hidden)
namespace ilupp {

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
inline BatchMember batch_member(ilupp_ilucp *m, int transpose)
{
    BatchMember v;
    v.p = m->obj; v.owner = m; v.perm = m->perm; v.plain_first = pivot_plain_first(m, transpose); v.tmp = m->tmp; v.n = m->n;
    return v;
}
inline BatchMember batch_member(ilupp_precond *p, int transpose)
{
    BatchMember v;
    v.p = p; v.plain_first = transpose == 0; v.n = p->n;
    return v;
}
inline BatchMember batch_member(ilupp_ml *m, int transpose)
{
    BatchMember v;
    v.ml = m; v.plain_first = transpose == 0; v.n = m->n;
    return v;
}
// the object whose stream a member's own work is queued on (a multilevel member: the first level's, which the others borrow)
inline ilupp_precond *batch_stream_obj(const BatchMember &v) { return v.ml ? v.ml->obj[0] : v.p; }
// a launch that reads the member is recorded in `ev` (nullptr: it has been waited for)
inline void batch_mark(const BatchMember &v, hipEvent_t ev)
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

// ---- api_batch.hip: the lock of the batched entries and this device's scratch (made on first use); ILUPP_BATCH_APPLY_MAX_N applied to a
// launch's cap; the scratch's stream behind a member's own; the routes into the caller's array; the members marked behind a launch ----
extern std::mutex g_batch_mu;
BatchScratch &batch_scratch();
int64_t batch_env_cap(int64_t cap_n);
void batch_join(hipStream_t bs, ilupp_precond *p);
void routes_out(const std::vector<int32_t> &from, int32_t *route);
void batch_launched(BatchScratch &S, const BatchMember *members);

// ---- the argument checks both files run, all before any device call ----

// a handle that stands twice in `seen` (a member's scratch vector and its factors serve one launch at a time)
inline int batch_no_duplicates(std::vector<const void *> &seen)
{
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { set_error("a preconditioner appears twice in the batch"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

// the three arrays of member i's matrix
inline int batch_matrix_arrays(const double *const *d_data, const int32_t *const *d_indices, const int32_t *const *d_indptr, int32_t i)
{
    if (!d_data[i] || !d_indices[i] || !d_indptr[i]) { set_error("null argument"); return ILUPP_ERR_INVALID; }
    return ILUPP_OK;
}

// null arguments, a negative count, a null member, a member named twice, for a list of non-pivoting objects; null_ok: a null handle is a member without a preconditioner (the CG solve), any number of them.
// A multilevel object handed in as a member is named before anything reads it as an ilupp_precond.
inline int plain_batch_args(int32_t count, ilupp_precond *const *members, bool null_ok, const void *a, const void *b)
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

}  // namespace ilupp
#pragma GCC visibility pop
