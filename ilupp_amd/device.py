"""GPU-resident Krylov building blocks: the preconditioners of this package and a CSR
operator that work on torch tensors living in HBM, so that an iteration of CG / BiCGstab / GMRES never crosses PCIe.

    import torch, ilupp_amd.device as ild
    A = ild.DeviceCSR.from_scipy(A_scipy)                  # one H2D copy
    M = ild.DevicePreconditioner("ICholT", A, add_fill_in=0, threshold=0.0)
    x = ild.cg(A, b, M, maxiter=50)                        # b, x: torch.float64 tensors on the GPU

k right-hand sides at once: B of shape (n, k), row-major; the k recurrences advance in lockstep, each iteration one SpMM, one block
apply and the block dot products, and column j of the result has the bits of the same solve of B[:, j:j+1] alone.

    B = torch.randn(A.n, 8, dtype=torch.float64, device="cuda")
    stats = {}
    X = ild.cg(A, B, M, maxiter=500, rtol=1e-8, check_every=10, stats=stats)
    stats["iterations"], stats["converged"], stats["relres"]        # (8,) each, on the CPU

Everything is ordered on torch's current stream (ilupp_hip_set_caller_stream): no host synchronisation per call.
The reference's counterpart is the loop of iterative_solvers_implementation.h:385-530 around
matrix_sparse::matrix_vector_multiplication (sparse_implementation.h:2733-2760) and apply_preconditioner_only.
"""
import torch

from . import _native

_FACTORIES = {
    "ILU0": (_native.ILU0Preconditioner_device, ()),
    "ILUT": (_native.ILUTPreconditioner_device, ("fill_in", "threshold")),
    "IChol0": (_native.IChol0Preconditioner_device, ()),
    "ICholT": (_native.ICholTPreconditioner_device, ("add_fill_in", "threshold")),
    "ILUC": (_native.ILUCPreconditioner_device, ("fill_in", "threshold")),
    "ILUpp": (_native.MultilevelILUCDPPreconditioner_device, ("params",)),     # params: an iluplusplus_precond_parameter (no default: see ILUppPreconditioner)
}
_DEFAULTS = {"ILUT": {"fill_in": 100, "threshold": 0.1}, "ICholT": {"add_fill_in": 0, "threshold": 0.0},
             "ILUC": {"fill_in": 100, "threshold": 0.1}}


def _on_current_stream():
    _native.set_caller_stream(torch.cuda.current_stream().cuda_stream, True)


def _check_block(X, n, name, contiguous=True):
    """a row-major fp64 (n, k) device tensor (unit column stride; with contiguous=False a leading dimension >= k is allowed): its leading
    dimension.  ValueError otherwise -- raised before any native call"""
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] != n:
        raise ValueError("%s: expected a 2-D tensor with %d rows, got shape %s" % (name, n, tuple(getattr(X, "shape", ()))))
    if X.dtype != torch.float64:
        raise ValueError("%s: expected torch.float64, got %s" % (name, X.dtype))
    k = X.shape[1]
    ld = X.stride(0) if n > 1 else max(k, 1)
    if contiguous:
        if not X.is_contiguous():
            raise ValueError("%s: expected a contiguous (row-major) tensor" % name)
        ld = k
    elif (k > 1 and X.stride(1) != 1) or ld < max(k, 1):
        raise ValueError("%s: expected row-major storage (unit column stride, leading dimension >= k)" % name)
    if not X.is_cuda:
        raise ValueError("%s: expected a CUDA tensor" % name)
    return ld


def _block_dot(A, B, out=None):
    """(k,) device tensor: column j = the dot product of A[:, j] and B[:, j] (ilupp_hip_block_dot_device: the reduction shape depends on
    n alone, so column j has the same bits whatever k is)"""
    n, k = A.shape
    out = torch.empty(k, dtype=torch.float64, device=A.device) if out is None else out
    if k:
        rc = _native.lib().ilupp_hip_block_dot_device(n, k, A.data_ptr(), k, B.data_ptr(), k, out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream)
        if rc:
            _native._raise(rc)
    return out


def _ok(v):
    """the scalars a recurrence may divide by: non-zero and finite"""
    return (v != 0) & torch.isfinite(v)


class DeviceCSR:
    """a square CSR matrix in HBM (fp64 values, int32 indices) with a bit-exact matvec"""

    def __init__(self, data, indices, indptr):
        assert data.is_cuda and data.dtype == torch.float64 and indices.dtype == torch.int32 and indptr.dtype == torch.int32
        self.data, self.indices, self.indptr = data.contiguous(), indices.contiguous(), indptr.contiguous()
        self.n = indptr.numel() - 1
        self.nnz = data.numel()
        self.shape = (self.n, self.n)

    @classmethod
    def from_scipy(cls, A, device=None):
        import numpy as np
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        A.sort_indices()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        return cls(torch.from_numpy(np.ascontiguousarray(A.data, dtype=np.float64)).to(dev),
                   torch.from_numpy(A.indices.astype(np.int32)).to(dev), torch.from_numpy(A.indptr.astype(np.int32)).to(dev))

    def matvec(self, x, out=None):
        if x.dim() == 2:
            return self.matmat(x, out=out)
        y = torch.empty_like(x) if out is None else out
        rc = _native.lib().ilupp_hip_spmv_device(self.data.data_ptr(), self.indices.data_ptr(), self.indptr.data_ptr(), self.n,
                                                 self.nnz, x.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc:
            _native._raise(rc)
        return y

    def matmat(self, X, out=None):
        """Y = A X for a row-major fp64 (n, k) CUDA tensor (contiguous, or a row-major view with a leading dimension >= k, such as
        X[:, c0:c1] of a wider block), ordered on torch's current stream.  Column j of Y has the bits of matvec(X[:, j]).  `out`: a
        row-major (n, k) tensor that does not overlap X.  ValueError for a wrong shape, dtype or layout, before any native call."""
        ldx = _check_block(X, self.n, "X", contiguous=False)
        k = X.shape[1]
        if out is None:
            Y, ldy = torch.empty((self.n, k), dtype=torch.float64, device=X.device), k
        else:
            if tuple(out.shape) != (self.n, k):
                raise ValueError("out: expected shape %s, got %s" % ((self.n, k), tuple(out.shape)))
            Y, ldy = out, _check_block(out, self.n, "out", contiguous=False)
        if k == 0:
            return Y
        rc = _native.lib().ilupp_hip_spmm_device(self.data.data_ptr(), self.indices.data_ptr(), self.indptr.data_ptr(), self.n, self.nnz,
                                                 X.data_ptr(), ldx, Y.data_ptr(), ldy, k, torch.cuda.current_stream().cuda_stream)
        if rc:
            _native._raise(rc)
        return Y

    __matmul__ = matvec


class DevicePreconditioner:
    """ILU0 / ILUT / ILUC / IChol0 / ICholT / multilevel ILU++ of a DeviceCSR, applied to device tensors in place or out of place"""

    def __init__(self, kind, A, **params):
        make, names = _FACTORIES[kind]
        p = dict(_DEFAULTS.get(kind, {}))
        p.update(params)
        _on_current_stream()
        self.pr = make(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.n, True, *[p[k] for k in names])
        self.kind = kind
        self.n = A.n
        self.shape = A.shape

    @classmethod
    def batch(cls, kind, As):
        """``[DevicePreconditioner(kind, A) for A in As]`` from ONE native call, for MANY SMALL matrices: ``As`` is a list of DeviceCSR,
        ``kind`` must be "ILU0" (the one class whose pattern does not depend on the values and which has a re-factorisation to share a
        kernel with).  Two kernel launches of one workgroup per matrix around one read-back (ilupp_hip_ilu0_create_batch_device) where
        the loop pays the single constructor's analysis and host waits per object; factors and every apply of a member have the bits
        of the singly built object.  The members go into ``apply_batch_`` / ``cg_batch`` / ``bicgstab_batch`` / ``refactor_batch_``
        (always route 0 there) as they are; the tables of the single ``apply_`` are built at a member's first one, and ``refactor_``
        runs the batched launch with that one member.  A matrix above the launches' caps (n above
        ``_native.ilu0_refactor_batch_max_n()``, a row of more than 31 entries), one with an unsorted row, and a batch of one are built
        by the single constructor inside the same call.  Ordered on torch's current stream; the call returns when every member is
        built.  A matrix without a diagonal entry in some row raises the constructor's RuntimeError, named by its number, and no object
        is returned.  (IChol(0) has a batched construction under a name of its own: ``ichol0_batch``.)  NotImplementedError for any other kind, TypeError for a member that is not a DeviceCSR -- before any native call;
        an empty list gives ``[]``."""
        if kind != "ILU0":
            raise NotImplementedError("DevicePreconditioner.batch: only the \"ILU0\" kind has a batched construction, not %s" % (kind,))
        As = list(As)
        for A in As:
            if not isinstance(A, DeviceCSR):
                raise TypeError("DevicePreconditioner.batch takes DeviceCSR matrices, got %s" % type(A).__name__)
        if not As:
            return []
        _on_current_stream()
        natives = _native.ILU0Preconditioner_batch_device(
            [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.n, A.nnz) for A in As], True)
        out = []
        for A, pr in zip(As, natives):
            M = cls.__new__(cls)
            M.pr, M.kind, M.n, M.shape = pr, kind, A.n, A.shape
            out.append(M)
        return out

    def apply_(self, x, transpose=False):
        """in place on a contiguous fp64 device tensor; asynchronous, ordered on torch's current stream.  A tensor of shape (n, k) is
        k right-hand sides, solved in one block apply (every column as apply_ on that column gives it; not for the "ILUpp" kind)"""
        if x.dim() == 2:
            if self.kind == "ILUpp":
                raise NotImplementedError("block apply of the multilevel preconditioner: apply_ one column at a time")
            assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.shape[0] == self.n
            _on_current_stream()
            self.pr.apply_block_device(x.data_ptr(), self.n, x.shape[1], transpose=transpose, sync=False)
            return x
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.numel() == self.n
        _on_current_stream()
        self.pr.apply_device(x.data_ptr(), self.n, transpose=transpose, sync=False)
        return x

    def matvec(self, x):
        return self.apply_(x.clone())

    __matmul__ = matvec

    def apply_part_(self, x, left, transpose=False):
        """the left or the right half of a split preconditioner in place (multilevel ILU++ objects only)"""
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.numel() == self.n
        _on_current_stream()
        self.pr.apply_part_device(x.data_ptr(), self.n, left, transpose=transpose, sync=False)
        return x

    def refactor_(self, A):
        """the numeric phase again on a DeviceCSR with the SAME pattern and (possibly) new values, the analysis kept
        (ilupp_hip_ilu0_refactor_device); ordered on torch's current stream, the host waits for the new factor.  "ILU0" only:
        NotImplementedError for any other kind; ValueError for a matrix of another dimension -- before any native call.  A matrix whose
        number of stored entries differs from the analysed one's is refused by the library (RuntimeError).  Many small members at once:
        ``refactor_batch_``.  (IChol(0): ``ichol0_refactor_`` / ``ichol0_refactor_batch_``.)"""
        if self.kind != "ILU0":
            raise NotImplementedError("refactor_: only the \"ILU0\" kind has a numeric re-factorisation, not %s" % self.kind)
        if not isinstance(A, DeviceCSR):
            raise TypeError("refactor_ takes a DeviceCSR, got %s" % type(A).__name__)
        if A.n != self.n:
            raise ValueError("refactor_: the matrix has dimension %d, the preconditioner %d" % (A.n, self.n))
        _on_current_stream()
        self.pr.refactor_device(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr())
        return self

    def sync(self):
        self.pr.sync()


def pivot_apply_batch_(members, x, offsets, transpose=False):
    """The applies of many ``ilupp_amd.ILUCPPreconditioner`` / ``ILUTPPreconditioner`` objects (mixed at will) in place on ONE contiguous
    fp64 CUDA tensor: member k's vector is ``x[offsets[k] : offsets[k] + n_k]``; what lies between the vectors is left untouched.  One
    kernel launch for all members that fit (``ilupp_hip_pivot_apply_batch_device``), ordered on torch's current stream, no host
    synchronisation.  Returns the route of every member (0 = the launch, 1 = too large, 2 = a factor with an empty row: applied alone
    inside the same call).  ValueError for a wrong tensor, unequal lengths or a vector that does not lie inside ``x``; TypeError for a
    member of another class -- before any native call.  Out of scope: ``DevicePreconditioner("ILUTP" / "ILUCP")`` (construction from device
    arrays).  The multilevel class has a batched apply of its own: ``ml_apply_batch_``.  The whole preconditioned BiCGstab solve of many systems in one launch:
    ``bicgstab_batch``."""
    def native(P):
        pr = getattr(P, "pr", P)
        if not isinstance(pr, _native.PivotedPreconditioner):
            raise TypeError("pivot_apply_batch_ takes ILUCPPreconditioner / ILUTPPreconditioner instances of the ctypes binding, got %s"
                            % type(P).__name__)
        return pr

    return _apply_batch(members, x, offsets, transpose, entry=_native.pivot_apply_batch_device, native=native)


class _HostBuiltOperator:
    """what PivotedOperator, MultilevelOperator and FactorOperator share: the apply of ``self.pr`` (dimension ``self.n``) on device tensors"""

    _block = False          # k right-hand sides in one apply_ (FactorOperator); else one column at a time, and
    _whose = ""             # ... the NotImplementedError names the class

    def apply_(self, x, transpose=False):
        """in place on a contiguous fp64 CUDA tensor of shape (n,) or (n, 1) -- (n, k) for a FactorOperator --; asynchronous, ordered on
        torch's current stream"""
        if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.shape[0] != self.n:
            raise ValueError("x: expected a tensor of shape (%d,) or (%d, %s), got %s"
                             % (self.n, self.n, "k" if self._block else "1", tuple(getattr(x, "shape", ()))))
        if x.dim() == 2 and x.shape[1] != 1 and not self._block:
            raise NotImplementedError("k right-hand sides with %s preconditioner: apply_ one column at a time" % self._whose)
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous():
            raise ValueError("x: expected a contiguous torch.float64 CUDA tensor")
        _on_current_stream()
        if x.dim() == 2 and self._block:
            self.pr.apply_block_device(x.data_ptr(), self.n, x.shape[1], transpose=transpose, sync=False)
        else:
            self.pr.apply_device(x.data_ptr(), self.n, transpose=transpose, sync=False)
        return x

    def matvec(self, x):
        return self.apply_(x.clone())

    __matmul__ = matvec

    def sync(self):
        """wait for what was queued on torch's current stream (the applies are ordered on it)"""
        torch.cuda.current_stream().synchronize()


class PivotedOperator(_HostBuiltOperator):
    """An ``ilupp_amd.ILUCPPreconditioner`` / ``ILUTPPreconditioner`` (built on the host by the ctypes binding) as the ``M`` of ``cg`` /
    ``bicgstab``: ``apply_`` works in place on a device tensor through the single device apply (ilupp_hip_ilucp_apply_device), ordered on
    torch's current stream.  One right-hand side at a time: shape (n,) or (n, 1).  ``bicgstab(A, b[:, None], M=PivotedOperator(P))`` is
    the solve every member of ``bicgstab_batch`` has the bits of.  Not ``DevicePreconditioner("ILUCP")``: these classes are not constructed
    from device arrays."""

    _whose = "a pivoting"

    def __init__(self, P):
        pr = getattr(P, "pr", P)
        if not isinstance(pr, _native.PivotedPreconditioner):
            raise TypeError("PivotedOperator takes an ILUCPPreconditioner / ILUTPPreconditioner instance of the ctypes binding, got %s"
                            % type(P).__name__)
        self.P, self.pr = P, pr
        self.kind = "ILUTP" if pr._rows else "ILUCP"
        self.n = pr._n
        self.shape = (self.n, self.n)


def _ml_native(P):
    """the native object of a multilevel member: an ``ilupp_amd.ILUppPreconditioner`` of the ctypes binding, a
    ``DevicePreconditioner("ILUpp", ...)`` or a ``MultilevelOperator``; None for anything else -- no native call"""
    if isinstance(P, DevicePreconditioner) and getattr(P, "kind", None) != "ILUpp":
        return None
    pr = getattr(P, "pr", P)
    return pr if isinstance(pr, _native.MultilevelPreconditioner) else None


class MultilevelOperator(_HostBuiltOperator):
    """A multilevel ILU++ preconditioner -- an ``ilupp_amd.ILUppPreconditioner`` (built on the host by the ctypes binding, alone or by
    ``ILUppPreconditioner.batch``) or a ``DevicePreconditioner("ILUpp", ...)`` -- as the ``M`` of ``bicgstab`` with a 2-D right-hand side
    and as a member of ``bicgstab_batch``: the sibling of ``PivotedOperator``.  ``apply_`` works in place on a device tensor through the
    single device apply (ilupp_hip_ml_apply_device), ordered on torch's current stream.  One right-hand side at a time: shape (n,) or
    (n, 1).  ``bicgstab(A, b[:, None], M=MultilevelOperator(P))`` is the solve every such member of ``bicgstab_batch`` has the bits of.
    TypeError for any other class."""

    kind = "ILUppOperator"       # (not "ILUpp": the block loops of cg / bicgstab take this wrapper, with k = 1)
    _whose = "the multilevel"

    def __init__(self, P):
        pr = None if isinstance(P, MultilevelOperator) else _ml_native(P)
        if pr is None:
            raise TypeError("MultilevelOperator takes an ILUppPreconditioner instance of the ctypes binding or a "
                            "DevicePreconditioner of the \"ILUpp\" kind, got %s" % type(P).__name__)
        self.P, self.pr = P, pr
        self.n = pr._n
        self.shape = (self.n, self.n)


def ml_apply_batch_(members, x, offsets, transpose=False):
    """The applies of many multilevel ILU++ preconditioners in place on ONE contiguous fp64 CUDA tensor: member k's vector is
    ``x[offsets[k] : offsets[k] + n_k]``; what lies between the vectors is left untouched.  Members: ``ilupp_amd.ILUppPreconditioner``
    objects of the ctypes binding, ``DevicePreconditioner("ILUpp", ...)`` objects or ``MultilevelOperator``s, mixed at will, each at
    most once.  One kernel launch for all members that fit (``ilupp_hip_ml_apply_batch_device``: one workgroup per member walks its
    levels up and down), ordered on torch's current stream, no host synchronisation.  Every member's vector has the bits of its single
    ``apply_``.  Returns the route of every member (0 = the launch, 1 = too large, 2 = a level's factor with an empty row: applied alone
    inside the same call).  ValueError for a wrong tensor, unequal lengths or a vector that does not lie inside ``x``; TypeError for a
    member of another class -- before any native call.  The whole preconditioned BiCGstab solve of many systems in one launch:
    ``bicgstab_batch`` with ``MultilevelOperator`` members."""
    def native(P):
        pr = _ml_native(P)
        if pr is None:
            raise TypeError("ml_apply_batch_ takes ILUppPreconditioner instances of the ctypes binding, DevicePreconditioners of the "
                            "\"ILUpp\" kind or MultilevelOperators, got %s" % type(P).__name__)
        return pr

    return _apply_batch(members, x, offsets, transpose, entry=_native.ml_apply_batch_device, native=native)


def bicgstab_batch(As, b, offsets, Ms, x0=None, maxiter=100, rtol=0.0, check_every=0, stats=None):
    """Left-preconditioned BiCGstab for MANY small systems in ONE kernel launch (one workgroup per system runs the whole loop -- SpMV,
    apply, dot products, updates, convergence test -- with no host round trip).

    ``As``: a list of DeviceCSR; ``Ms``: as many members, each of them an ``ilupp_amd.ILUCPPreconditioner`` / ``ILUTPPreconditioner``
    object or a ``PivotedOperator``; or anything ``cg_batch`` takes (a ``DevicePreconditioner`` of the ILU0 / ILUT / ILUC / IChol0 /
    ICholT kinds, a ``FactorOperator`` or a host class of the ctypes binding); or a ``MultilevelOperator`` (a multilevel ILU++ object in
    its wrapper); or ``None`` (no preconditioner) -- mixed at will, each object at most once.  A batch without a multilevel member goes
    through ilupp_hip_bicgstab_batch_device (k_bicgstab_batch, which takes the other kinds of member in the same launch); one with a
    multilevel member through ilupp_hip_bicgstab_batch_ml_device, whose launch is a second instantiation of that kernel with the
    multilevel apply as a choice on the member's descriptor and an LDS cap of its own (``_native.bicgstab_batch_ml_max_n()``).  ``b``: ONE contiguous 1-D fp64 CUDA tensor, member k's right-hand side is
    ``b[offsets[k] : offsets[k] + n_k]``; ``x0``: the same layout.  Returns a new tensor of b's shape, a clone of ``x0`` or zeros, whose
    member slices hold the solutions; every other element is untouched.  Per member the loop of ``bicgstab`` for one column: ``maxiter``,
    ``rtol`` and ``check_every`` mean what they mean there, a member that converges or breaks down stops alone, and every member has the
    bits of ``bicgstab(A_k, b_k[:, None], M_k, ...)`` (``M_k`` in a ``PivotedOperator`` / ``FactorOperator`` where it has no ``apply_``).
    ``stats``, when a dict, receives "iterations" (int64), "converged" (bool), "relres" (float64: sqrt(r.r) / ||r_0|| of the
    preconditioned residuals, 0 for a zero member) -- `count` entries each, on the CPU -- and "route" (a list: 0 = solved in the launch,
    1 = n above the launch's LDS cap, 2 = degenerate factor; members of routes 1 and 2 are solved by that single solve inside the same
    call).  Ordered on torch's current stream; the host waits only when ``stats`` is asked for or a member takes route 1 or 2, so
    ``refactor_batch_(check=False)`` -> ``bicgstab_batch`` -> ``refactor_batch_`` runs without a host wait.  ValueError for a wrong
    tensor, lists of unequal length, a slice outside ``b`` or a matrix and a preconditioner of different dimensions; TypeError for a
    member of another class or a bare multilevel object (the "ILUpp" kind, ``ILUppPreconditioner``: wrap it in a
    ``MultilevelOperator``) -- before any native call.  Out of scope: a transposed solve, host (numpy) vectors, several right-hand sides
    per member."""
    As, Ms, offsets = list(As), list(Ms), [int(o) for o in offsets]
    natives, dims = [], []
    for A in As:
        if not isinstance(A, DeviceCSR):
            raise TypeError("bicgstab_batch takes DeviceCSR matrices, got %s" % type(A).__name__)
    for M in Ms:
        if M is None:
            natives.append(None)
            continue
        if isinstance(M, MultilevelOperator):
            natives.append(M.pr)
            continue
        pr = M.pr if isinstance(M, PivotedOperator) else getattr(M, "pr", M)
        if not isinstance(pr, _native.PivotedPreconditioner):
            try:
                pr = _factor_native(M, "bicgstab_batch")[0]
            except TypeError:
                raise TypeError("bicgstab_batch takes ILUCPPreconditioner / ILUTPPreconditioner instances of the ctypes binding or "
                                "PivotedOperators, ILU0 / ILUT / ILUC / IChol0 / ICholT preconditioners (DevicePreconditioners of those "
                                "kinds, FactorOperators or the host classes), MultilevelOperators or None, got %s"
                                % type(M).__name__) from None
        natives.append(pr)
    if not (len(As) == len(Ms) == len(offsets)):
        raise ValueError("%d matrices, %d preconditioners and %d offsets" % (len(As), len(Ms), len(offsets)))
    for name, t in (("b", b), ("x0", x0)):
        if t is None and name == "x0":
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("%s: expected a contiguous 1-D torch.float64 CUDA tensor" % name)
    if x0 is not None and x0.shape != b.shape:
        raise ValueError("x0: expected shape %s, got %s" % (tuple(b.shape), tuple(x0.shape)))
    for k, (A, M, pr, o) in enumerate(zip(As, Ms, natives, offsets)):
        n = A.n if pr is None else pr._n if isinstance(pr, (_native.PivotedPreconditioner, _native.MultilevelPreconditioner)) else _factor_n(M, pr)
        if A.n != n:
            raise ValueError("member %d: the matrix has dimension %d, the preconditioner %d" % (k, A.n, n))
        if o < 0 or o + n > b.numel():
            raise ValueError("a vector of %d elements at offset %d does not lie inside b (%d elements)" % (n, o, b.numel()))
        dims.append(n)
    # (a batch with a multilevel member: the entry with the third handle list, whose launch is the kernel's second instantiation)
    has_ml = any(isinstance(pr, _native.MultilevelPreconditioner) for pr in natives)
    return _solve_batch(bicgstab, _native.bicgstab_batch_ml_device if has_ml else _native.bicgstab_batch_device, 7, "init", As, Ms, natives,
                        dims, b, offsets, x0, maxiter, rtol, check_every, stats)


def _solve_batch(single, entry, work_factor, relres, As, Ms, natives, dims, b, offsets, x0, maxiter, rtol, check_every, stats):
    """``bicgstab_batch`` / ``cg_batch`` behind their argument checks: the result tensor, the workspace of ``work_factor`` doubles per
    unknown and the per-member outputs, the launch through ``entry`` (``_native.bicgstab_batch_device`` / ``cg_batch_device``) on torch's
    current stream, ``single`` (``bicgstab`` / ``cg``) for the members of routes 1 and 2, and the stats.  ``relres`` names the launch's last
    per-member word, which sqrt(r.r) is divided by: "init", BiCGstab's ||r_0|| (0 where flag 8 marks a zero member), or "bnorm", CG's
    ||b|| (0 where it is 0; 1 for a member that was not launched)."""
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    count = len(natives)
    if count == 0:
        if isinstance(stats, dict):
            stats.update(iterations=torch.zeros(0, dtype=torch.int64), converged=torch.zeros(0, dtype=torch.bool),
                         relres=torch.zeros(0, dtype=torch.float64), route=[])
        return x
    work = torch.empty(work_factor * sum(dims), dtype=torch.float64, device=b.device)
    iters = torch.zeros(count, dtype=torch.int64, device=b.device)
    flags = torch.zeros(count, dtype=torch.int32, device=b.device)
    rr = torch.zeros(count, dtype=torch.float64, device=b.device)
    last = (torch.zeros if relres == "init" else torch.ones)(count, dtype=torch.float64, device=b.device)
    matrices = [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.nnz) for A in As]
    _on_current_stream()
    route = entry(natives, dims, matrices, b.data_ptr(), 0 if x0 is None else x0.data_ptr(), x.data_ptr(), offsets, work.data_ptr(),
                  work.numel(), maxiter, rtol, check_every, iters.data_ptr(), flags.data_ptr(), rr.data_ptr(), last.data_ptr(), sync=False)
    alone = {}
    for k, rt in enumerate(route):
        if rt == 0:
            continue
        # too large for the launch or degenerate: the single solve, whose bits the launch's members have
        o, n = offsets[k], dims[k]
        M = Ms[k]
        if M is not None and not hasattr(M, "apply_"):
            M = PivotedOperator(M) if isinstance(natives[k], _native.PivotedPreconditioner) else FactorOperator(M)
        st = {}
        xk = single(As[k], b[o:o + n][:, None], M, x0=None if x0 is None else x0[o:o + n][:, None], maxiter=maxiter, rtol=rtol,
                    check_every=check_every, stats=st)
        x[o:o + n] = xk[:, 0]
        alone[k] = st
    if isinstance(stats, dict):
        zero = (flags & 8) != 0 if relres == "init" else last == 0
        rel = torch.sqrt(rr) / last                      # as _bicgstab_block / _cg_block computes it
        rel = torch.where(zero, torch.zeros_like(rel), rel).cpu()
        its, conv = iters.cpu(), ((flags & 2) != 0).cpu()
        for k, st in alone.items():
            its[k], conv[k], rel[k] = st["iterations"][0], st["converged"][0], st["relres"][0]
        stats["iterations"], stats["converged"], stats["relres"], stats["route"] = its, conv, rel, route
    return x


_FACTOR_KINDS = ("ILU0", "ILUT", "ILUC", "IChol0", "ICholT")


def _factor_native(P, who):
    """the native object and the kind of a non-pivoting member: a DevicePreconditioner of the five kinds, a FactorOperator, or a host-built
    ILU0 / ILUT / ILUC / IChol0 / ICholT Preconditioner of the ctypes binding.  TypeError for anything else -- no native call"""
    if isinstance(P, FactorOperator):
        return P.pr, P.kind
    if isinstance(P, DevicePreconditioner):
        if getattr(P, "kind", None) not in _FACTOR_KINDS:
            raise TypeError("%s: the multilevel (\"ILUpp\") class is not a member of a batch" % who)
        return P.pr, P.kind
    pr = getattr(P, "pr", P)
    if isinstance(pr, _native.PivotedPreconditioner):
        raise TypeError("%s takes the non-pivoting classes; ILUCPPreconditioner / ILUTPPreconditioner go through pivot_apply_batch_ / "
                        "bicgstab_batch (which takes both families in one batch)" % who)
    kind = type(P).__name__[:-len("Preconditioner")] if type(P).__name__.endswith("Preconditioner") else ""
    if not isinstance(pr, _native.Preconditioner) or (pr is not P and kind not in _FACTOR_KINDS):
        raise TypeError("%s takes ILU0 / ILUT / ILUC / IChol0 / ICholT preconditioners of the ctypes binding, DevicePreconditioners of "
                        "those kinds or FactorOperators, got %s" % (who, type(P).__name__))
    return pr, kind if kind in _FACTOR_KINDS else "factor"


def _factor_n(P, pr):
    """the dimension of a member: what the wrapper knows, else the library's answer"""
    if hasattr(P, "n"):
        return int(P.n)
    if hasattr(P, "shape"):
        return int(P.shape[0])
    return int(_native.lib().ilupp_hip_dimension(pr._h))


class FactorOperator(_HostBuiltOperator):
    """An ``ilupp_amd.ILU0Preconditioner`` / ``ILUTPreconditioner`` / ``ILUCPreconditioner`` / ``IChol0Preconditioner`` /
    ``ICholTPreconditioner`` (built on the host by the ctypes binding) as the ``M`` of ``cg`` / ``bicgstab``: the counterpart of
    ``PivotedOperator`` for the non-pivoting classes.  ``apply_`` works in place on a device tensor of shape (n,) or (n, k) through
    ilupp_hip_apply_device / ilupp_hip_apply_block_device, ordered on torch's current stream.  ``cg(A, b[:, None], FactorOperator(P))``
    is the solve every member of ``cg_batch`` has the bits of, ``bicgstab(A, b[:, None], FactorOperator(P))`` the one every such member
    of ``bicgstab_batch`` has the bits of.  TypeError for any other class."""

    _block = True

    def __init__(self, P):
        if isinstance(P, (FactorOperator, DevicePreconditioner)):
            raise TypeError("FactorOperator takes a host-built ILU0 / ILUT / ILUC / IChol0 / ICholT preconditioner of the ctypes binding, "
                            "got %s" % type(P).__name__)
        pr, kind = _factor_native(P, "FactorOperator")
        self.P, self.pr, self.kind = P, pr, kind
        self.n = _factor_n(P, pr)
        self.shape = (self.n, self.n)


def _packed_vector(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError("%s: expected a contiguous 1-D torch.float64 CUDA tensor" % name)


def _on_device(t, name):
    if not t.is_cuda:
        raise ValueError("%s: expected a contiguous 1-D torch.float64 CUDA tensor" % name)


def _apply_batch(members, x, offsets, transpose, *, entry, native, size=lambda P, pr: pr._n, members_first=False):
    """what the three batched applies do through ``entry``: ``native(P)`` is a member's native object (TypeError for another class),
    ``size(P, pr)`` its dimension.  The checks run in the caller's order.  members_first: the member classes before the tensor, and whether the tensor
    lives on the device last of all -- else the tensor first, device and all, and the member classes behind the two lengths."""
    members, offsets = list(members), [int(o) for o in offsets]
    if members_first:
        natives = [native(P) for P in members]
    _packed_vector(x, "x")
    if not members_first:
        _on_device(x, "x")
    if len(members) != len(offsets):
        raise ValueError("%d preconditioners but %d offsets" % (len(members), len(offsets)))
    if not members_first:
        natives = [native(P) for P in members]
    for P, pr, o in zip(members, natives, offsets):
        n = size(P, pr)
        if o < 0 or o + n > x.numel():
            raise ValueError("a vector of %d elements at offset %d does not lie inside x (%d elements)" % (n, o, x.numel()))
    if members_first:
        _on_device(x, "x")
    if not natives:
        return []
    _on_current_stream()
    return entry(natives, x.data_ptr(), offsets, transpose=transpose, sync=False)


def apply_batch_(members, x, offsets, transpose=False):
    """``pivot_apply_batch_`` for the NON-pivoting classes: the applies of many ILU0 / ILUT / ILUC / IChol0 / ICholT objects in place on
    ONE contiguous fp64 CUDA tensor, member k's vector being ``x[offsets[k] : offsets[k] + n_k]``, with one kernel launch for all members
    that fit (``ilupp_hip_apply_batch_device``), ordered on torch's current stream.  Members: ``DevicePreconditioner`` objects of the
    five kinds, ``FactorOperator``s, or the host classes of the ctypes binding themselves, mixed at will, each at most once.  Every
    member's vector has the bits of its single ``apply_``.  Returns the routes (0 = the launch, 1 = too large, 2 = a factor with an empty
    row: applied alone inside the same call).  ValueError for a wrong tensor, unequal lengths or a vector that does not lie inside ``x``;
    TypeError for the "ILUpp" kind, a pivoting member or any other class -- before any native call."""
    return _apply_batch(members, x, offsets, transpose, entry=_native.apply_batch_device,
                        native=lambda P: _factor_native(P, "apply_batch_")[0], size=_factor_n, members_first=True)


def refactor_batch_(members, As, check=True):
    """The numeric ILU(0) re-factorisation of MANY small members in ONE kernel launch (ilupp_hip_ilu0_refactor_batch_device: one workgroup
    per member, its rows side by side): the members keep their patterns, schedules and tables and get the factors of ``As[k]``, a
    DeviceCSR with member k's pattern and new values -- the step in front of ``bicgstab_batch`` (nonsymmetric systems), ``cg_batch`` /
    ``apply_batch_`` when the values change and the patterns do not.  ``members``: as for ``apply_batch_`` but of the ILU0 kind only
    (``DevicePreconditioner("ILU0", ...)``, ``FactorOperator``s of, or the host class ``ILU0Preconditioner`` itself), each at most
    once.  Every member's factor has the bits of a fresh construction from ``As[k]`` (and of the single ``refactor_``).  Returns the routes: 0 = the launch; 1 = n above the launch's
    cap (``_native.ilu0_refactor_batch_max_n()``), a longest row above the row cap (31 entries, fewer where 4 n + 5 120 bytes per entry
    do not fit into a workgroup's LDS: 28 at n = 4 000), or a member that would have the launch to itself with n >= 1 000 (alone it is
    faster on the single path); 2 = static form.  Members of routes 1 and 2 are re-factorised alone inside the same call, with the
    single path's host waits.  Ordered on torch's current stream.  Inside the launch every member's pattern is PROVED equal to the analysed one row by row; a member
    whose pattern differs keeps its factor bitwise as it was (status 1), the others are re-factorised.  ``check=True`` reads the status
    words with one host wait and raises ValueError naming the first such member (RuntimeError for status 2, a dependency wait that gave
    up); ``check=False`` returns ``(routes, status)``, status an int32 CUDA tensor, and waits for nothing in the steady state (refactor_batch_
    -> ``bicgstab_batch`` / ``cg_batch`` / plain ``apply_batch_`` -> refactor_batch_ with all members on route 0): a call whose launched
    members still hold copies of the old values -- the packed sweeps a construction leaves, the packed / transposed / level-ordered
    sweeps of single or block applies -- waits once for its launch before it frees them, whatever the members' statuses turn out to be.  TypeError for a member of
    another kind or class, a pivoting member, the multilevel class or a matrix that is not a DeviceCSR; ValueError for lists of unequal
    length, a member named twice or a matrix and a member of different dimensions -- before any native call.  The batched FIRST
    construction of such members: ``DevicePreconditioner.batch("ILU0", As)`` / ``ilupp_amd.ILU0Preconditioner.batch`` (members built
    that way always take route 0 here).  IChol(0) members: ``ichol0_refactor_batch_``.  Out of scope: the other classes (no single
    re-factorisation to match), host (numpy) matrices."""
    return _refactor_batch("refactor_batch_", "ILU0", lambda *a, **k: _native.ilu0_refactor_batch_device(*a, **k), members, As, check)


def _refactor_batch(who, want, entry, members, As, check):
    """``refactor_batch_`` / ``ichol0_refactor_batch_`` for members of the kind ``want``: the argument checks, then ``entry``"""
    members, As = list(members), list(As)
    for A in As:
        if not isinstance(A, DeviceCSR):
            raise TypeError("%s takes DeviceCSR matrices, got %s" % (who, type(A).__name__))
    natives = []
    for P in members:
        pr, kind = _factor_native(P, who)
        if kind != want:
            raise TypeError("%s takes members of the %s kind only (DevicePreconditioner(\"%s\"), %sPreconditioner or a "
                            "FactorOperator of one), got %s" % (who, want, want, want, kind if kind != "factor" else type(P).__name__))
        natives.append(pr)
    if len(members) != len(As):
        raise ValueError("%d preconditioners but %d matrices" % (len(members), len(As)))
    if len(set(id(pr) for pr in natives)) != len(natives):
        raise ValueError("a preconditioner appears twice in the batch")
    for k, (P, pr, A) in enumerate(zip(members, natives, As)):
        if _factor_n(P, pr) != A.n:
            raise ValueError("member %d: the matrix has dimension %d, the preconditioner %d" % (k, A.n, _factor_n(P, pr)))
    if not natives:
        return [] if check else ([], torch.zeros(0, dtype=torch.int32))
    status = torch.zeros(len(natives), dtype=torch.int32, device=As[0].data.device)
    _on_current_stream()
    route = entry(
        natives, [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.nnz) for A in As], status.data_ptr(), sync=False)
    if not check:
        return route, status
    for k, v in enumerate(status.cpu().tolist()):                        # the one host wait
        if v == 1:
            raise ValueError("member %d of the batch: the matrix does not have the analysed pattern (its factor is unchanged)" % k)
        if v != 0:
            raise RuntimeError("member %d of the batch: %s: dependency wait timed out" % (k, want))
    return route


def ichol0_batch(As):
    """``[DevicePreconditioner("IChol0", A) for A in As]`` from ONE native call, for MANY SMALL symmetric positive definite matrices: what
    ``DevicePreconditioner.batch("ILU0", As)`` is for ILU(0).  Two kernel launches of one workgroup per matrix around one read-back
    (ilupp_hip_ichol0_create_batch_device) where the loop pays the single constructor's five host waits and dozen launches per object;
    the factor and every apply of a member have the bits of the singly built object.  The members go into ``apply_batch_`` / ``cg_batch``
    / ``ichol0_refactor_batch_`` as they are: the first ``cg_batch`` (or ``apply_batch_``) builds a member's transposed copy of the
    factor, and every ``ichol0_refactor_batch_`` after that keeps it current, so a loop of re-factorisation and ``cg_batch`` waits for
    nothing on the host.  A matrix above the launches' caps (n above ``_native.ichol0_refactor_batch_max_n()``, a row of L of more than 31
    entries -- 28 at n = 4 000), one with an unsorted row, and a batch of one are built by the single constructor inside the same call.
    Ordered on torch's current stream; the call returns when every member is built.  A matrix without a diagonal entry in some row raises
    the constructor's RuntimeError, named by its number, and no object is returned.  TypeError for a member that is not a DeviceCSR --
    before any native call; an empty list gives ``[]``."""
    As = list(As)
    for A in As:
        if not isinstance(A, DeviceCSR):
            raise TypeError("ichol0_batch takes DeviceCSR matrices, got %s" % type(A).__name__)
    if not As:
        return []
    _on_current_stream()
    natives = _native.IChol0Preconditioner_batch_device(
        [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.n, A.nnz) for A in As], True)
    out = []
    for A, pr in zip(As, natives):
        M = DevicePreconditioner.__new__(DevicePreconditioner)
        M.pr, M.kind, M.n, M.shape = pr, "IChol0", A.n, A.shape
        out.append(M)
    return out


def ilut_batch(As, fill_in=100, threshold=0.1):
    """``[DevicePreconditioner("ILUT", A, fill_in=fill_in, threshold=threshold) for A in As]`` from ONE native call, for MANY SMALL
    matrices (one parameter set per batch).  ILUT's pattern depends on the values, so there is nothing to re-factor: a time-stepping
    caller builds every member again at every step, and this is the call for that.  The rows of all members run in one launch of the
    single constructor's wave kernel, claimed round-robin so that the members' dependency chains advance side by side; one read-back,
    one fill launch (ilupp_hip_ilut_create_batch_device) where the loop pays five host waits, a nearly empty rows launch and the waves'
    working arrays per object.  The factors and every apply of a member have the bits of the singly built object; the members go into
    ``apply_batch_`` / ``cg_batch`` / ``bicgstab_batch`` as they are.  A batch of one, a budget min(fill_in, n) above 256 and a member
    with a row that outgrows the launch's 64 K pieces are built by the single constructor inside the same call.  Ordered on torch's
    current stream; the call returns when every member is built.  A zero pivot raises the constructor's RuntimeError, named by the
    member's number, and no object is returned.  TypeError for a member that is not a DeviceCSR -- before any native call; an empty
    list gives ``[]``."""
    As = list(As)
    for A in As:
        if not isinstance(A, DeviceCSR):
            raise TypeError("ilut_batch takes DeviceCSR matrices, got %s" % type(A).__name__)
    if not As:
        return []
    _on_current_stream()
    natives = _native.ILUTPreconditioner_batch_device(
        [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.n, A.nnz) for A in As], True, fill_in, threshold)
    out = []
    for A, pr in zip(As, natives):
        M = DevicePreconditioner.__new__(DevicePreconditioner)
        M.pr, M.kind, M.n, M.shape = pr, "ILUT", A.n, A.shape
        out.append(M)
    return out


def ichol0_refactor_(M, A):
    """The numeric IChol(0) factorisation again on a DeviceCSR with the SAME pattern and (possibly) new values, the analysis kept
    (ilupp_hip_ichol0_refactor_device); returns ``M``.  ``M``: a ``DevicePreconditioner("IChol0", ...)``, a host ``IChol0Preconditioner``
    of the ctypes binding or a ``FactorOperator`` of one.  The factor has the bits of a fresh construction from ``A``.  The pattern is
    PROVED equal to the analysed one (the lower triangle row by row; entries above the diagonal are ignored, as the constructor drops
    them): a matrix that differs is refused by the library (RuntimeError) and the factor stays as it was.  Ordered on torch's current
    stream, the host waits for the new factor; every copy of the old values (the transposed copy included) is rebuilt at its next use.
    Many small members at once, with the transposed copy kept current for ``cg_batch``: ``ichol0_refactor_batch_``.
    NotImplementedError naming the kind for any other member, TypeError for a matrix that is not a DeviceCSR, ValueError for a matrix
    of another dimension -- before any native call."""
    try:
        pr, kind = _factor_native(M, "ichol0_refactor_")
    except TypeError:
        pr, kind = None, getattr(M, "kind", type(M).__name__)
    if kind != "IChol0":
        raise NotImplementedError("ichol0_refactor_: the numeric IChol(0) re-factorisation takes the \"IChol0\" kind, not %s"
                                  % (kind if kind != "factor" else type(M).__name__))
    if not isinstance(A, DeviceCSR):
        raise TypeError("ichol0_refactor_ takes a DeviceCSR, got %s" % type(A).__name__)
    if _factor_n(M, pr) != A.n:
        raise ValueError("ichol0_refactor_: the matrix has dimension %d, the preconditioner %d" % (A.n, _factor_n(M, pr)))
    _on_current_stream()
    pr.ichol0_refactor_device(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr())
    return M


def ichol0_refactor_batch_(members, As, check=True):
    """The numeric IChol(0) re-factorisation of MANY small SPD members in ONE kernel launch (ilupp_hip_ichol0_refactor_batch_device: one
    workgroup per member, its rows side by side): what ``refactor_batch_`` is for ILU(0), in front of ``cg_batch``.  ``members``:
    ``DevicePreconditioner("IChol0", ...)`` objects (``ichol0_batch`` builds many at once), host ``IChol0Preconditioner``s of the ctypes
    binding or ``FactorOperator``s of them, each at most once; ``As[k]``: a DeviceCSR with member k's pattern and the new values.  Every
    member's factor has the bits of a fresh construction from ``As[k]`` (and of ``ichol0_refactor_``), NaN / Inf behind a negative or
    zero pivot included.
    For ``cg_batch`` users: the members go into ``apply_batch_`` / ``cg_batch`` as they are; the first ``cg_batch`` builds a member's
    transposed copy of the factor; every re-factorisation by this function after that writes the new values into that copy as well, so
    the loop re-factorisation -> ``cg_batch`` -> re-factorisation with all members on route 0 and ``check=False`` waits for nothing on
    the host and launches nothing per member.
    Returns the routes: 0 = the launch; 1 = n above the launch's cap (``_native.ichol0_refactor_batch_max_n()``), a longest row of L above
    the row cap (31 entries, fewer where 4 n + 5 120 bytes per entry do not fit into a workgroup's LDS: 28 at n = 4 000), or a member that
    would have the launch to itself and is faster alone; 2 = an object built by the static form.  Members of routes 1 and 2 are
    re-factorised by ``ichol0_refactor_``'s path inside the same call, with its host waits (their transposed copy is rebuilt at the next
    use).  Inside the launch every member's pattern is PROVED equal to the analysed one (entries above the diagonal are ignored); a
    member whose pattern differs keeps its factor and its transposed copy bitwise as they were (status 1), the others are re-factorised.
    ``check=True`` reads the status words with one host wait and raises ValueError naming the first such member (RuntimeError for status
    2); ``check=False`` returns ``(routes, status)``, status an int32 CUDA tensor.  A call whose launched members still hold packed or
    level-ordered copies of the old values (single or block applies leave them) waits once before it frees them.  TypeError for a member
    of another kind or class or a matrix that is not a DeviceCSR; ValueError for lists of unequal length, a member named twice or a
    matrix and a member of different dimensions -- before any native call."""
    return _refactor_batch("ichol0_refactor_batch_", "IChol0", lambda *a, **k: _native.ichol0_refactor_batch_device(*a, **k), members, As, check)


def cg_batch(As, b, offsets, Ms, x0=None, maxiter=100, rtol=0.0, check_every=0, stats=None):
    """Preconditioned conjugate gradients for MANY small symmetric positive definite systems in ONE kernel launch
    (ilupp_hip_cg_batch_device: one workgroup per system runs the whole loop -- SpMV, apply, dot products, updates, convergence test --
    with no host round trip).

    ``As``: a list of DeviceCSR; ``Ms``: as many members as for ``apply_batch_`` (``DevicePreconditioner`` objects of the ILU0 / ILUT /
    ILUC / IChol0 / ICholT kinds, ``FactorOperator``s or the host classes, mixed at will, each at most once) or ``None`` (no
    preconditioner); ``b``, ``x0``, ``offsets`` and the result as in ``bicgstab_batch``.  Per member the loop of ``cg`` for one column:
    ``maxiter``, ``rtol`` and ``check_every`` mean what they mean there, a member that converges or breaks down stops alone, and every
    member has the bits of ``cg(A_k, b_k[:, None], M_k, ...)``.  ``stats``, when a dict, receives "iterations" (int64), "converged"
    (bool), "relres" (float64: sqrt(r.r) / ||b||, 0 where ||b|| is 0) -- `count` entries each, on the CPU -- and "route" (0 = solved in
    the launch, 1 = n above the launch's LDS cap, 2 = degenerate factor; members of routes 1 and 2 are solved by that single solve
    inside the same call).  Ordered on torch's current stream; the host waits only when ``stats`` is asked for or a member takes route 1
    or 2.  ValueError for a wrong tensor, lists of unequal length, a slice outside ``b`` or a matrix and a preconditioner of different
    dimensions; TypeError for a member of another class -- before any native call.  Out of scope: the multilevel class, pivoting members
    (``bicgstab_batch``, which takes them next to everything this function takes, for nonsymmetric systems), k > 1 right-hand sides
    per member, host (numpy) vectors, a batched construction of the non-pivoting classes other than ILU(0)
    (``DevicePreconditioner.batch("ILU0", As)`` builds such members with two launches)."""
    As, Ms, offsets = list(As), list(Ms), [int(o) for o in offsets]
    for A in As:
        if not isinstance(A, DeviceCSR):
            raise TypeError("cg_batch takes DeviceCSR matrices, got %s" % type(A).__name__)
    natives = [None if M is None else _factor_native(M, "cg_batch")[0] for M in Ms]
    if not (len(As) == len(Ms) == len(offsets)):
        raise ValueError("%d matrices, %d preconditioners and %d offsets" % (len(As), len(Ms), len(offsets)))
    _packed_vector(b, "b")
    if x0 is not None:
        _packed_vector(x0, "x0")
        if x0.shape != b.shape:
            raise ValueError("x0: expected shape %s, got %s" % (tuple(b.shape), tuple(x0.shape)))
    for k, (A, M, pr, o) in enumerate(zip(As, Ms, natives, offsets)):
        if pr is not None and _factor_n(M, pr) != A.n:
            raise ValueError("member %d: the matrix has dimension %d, the preconditioner %d" % (k, A.n, _factor_n(M, pr)))
        if o < 0 or o + A.n > b.numel():
            raise ValueError("a vector of %d elements at offset %d does not lie inside b (%d elements)" % (A.n, o, b.numel()))
    _on_device(b, "b")
    if x0 is not None:
        _on_device(x0, "x0")
    return _solve_batch(cg, _native.cg_batch_device, 5, "bnorm", As, Ms, natives, [A.n for A in As], b, offsets, x0, maxiter, rtol,
                        check_every, stats)


def cg(A, b, M=None, x0=None, maxiter=100, rtol=0.0, check_every=0, stats=None):
    """preconditioned conjugate gradients on device tensors.  No host round trip per iteration: the scalars stay 0-dim
    device tensors; the residual is only looked at every `check_every` iterations (0 = never: run maxiter iterations).

    b of shape (n, k): k right-hand sides, k independent recurrences in lockstep, each column statement for statement the loop
    below (not a block Krylov space); one SpMM, one block apply and the block dot products per iteration.  Per column:
      - every `check_every` iterations one (k,) vector of relative residuals ||r|| / ||b|| is copied to the host; columns at or below
        `rtol` freeze (converged), and the loop ends when no column is active.  check_every = 0: every column runs maxiter iterations;
      - a zero right-hand-side column (or one whose x0 leaves a zero residual) returns x0's column (zeros) and counts as converged at
        iteration 0 -- the 1-D function gives NaN there;
      - a breakdown, p^T A p zero or not finite, freezes the column as not converged, without any host read;
      - a frozen column is bitwise untouched from then on, and a NaN in one column never reaches another;
      - column j of the result has the bits of the same solve of b[:, j:j+1] alone.
    `stats`, when a dict and b is 2-D, receives "iterations" (k,) int64, "converged" (k,) bool and "relres" (k,) float64 on the CPU.
    M of the "ILUpp" kind with a 2-D b: NotImplementedError."""
    if b.dim() == 2:
        return _cg_block(A, b, M, x0, maxiter, rtol, check_every, stats)
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    r = b - A.matvec(x) if x0 is not None else b.clone()
    z = M.matvec(r) if M is not None else r.clone()
    p = z.clone()
    rz = torch.dot(r, z)
    bnorm = torch.linalg.vector_norm(b)
    Ap = torch.empty_like(b)
    for it in range(maxiter):
        A.matvec(p, out=Ap)
        alpha = rz / torch.dot(p, Ap)
        x.add_(p * alpha)
        r.sub_(Ap * alpha)
        if check_every and (it + 1) % check_every == 0 and rtol > 0.0:
            if float(torch.linalg.vector_norm(r) / bnorm) <= rtol:      # the only device-to-host read
                break
        z = M.matvec(r) if M is not None else r
        rz_new = torch.dot(r, z)
        p = z + p * (rz_new / rz)
        rz = rz_new
    if M is not None:
        M.sync()
    return x


def bicgstab(A, b, M=None, x0=None, maxiter=100, rtol=0.0, check_every=0, history=None, stats=None):
    """left-preconditioned BiCGstab on device tensors, statement for statement the loop of the reference
    (iterative_solvers_implementation.h:385-530 with a LEFT preconditioner application): the residual recurrence runs on
    r = M^-1 (b - A x), Ap = M^-1 (A p), As = M^-1 (A s).  No host round trip per iteration (the scalars stay 0-dim device tensors;
    the residual norm is looked at every `check_every` iterations only); `history`, when a list, receives a copy of the iterate after
    every iteration (tests).

    b of shape (n, k): k right-hand sides as in cg() -- k recurrences in lockstep, each column statement for statement this loop; the
    relative residual of a column is ||r|| / ||r_0|| of the preconditioned residual, as here.  Per column:
      - every `check_every` iterations one (k,) vector of relative residuals is copied to the host; columns at or below `rtol` freeze
        (converged), and the loop ends when no column is active.  check_every = 0: every column runs maxiter iterations;
      - a zero right-hand-side column (or a zero initial residual) returns x0's column (zeros) and counts as converged at iteration 0
        -- the 1-D function gives NaN there;
      - a breakdown, rho = (r, r0*), (Ap, r0*) or omega zero or not finite, freezes the column as not converged, without any host read;
      - a frozen column is bitwise untouched from then on, and a NaN in one column never reaches another;
      - column j of the result has the bits of the same solve of b[:, j:j+1] alone.
    `stats` as in cg().  M of the "ILUpp" kind with a 2-D b: NotImplementedError."""
    if b.dim() == 2:
        return _bicgstab_block(A, b, M, x0, maxiter, rtol, check_every, history, stats)
    def prec(v):
        return M.matvec(v) if M is not None else v.clone()
    y = torch.zeros_like(b) if x0 is None else x0.clone()
    r0star = b.clone() if x0 is None else b - A.matvec(y)
    r = prec(r0star)
    r0star = r.clone()
    p = r.clone()
    initial_res = torch.linalg.vector_norm(r)
    Ap = torch.empty_like(b)
    As = torch.empty_like(b)
    for it in range(maxiter):
        Ap = prec(A.matvec(p))
        dot_r_r0star = torch.dot(r, r0star)
        alpha = dot_r_r0star / torch.dot(Ap, r0star)
        s = r - alpha * Ap
        As = prec(A.matvec(s))
        omega = torch.dot(As, s) / torch.dot(As, As)
        y.add_(alpha * p)
        y.add_(omega * s)
        r = s - omega * As
        beta = (torch.dot(r, r0star) / dot_r_r0star) * (alpha / omega)
        p.sub_(omega * Ap)
        p = beta * p + r
        if history is not None:
            history.append(y.clone())
        if check_every and (it + 1) % check_every == 0 and rtol > 0.0:
            if float(torch.linalg.vector_norm(r) / initial_res) <= rtol:      # the only device-to-host read
                break
    if M is not None:
        M.sync()
    return y


# ---- k right-hand sides: the 2-D paths of cg() and bicgstab() ---------------------------------------------------------------------
def _block_setup(A, B, M, x0):
    """the checks of a 2-D solve, all before any native call"""
    if M is not None and getattr(M, "kind", None) == "ILUpp":
        raise NotImplementedError("k right-hand sides with the multilevel preconditioner: solve one column at a time")
    n = A.n
    _check_block(B, n, "b")
    if x0 is not None:
        _check_block(x0, n, "x0")
        if x0.shape != B.shape:
            raise ValueError("x0: expected shape %s, got %s" % (tuple(B.shape), tuple(x0.shape)))
    if M is not None and M.n != n:
        raise ValueError("M: dimension %d, the matrix has %d" % (M.n, n))
    return n, B.shape[1]


def _block_update(solver, stage, n, k, active, *ptrs):
    lib = _native.lib()
    fn = lib.ilupp_hip_cg_block_update_device if solver == "cg" else lib.ilupp_hip_bicgstab_block_update_device
    rc = fn(stage, n, k, active.data_ptr(), *[0 if t is None else t.data_ptr() for t in ptrs], torch.cuda.current_stream().cuda_stream)
    if rc:
        _native._raise(rc)


def _block_stats(stats, iters, converged, relres):
    if isinstance(stats, dict):
        stats["iterations"] = iters.cpu()
        stats["converged"] = converged.cpu()
        stats["relres"] = relres.cpu()


def _check_point(R, den, active, converged, rtol):
    """freeze the columns at or below rtol; the one host read: the (k,) relative residuals of the columns still active (-1 for the
    others).  True when no column is active."""
    rel = torch.sqrt(_block_dot(R, R)) / den
    newly = active & (rel <= rtol)
    converged |= newly
    active &= ~newly
    h = torch.where(active, rel, torch.full_like(rel, -1.0)).cpu()
    return not bool((h != -1.0).any())


def _cg_block(A, B, M, x0, maxiter, rtol, check_every, stats):
    n, k = _block_setup(A, B, M, x0)
    X = torch.zeros_like(B) if x0 is None else x0.clone()
    R = B - A.matmat(X) if x0 is not None else B.clone()
    Z = M.apply_(R.clone()) if M is not None else R.clone()
    P = Z.clone()
    rz = _block_dot(R, Z)
    bnorm = torch.sqrt(_block_dot(B, B))
    zero = (bnorm == 0) | (_block_dot(R, R) == 0)
    active = ~zero
    converged = zero.clone()
    iters = torch.zeros(k, dtype=torch.int64, device=B.device)
    AP = torch.empty_like(B)
    for it in range(maxiter):
        A.matmat(P, out=AP)
        pap = _block_dot(P, AP)
        alpha = rz / pap
        active &= _ok(pap)                                               # breakdown: frozen, not converged
        _block_update("cg", 0, n, k, active, alpha, X, R, P, AP)         # x = x + p alpha; r = r - Ap alpha
        iters += active
        if check_every and (it + 1) % check_every == 0 and rtol > 0.0:
            if _check_point(R, bnorm, active, converged, rtol):
                break
        if M is not None:
            Z.copy_(R)
            M.apply_(Z)
        else:
            Z = R
        rz_new = _block_dot(R, Z)
        _block_update("cg", 1, n, k, active, rz_new / rz, None, None, P, Z)   # p = z + p (rz_new / rz)
        rz = rz_new
    if M is not None:
        M.sync()
    if isinstance(stats, dict):
        rel = torch.sqrt(_block_dot(R, R)) / bnorm
        _block_stats(stats, iters, converged, torch.where(bnorm == 0, torch.zeros_like(rel), rel))
    return X


def _bicgstab_block(A, B, M, x0, maxiter, rtol, check_every, history, stats):
    n, k = _block_setup(A, B, M, x0)

    def prec_(V):
        return M.apply_(V) if M is not None else V
    Y = torch.zeros_like(B) if x0 is None else x0.clone()
    R0s = B.clone() if x0 is None else B - A.matmat(Y)
    R = prec_(R0s)
    R0s = R.clone()
    P = R.clone()
    init = torch.sqrt(_block_dot(R, R))
    zero = (_block_dot(B, B) == 0) | (init == 0)
    active = ~zero
    converged = zero.clone()
    iters = torch.zeros(k, dtype=torch.int64, device=B.device)
    AP = torch.empty_like(B)
    AS = torch.empty_like(B)
    S = torch.zeros_like(B)
    for it in range(maxiter):
        prec_(A.matmat(P, out=AP))
        rho = _block_dot(R, R0s)
        apr = _block_dot(AP, R0s)
        active &= _ok(rho) & _ok(apr)                                    # breakdown: frozen, not converged
        alpha = rho / apr
        _block_update("bicgstab", 0, n, k, active, alpha, None, None, None, R, None, S, AP, None)     # s = r - alpha Ap
        prec_(A.matmat(S, out=AS))
        omega = _block_dot(AS, S) / _block_dot(AS, AS)
        active &= _ok(omega)
        # y = y + alpha p; y = y + omega s; r = s - omega As
        _block_update("bicgstab", 1, n, k, active, alpha, omega, None, Y, R, P, S, None, AS)
        beta = (_block_dot(R, R0s) / rho) * (alpha / omega)
        _block_update("bicgstab", 2, n, k, active, None, omega, beta, None, R, P, None, AP, None)        # p = p - omega Ap; p = beta p + r
        iters += active
        if history is not None:
            history.append(Y.clone())
        if check_every and (it + 1) % check_every == 0 and rtol > 0.0:
            if _check_point(R, init, active, converged, rtol):
                break
    if M is not None:
        M.sync()
    if isinstance(stats, dict):
        rel = torch.sqrt(_block_dot(R, R)) / init
        _block_stats(stats, iters, converged, torch.where(zero, torch.zeros_like(rel), rel))
    return Y


def bicgstab_split(A, b, M, min_iter=1, max_iter=500, rtol=1e-4, atol=1e-4):
    """BiCGstab with SPLIT preconditioning as the reference's `solve` runs it (solving_routines_implementation.h:81 ->
    iterative_solvers_implementation.h:385-530 from the zero vector): r = L' b, Ap = L'(A(R' p)), x = R' y at the end; the loop goes on
    while (res / initial_res > rtol or res > atol) and iter < max_iter, or iter < min_iter -- the residual is looked at after every
    iteration, as there.  Returns (x, iterations, res / initial_res, res).  M: a DevicePreconditioner of the "ILUpp" kind."""
    def pmv(v):
        w = M.apply_part_(v.clone(), left=False)
        return M.apply_part_(A.matvec(w), left=True)
    r = M.apply_part_(b.clone(), left=True)
    r0star = r.clone()
    p = r.clone()
    y = torch.zeros_like(b)
    initial_res = float(torch.linalg.vector_norm(r))
    res = initial_res
    it = 0
    # (IEEE division as the reference's doubles do it: a zero right-hand side gives 0 / 0 = NaN, every comparison with it is false, the
    # loop runs its min_iter iterations and the caller reports "did not converge" -- not a ZeroDivisionError)
    rel = lambda a, b: a / b if b != 0.0 else (float("nan") if (a == 0.0 or a != a) else float("inf"))
    while (((rel(res, initial_res) > rtol) or res > atol) and it < max_iter) or it < min_iter:
        it += 1
        Ap = pmv(p)
        dot_r_r0star = torch.dot(r, r0star)
        alpha = dot_r_r0star / torch.dot(Ap, r0star)
        s = r - alpha * Ap
        As = pmv(s)
        omega = torch.dot(As, s) / torch.dot(As, As)
        y.add_(alpha * p)
        y.add_(omega * s)
        r = s - omega * As
        beta = (torch.dot(r, r0star) / dot_r_r0star) * (alpha / omega)
        p.sub_(omega * Ap)
        p = beta * p + r
        res = float(torch.linalg.vector_norm(r))
    x = M.apply_part_(y, left=False)
    M.sync()
    return x, it, rel(res, initial_res), res
