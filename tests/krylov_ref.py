"""Plain references of the Krylov layer, independent of the package: numpy only, no torch, no import of ilupp_amd or of the oracle.

Every function takes a `dtype` (np.float64 or np.longdouble) and does all of its arithmetic in it; the float64 inputs are cast exactly.
A matrix is a CSR triple (data, indices, indptr) with sorted rows.  A vector argument is (n,) or an (n, k) block whose columns are
independent problems: every statement acts element by element, so column j of a block run has the bits of the same run of that column.

  cg, bicgstab          the 1-D loops of ilupp_amd/device.py statement for statement (CG: cg(); BiCGstab: the left-preconditioned loop
                        of bicgstab(), r, Ap and As all preconditioned); the iterate and the recurrence residual norm of every iteration
  csr_matvec            by rows, each row's products added in stored order
  ilu0, ichol0          row-wise IKJ on the pattern of A (L with a unit diagonal, stored last; U's diagonal first), and the row-wise
                        incomplete Cholesky factor of A's lower triangle (diagonal last)
  apply_lu, apply_llt   the two substitutions of L U and of L L^T
  block_dot_exact       the reduction shape that the header comment of block_krylov.hip documents, emulated in float64
  block_update          the five masked updates of k_block_update, one numpy statement per kernel statement
"""
import numpy as np


# ---- vectors ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    """column dot products, the products added in row order (a cumulative sum is sequential whatever the shape is)"""
    return np.cumsum(a * b, axis=0)[-1]


def _norm(a):
    return np.sqrt(_dot(a, a))


def as_csr(A, dtype, check=False):
    """(data in dtype, indices, indptr as int64) of a CSR triple; check: every row's columns increase"""
    data, indices, indptr = np.asarray(A[0], dtype=dtype), np.asarray(A[1], dtype=np.int64), np.asarray(A[2], dtype=np.int64)
    if check:
        inner = np.ones(indices.shape[0], dtype=bool)
        inner[indptr[:-1][indptr[:-1] < indices.shape[0]]] = False          # a row's first entry has no predecessor
        assert np.all(np.diff(indices)[inner[1:]] > 0), "rows must be sorted, without duplicates"
    return data, indices, indptr


def csr_matvec(A, x, dtype):
    """y = A x by rows in stored order: y[i] = (..(0 + a[p] x[j_p]) + a[p + 1] x[j_(p + 1)]) + ..; all rows advance together"""
    data, indices, indptr = as_csr(A, dtype)
    x = np.asarray(x, dtype=dtype)
    n = indptr.shape[0] - 1
    y = np.zeros((n,) + x.shape[1:], dtype=dtype)
    length = indptr[1:] - indptr[:-1]
    for t in range(int(length.max()) if n else 0):
        rows = np.nonzero(length > t)[0]
        at = indptr[rows] + t
        a = data[at] if x.ndim == 1 else data[at][:, None]
        y[rows] = y[rows] + a * x[indices[at]]
    return y


# ---- factorisations --------------------------------------------------------------------------------------------------------------
def ilu0(A, dtype):
    """(L, U), CSR triples on the pattern of A.  Row i: for every stored column k < i in increasing order, l_ik = w_ik / u_kk, then
    w_ij = w_ij - l_ik u_kj for the stored j > k of both rows, then w_ik = l_ik.  L = the l's and a unit diagonal (last), U = the rest
    (diagonal first)."""
    data, indices, indptr = as_csr(A, dtype, check=True)
    n = indptr.shape[0] - 1
    w = data.copy()
    diag_at = np.full(n, -1, dtype=np.int64)
    one = dtype(1)
    for i in range(n):
        lo, hi = indptr[i], indptr[i + 1]
        at = {int(indices[q]): q for q in range(lo, hi)}
        diag_at[i] = at[i]
        for q in range(lo, hi):
            k = int(indices[q])
            if k >= i:
                break
            l_ik = w[q] / w[diag_at[k]]
            for t in range(diag_at[k] + 1, indptr[k + 1]):             # row k right of its diagonal
                j = int(indices[t])
                if j in at:
                    w[at[j]] = w[at[j]] - l_ik * w[t]
            w[q] = l_ik
    Ld, Li, Lp, Ud, Ui, Up = [], [], [0], [], [], [0]
    for i in range(n):
        for q in range(indptr[i], indptr[i + 1]):
            (Ld if indices[q] < i else Ud).append(w[q])
            (Li if indices[q] < i else Ui).append(indices[q])
        Ld.append(one)
        Li.append(i)
        Lp.append(len(Li))
        Up.append(len(Ui))
    return ((np.array(Ld, dtype=dtype), np.array(Li, dtype=np.int64), np.array(Lp, dtype=np.int64)),
            (np.array(Ud, dtype=dtype), np.array(Ui, dtype=np.int64), np.array(Up, dtype=np.int64)))


def ichol0(A, dtype):
    """L, a CSR triple on the pattern of A's lower triangle (A's upper triangle is not read), A ~ L L^T, the diagonal last in its row:
    l_ij = (a_ij - sum_c l_ic l_jc) / l_jj over the stored c < j of both rows in increasing order, l_ii = sqrt(a_ii - sum_c l_ic^2)"""
    data, indices, indptr = as_csr(A, dtype, check=True)
    n = indptr.shape[0] - 1
    rows = np.repeat(np.arange(n), indptr[1:] - indptr[:-1])
    keep = indices <= rows
    Lp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
    Li, a = indices[keep], data[keep]
    L = np.zeros_like(a)
    for i in range(n):
        lo, hi = int(Lp[i]), int(Lp[i + 1])
        assert hi > lo and Li[hi - 1] == i, "row %d has no diagonal" % i
        mine = {}                                                      # column -> position, the finished entries of row i
        for q in range(lo, hi):
            j = int(Li[q])
            s = dtype(0)
            for t in range(int(Lp[j]), int(Lp[j + 1]) - 1):            # row j left of its diagonal
                c = int(Li[t])
                if c in mine:
                    s = s + L[mine[c]] * L[t]
            if j < i:
                L[q] = (a[q] - s) / L[Lp[j + 1] - 1]
                mine[j] = q
            else:
                L[q] = np.sqrt(a[q] - s)
    return L, Li, Lp


# ---- substitutions ---------------------------------------------------------------------------------------------------------------
def _forward_diag_last(T, x):
    """x[i] = (x[i] - t_ij x[j] ...) / t_ii, rows upwards, a row's entries in stored order"""
    data, indices, indptr = T
    for i in range(indptr.shape[0] - 1):
        for q in range(indptr[i], indptr[i + 1] - 1):
            x[i] = x[i] - data[q] * x[indices[q]]
        x[i] = x[i] / data[indptr[i + 1] - 1]


def _backward_diag_first(T, x):
    data, indices, indptr = T
    for i in range(indptr.shape[0] - 2, -1, -1):
        for q in range(indptr[i] + 1, indptr[i + 1]):
            x[i] = x[i] - data[q] * x[indices[q]]
        x[i] = x[i] / data[indptr[i]]


def _backward_transposed_diag_last(T, x):
    """solves T^T x = b with the rows of T: x[i] = x[i] / t_ii, then x[j] = x[j] - t_ij x[i] for the row's other entries"""
    data, indices, indptr = T
    for i in range(indptr.shape[0] - 2, -1, -1):
        x[i] = x[i] / data[indptr[i + 1] - 1]
        for q in range(indptr[i], indptr[i + 1] - 1):
            x[indices[q]] = x[indices[q]] - data[q] * x[i]


def apply_lu(L, U, x, dtype):
    """U^-1 (L^-1 x): a new array"""
    x = np.array(x, dtype=dtype)
    assert L[0].dtype == dtype and U[0].dtype == dtype
    _forward_diag_last(L, x)
    _backward_diag_first(U, x)
    return x


def apply_llt(L, x, dtype):
    """L^-T (L^-1 x): a new array"""
    x = np.array(x, dtype=dtype)
    assert L[0].dtype == dtype
    _forward_diag_last(L, x)
    _backward_transposed_diag_last(L, x)
    return x


# ---- the loops -------------------------------------------------------------------------------------------------------------------
def cg(A, b, iterations, dtype, prec=None, x0=None):
    """the loop of cg() in device.py.  Returns (xs, res, ||b||): the iterate and sqrt(r.r) of the recurrence residual after every
    iteration; res[m - 1] / ||b|| is what a check after iteration m compares with rtol"""
    A = as_csr(A, dtype)
    b = np.asarray(b, dtype=dtype)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=dtype)
    r = b - csr_matvec(A, x, dtype) if x0 is not None else b.copy()
    z = prec(r) if prec is not None else r.copy()
    p = z.copy()
    rz = _dot(r, z)
    xs, res = [], []
    for it in range(iterations):
        Ap = csr_matvec(A, p, dtype)
        alpha = rz / _dot(p, Ap)
        x = x + p * alpha
        r = r - Ap * alpha
        xs.append(x.copy())
        res.append(_norm(r))
        z = prec(r) if prec is not None else r
        rz_new = _dot(r, z)
        p = z + p * (rz_new / rz)
        rz = rz_new
    return xs, res, _norm(b)


def bicgstab(A, b, iterations, dtype, prec=None, x0=None):
    """the left-preconditioned loop of bicgstab() in device.py.  Returns (xs, res, ||r_0||), r the preconditioned residual"""
    A = as_csr(A, dtype)
    b = np.asarray(b, dtype=dtype)

    def pre(v):
        return prec(v) if prec is not None else v.copy()
    y = np.zeros_like(b) if x0 is None else np.array(x0, dtype=dtype)
    r0star = b.copy() if x0 is None else b - csr_matvec(A, y, dtype)
    r = pre(r0star)
    r0star = r.copy()
    p = r.copy()
    initial_res = _norm(r)
    xs, res = [], []
    for it in range(iterations):
        Ap = pre(csr_matvec(A, p, dtype))
        dot_r_r0star = _dot(r, r0star)
        alpha = dot_r_r0star / _dot(Ap, r0star)
        s = r - alpha * Ap
        As = pre(csr_matvec(A, s, dtype))
        omega = _dot(As, s) / _dot(As, As)
        y = y + alpha * p
        y = y + omega * s
        r = s - omega * As
        beta = (_dot(r, r0star) / dot_r_r0star) * (alpha / omega)
        p = p - omega * Ap
        p = beta * p + r
        xs.append(y.copy())
        res.append(_norm(r))
    return xs, res, initial_res


# ---- what the tests of the loops share -------------------------------------------------------------------------------------------
def preconditioner(kind, A, dtype):
    """None, or v -> M^-1 v with the factor of `kind` ("ILU0", "IChol0") built here in dtype"""
    if kind is None:
        return None
    if kind == "ILU0":
        L, U = ilu0(A, dtype)
        return lambda v: apply_lu(L, U, v, dtype)
    if kind == "IChol0":
        L = ichol0(A, dtype)
        return lambda v: apply_llt(L, v, dtype)
    raise ValueError(kind)


def rhs_block(A, seed):
    """(n, 5) float64: ones, normal times 1e4, uniform times 1e-6, A times a normal vector, one unit vector e_i.  i is the first row
    from n // 3 on with a j != i for which a_ij and a_ji are both stored: otherwise unpreconditioned BiCGstab breaks down in its second
    iteration in exact arithmetic (s_i = 0 after the first, then (A s)_i = 0 and r_i = (r, r0*) = 0), which is no recurrence to compare"""
    data, indices, indptr = as_csr(A, np.float64)
    n = indptr.shape[0] - 1
    stored = set(zip(np.repeat(np.arange(n), indptr[1:] - indptr[:-1]).tolist(), indices.tolist()))
    i = next(i for i in range(n // 3, n) if any(j != i and (j, i) in stored for j in indices[indptr[i]:indptr[i + 1]].tolist()))
    rng = np.random.default_rng(seed)
    cols = [np.ones(n), rng.standard_normal(n) * 1e4, rng.random(n) * 1e-6, csr_matvec(A, rng.standard_normal(n), np.float64),
            np.where(np.arange(n) == i, 1.0, 0.0)]
    return np.ascontiguousarray(np.column_stack(cols))


class Pair:
    """the same solve in long double and in float64: xld[m - 1], x64[m - 1] the iterates after m iterations, rel[m - 1] the long-double
    relative residuals a check after m iterations sees, dev[m - 1] = max over the rows of |x64 - xld| (per column of a block)"""

    def __init__(self, solver, A, kind, b, iterations, x0=None):
        loop = {"cg": cg, "bicgstab": bicgstab}[solver]
        self.xld, res, den = loop(A, b, iterations, np.longdouble, preconditioner(kind, A, np.longdouble), x0)
        self.x64 = loop(A, b, iterations, np.float64, preconditioner(kind, A, np.float64), x0)[0]
        self.rel = [r / den for r in res]
        self.dev = [np.max(np.abs(u - v), axis=0) for u, v in zip(self.x64, self.xld)]
        self.scale = [np.max(np.abs(x), axis=0) for x in self.xld]

    def bound(self, m):
        """8 times the largest deviation of the float64 run from the long-double run in the first m iterations (per column)"""
        return 8 * np.max(np.stack(self.dev[:m]), axis=0)

    def stop(self, rtol, maxiter):
        """(iterations, converged) of a run of at most maxiter iterations that checks after every one, by the long-double residuals
        (per column)"""
        rel = np.stack(self.rel[:maxiter])
        hit = rel <= rtol
        return np.where(hit.any(axis=0), hit.argmax(axis=0) + 1, maxiter), hit.any(axis=0)

    def margin(self, rtol, maxiter):
        """the smallest factor between rtol and a long-double relative residual that such a run looks at before it stops"""
        rel = np.stack(self.rel[:maxiter]).astype(np.float64).reshape(maxiter, -1)
        first = np.atleast_1d(self.stop(rtol, maxiter)[0])
        seen = np.concatenate([rel[:first[j], j] for j in range(rel.shape[1])])
        return float(np.min(np.maximum(seen / rtol, rtol / seen)))


# ---- the block kernels -----------------------------------------------------------------------------------------------------------
def _workgroup_sum(items, count):
    """items (G, L, k): the L ordered items of G workgroups, of which group g has the first count[g].  Each group: 256 partial sums,
    partial v = ((0.0 + item v) + item v + 256) + .., then sh[w] = sh[w] + sh[w + s] for s = 128 .. 1.  Returns sh[0], (G, k)."""
    G, L, k = items.shape
    sh = np.zeros((G, 256, k), dtype=np.float64)
    for base in range(0, L, 256):
        w = min(256, L - base)
        live = (base + np.arange(w))[None, :] < count[:, None]
        part = sh[:, :w]
        part[live] = part[live] + items[:, base:base + w][live]
    s = 128
    while s:
        sh[:, :s] = sh[:, :s] + sh[:, s:2 * s]
        s >>= 1
    return sh[:, 0]


def block_dot_shape(n):
    """(nb, chunk) of ilupp_hip_block_dot_device for n rows"""
    nb = max(1, min(1024, -(-n // 256)))
    return nb, -(-n // nb)


def block_dot_exact(a, b):
    """the float64 result of ilupp_hip_block_dot_device for the columns a, b ((n,) -> a scalar, (n, k) -> (k,)): nb workgroups of
    `chunk` consecutive rows each, every one reduced by _workgroup_sum over its products (multiply and add separate), then the nb
    partial results reduced the same way by one finishing workgroup"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    one = a.ndim == 1
    if one:
        a, b = a[:, None], b[:, None]
    n, k = a.shape
    nb, chunk = block_dot_shape(n)
    prod = np.zeros((nb * chunk, k), dtype=np.float64)
    prod[:n] = a * b
    count = np.clip(n - np.arange(nb) * chunk, 0, chunk)
    partial = _workgroup_sum(prod.reshape(nb, chunk, k), count)
    out = _workgroup_sum(partial[None], np.array([nb]))[0]
    return out[0] if one else out


def block_update(solver, stage, active, c0, c1, c2, V0, V1, V2, V3, W0, W1):
    """k_block_update<solver> on (n, k) arrays, in place, columns with active[j] != 0 only; the arguments are the kernel's.
    "cg":       V0 = x, V1 = r, V2 = p, W0 = Ap (stage 0) or z (stage 1), c0 = alpha or beta.
    "bicgstab": V0 = y, V1 = r, V2 = p, V3 = s, W0 = Ap, W1 = As, c0 = alpha, c1 = omega, c2 = beta."""
    a = np.asarray(active).astype(bool)
    if solver == "cg":
        if stage == 0:
            pa = V2[:, a] * c0[a]
            V0[:, a] = V0[:, a] + pa
            apa = W0[:, a] * c0[a]
            V1[:, a] = V1[:, a] - apa
        elif stage == 1:
            pb = V2[:, a] * c0[a]
            V2[:, a] = W0[:, a] + pb
        else:
            raise ValueError(stage)
    elif solver == "bicgstab":
        if stage == 0:
            aap = c0[a] * W0[:, a]
            V3[:, a] = V1[:, a] - aap
        elif stage == 1:
            ap = c0[a] * V2[:, a]
            y = V0[:, a] + ap
            os = c1[a] * V3[:, a]
            y = y + os
            V0[:, a] = y
            oas = c1[a] * W1[:, a]
            V1[:, a] = V3[:, a] - oas
        elif stage == 2:
            oap = c1[a] * W0[:, a]
            p = V2[:, a] - oap
            bp = c2[a] * p
            V2[:, a] = bp + V1[:, a]
        else:
            raise ValueError(stage)
    else:
        raise ValueError(solver)
