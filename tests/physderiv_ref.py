"""Reference and error bounds of BwdTrans fused with the physical-space gradient (include/sumfact.h sf_physderiv_*) for
tests/test_physderiv_cpu.py and tests/test_gpu_physderiv.py.  Imports nothing of the product.

    u = B x_e,   du_b = D_b u,   out_a[e][k][j][i] = sum_b df[e][a d + b][k][j][i] du_b[e][k][j][i]

B the tensor-product BwdTrans basis (bases nm x nq row-major), D_b row-major nq x nq with (D_b u)[i] = sum_m D_b[i][m]
u[m], df[e][c][k][j][i] the d*d planes of the inverse Jacobian, c = a d + b for d xi_b / d x_a (None: out_a = du_a).
Results have the shape (d, nelmt * nq^d): row a is out_a.

The reference runs sweep by sweep in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is negligible against
the bound.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),

    N = sum_d nq_d + max_d nq_d + d

-- the forward chain of inner products (sum nq_d), one derivative inner product (max nq_d), the d-term sum over b (d);
relative errors of chained operations compose additively, as in tests/helm_ref.py -- u = 2^-53 (fp64) or 2^-24 (fp32),
absref = the same operator applied to |B|, |D|, |df| and |x|.  The bound is derived, not tuned, holds for any summation
order, and is kept for df = None, where the last d operations do not happen.  A zero bound needs a zero error.
"""
import math

import numpy as np
from numpy.polynomial import legendre as _leg

from helm_ref import gll, legendre_basis
from iprod_ref import U32, U64, gamma, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps


def physderiv_n(nq):
    nq = [int(q) for q in nq]
    return sum(nq) + max(nq) + len(nq)


def _apply(a, M, f):
    """(M f) along direction a: out[.., i_a, ..] = sum_m M[i_a][m] f[.., m, ..]"""
    axis = f.ndim - 1 - a
    return np.moveaxis(np.moveaxis(f, axis, -1) @ M.T, -1, axis)


def _physderiv(nq, nelmt, bases, derivs, df, x, dt):
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    u = _forward_sweeps(nq, nelmt, bases, x, dt).reshape(shape)
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    du = [_apply(a, D[a], u) for a in range(dim)]
    if df is None:
        return np.stack([np.ascontiguousarray(d).reshape(-1) for d in du])
    dd = np.asarray(df, dtype=dt).reshape((nelmt, dim * dim) + shape[1:])
    out = []
    for a in range(dim):
        f = None
        for b in range(dim):
            term = dd[:, a * dim + b] * du[b]
            f = term if f is None else f + term
        out.append(np.ascontiguousarray(f).reshape(-1))
    return np.stack(out)


def _abs(a, dt):
    return None if a is None else np.abs(np.asarray(a, dtype=dt))


def ref_physderiv(nq, nelmt, bases, derivs, df, x):
    """(ref, absref) in np.longdouble, each of shape (d, nelmt * nq^d).  df may be None."""
    ld = np.longdouble
    ref = _physderiv(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], derivs, df, x, ld)
    absref = _physderiv(nq, nelmt, [_abs(b, ld) for b in bases], [_abs(d, ld) for d in derivs], _abs(df, ld),
                        _abs(x, ld), ld)
    return ref, absref


def physderiv_f64(nq, nelmt, bases, derivs, df, x):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    f = np.float64
    return (_physderiv(nq, nelmt, bases, derivs, df, x, f),
            _physderiv(nq, nelmt, [_abs(b, f) for b in bases], [_abs(d, f) for d in derivs], _abs(df, f), _abs(x, f), f))


def physderiv_excess(got, ref, absref, nq, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    gN = gamma(physderiv_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def dense_physderiv(nq, bases, derivs, df_e, x_e):
    """The d outputs of ONE element by einsum over dense point x mode matrices, in np.longdouble: an independent
    restatement of the operator.  Shape (d, nq^d)."""
    ld = np.longdouble
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    nm = [q - 1 for q in nq]
    B = [np.asarray(bases[d], dtype=ld).reshape(nm[d], nq[d]) for d in range(dim)]
    D = [np.asarray(derivs[d], dtype=ld).reshape(nq[d], nq[d]) for d in range(dim)]
    npt = int(np.prod(nq))
    x = np.asarray(x_e, dtype=ld).reshape(-1)
    grads = []
    for b in range(dim):
        # (D_b B_b)[p][i] = sum_m B_b[p][m] D_b[i][m] in direction b, B_d in the others
        f = [B[d] @ D[d].T if d == b else B[d] for d in range(dim)]
        if dim == 3:
            E = np.einsum("pi,qj,rk->kjirqp", f[0], f[1], f[2]).reshape(npt, -1)          # points x modes
        else:
            E = np.einsum("pi,qj->jiqp", f[0], f[1]).reshape(npt, -1)
        grads.append(E @ x)
    if df_e is None:
        return np.stack(grads)
    dd = np.asarray(df_e, dtype=ld).reshape(dim * dim, npt)
    return np.stack([sum(dd[a * dim + b] * grads[b] for b in range(dim)) for a in range(dim)])


def analytic_case(nq_iso, dim, nelmt, seed=0):
    """A polynomial on affine elements with its exact gradient: the Legendre modal basis at the Gauss-Lobatto points
    (helm_ref.gll / legendre_basis), the GLL differentiation matrix, x = A_e xi + c with A_e = 2 I + uniform(-1, 1), so
    d xi_b / d x_a = (A_e^-1)[b][a] on every point of the element.  Returns (bases, derivs, df, x, exact): exact[a] is
    d u / d x_a of u = sum x[r][q][p] P_p(xi_0) P_q(xi_1) P_r(xi_2) at the points, in np.longdouble, shape
    (dim, nelmt * nq^dim)."""
    ld = np.longdouble
    nq, nm = int(nq_iso), int(nq_iso) - 1
    rng = np.random.default_rng(4242 + seed + 31 * nq + dim)
    xi, _, D = gll(nq)
    basis = legendre_basis(nq)
    P = basis.reshape(nm, nq).astype(ld)
    dP = np.stack([_leg.Legendre.basis(p).deriv()(xi) for p in range(nm)]).astype(ld)
    A = 2.0 * np.eye(dim) + rng.uniform(-1, 1, (nelmt, dim, dim))
    Ainv = _inv_ld(A)
    npt = nq ** dim
    df = np.empty((nelmt, dim * dim, npt))
    for a in range(dim):
        for b in range(dim):
            df[:, a * dim + b, :] = np.asarray(Ainv[:, b, a], dtype=np.float64)[:, None]
    x = rng.uniform(-1, 1, nelmt * nm ** dim)
    xm = x.astype(ld).reshape((nelmt,) + (nm,) * dim)
    dfl = df.astype(ld)                                                         # the rounded planes the operator gets
    ref_grad = []
    for b in range(dim):
        f = [dP if d == b else P for d in range(dim)]
        if dim == 3:
            g = np.einsum("erqp,pi,qj,rk->ekji", xm, f[0], f[1], f[2])
        else:
            g = np.einsum("eqp,pi,qj->eji", xm, f[0], f[1])
        ref_grad.append(g.reshape(nelmt, npt))
    exact = np.stack([sum(dfl[:, a * dim + b] * ref_grad[b] for b in range(dim)).reshape(-1) for a in range(dim)])
    return [basis] * dim, [D.reshape(-1)] * dim, df.reshape(-1), x, exact


def _inv_ld(A):
    """Inverses of the small matrices A[e] in np.longdouble (adjugate over determinant; numpy's inv has no long double)."""
    ld = np.longdouble
    A = np.asarray(A, dtype=ld)
    n = A.shape[-1]
    out = np.empty_like(A)
    if n == 2:
        det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        out[:, 0, 0], out[:, 0, 1], out[:, 1, 0], out[:, 1, 1] = A[:, 1, 1], -A[:, 0, 1], -A[:, 1, 0], A[:, 0, 0]
        return out / det[:, None, None]
    c = lambda i, j: (A[:, (i + 1) % 3, (j + 1) % 3] * A[:, (i + 2) % 3, (j + 2) % 3]          # noqa: E731
                      - A[:, (i + 1) % 3, (j + 2) % 3] * A[:, (i + 2) % 3, (j + 1) % 3])
    for i in range(3):
        for j in range(3):
            out[:, j, i] = c(i, j)                                               # adjugate = cofactor transposed
    det = sum(A[:, 0, j] * c(0, j) for j in range(3))
    return out / det[:, None, None]
