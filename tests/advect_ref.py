"""Reference and error bounds of the weak advection term (include/sumfact.h sf_advect_*) for tests/test_advect_cpu.py and
tests/test_gpu_advect.py.  Imports nothing of the product.

    u_a = B in_a,   J[a][b] = D_b u_a,   beta_b = sum_j c_j df[j d + b],   r_a = w (sum_b beta_b J[a][b]),
    out_a = B^T r_a                                             (a = 0 .. nf-1, nf = 1 or d; b, j = 0 .. d-1)

B the tensor-product BwdTrans basis (bases nm x nq row-major), D_b row-major nq x nq with (D_b u)[i] = sum_m D_b[i][m]
u[m], df[e][c][k][j][i] the d*d planes of the inverse Jacobian, c = a d + b for d xi_b / d x_a, w[e][k][j][i] the weight
plane, c_j[e][k][j][i] the d planes of the advecting velocity.  `x` holds the nf fields, shape (nf, nelmt * nm^d) or a
sequence of nf flat arrays; results have the shape (nf, nelmt * nm^d): row a is out_a.

The reference runs step by step, in the order above, in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is
negligible against the bound.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,
gamma_N = N u / (1 - N u),

    N = 2 sum_d nq_d + max_d nq_d + 2 d + 1

-- the forward chain of inner products (sum nq_d), one derivative inner product (max nq_d), the d-term sum of beta (d),
the d-term dot product with beta (d), the weight (1), the transposed chain (sum nq_d), by the counting of
tests/physderiv_ref.py and tests/mass_ref.py; relative errors of chained operations compose additively -- u = 2^-53
(fp64) or 2^-24 (fp32), absref = the same operator applied to |B|, |D|, |df|, |w|, |c| and |x|.  The bound is derived, not
tuned, and holds for any summation order.  A zero bound needs a zero error.
"""
import math

import numpy as np

from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps
from physderiv_ref import _apply


def advect_n(nq):
    nq = [int(q) for q in nq]
    return 2 * sum(nq) + max(nq) + 2 * len(nq) + 1


def _fields(x):
    """The nf flat fields of `x`: a (nf, n) array, a flat array (one field) or a sequence of flat arrays."""
    if isinstance(x, np.ndarray):
        return [x] if x.ndim == 1 else [x[a] for a in range(x.shape[0])]
    return list(x)


def _advect(nq, nelmt, bases, derivs, df, w, c, x, dt, mutate=None):
    """mutate: None, or a deliberately wrong variant for the tests of the bound -- "df-transposed" (df[b d + j] in the place
    of df[j d + b]), "c-field-swapped" (beta dotted with J[b][a] in the place of J[a][b]; nf = d), "no-w"."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    dd = np.asarray(df, dtype=dt).reshape((nelmt, dim * dim) + shape[1:])
    ww = np.asarray(w, dtype=dt).reshape(shape)
    cs = [np.asarray(v, dtype=dt).reshape(shape) for v in _fields(c)]
    assert len(cs) == dim
    beta = []
    for b in range(dim):
        s = None
        for j in range(dim):
            plane = dd[:, b * dim + j] if mutate == "df-transposed" else dd[:, j * dim + b]
            term = cs[j] * plane
            s = term if s is None else s + term
        beta.append(s)
    xs = _fields(x)
    assert len(xs) in (1, dim)
    J = []
    for xa in xs:
        u = _forward_sweeps(nq, nelmt, bases, xa, dt).reshape(shape)
        J.append([_apply(b, D[b], u) for b in range(dim)])
    out = []
    for a in range(len(xs)):
        s = None
        for b in range(dim):
            term = beta[b] * (J[b][a] if mutate == "c-field-swapped" else J[a][b])
            s = term if s is None else s + term
        r = s if mutate == "no-w" else ww * s
        out.append(_transposed_sweeps(nq, nelmt, bases, np.ascontiguousarray(r).reshape(-1), dt))
    return np.stack(out)


def _abs(a, dt):
    return np.abs(np.asarray(a, dtype=dt))


def ref_advect(nq, nelmt, bases, derivs, df, w, c, x):
    """(ref, absref) in np.longdouble, each of shape (nf, nelmt * nm^d)."""
    ld = np.longdouble
    ref = _advect(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], derivs, df, w, c, x, ld)
    absref = _advect(nq, nelmt, [_abs(b, ld) for b in bases], [_abs(d, ld) for d in derivs], _abs(df, ld), _abs(w, ld),
                     [_abs(v, ld) for v in _fields(c)], [_abs(v, ld) for v in _fields(x)], ld)
    return ref, absref


def advect_f64(nq, nelmt, bases, derivs, df, w, c, x, dt=np.float64, mutate=None):
    """(out, absout) with sweeps in dt (reshaped matmuls): an evaluation in working precision, and the deliberately wrong
    variants of the CPU tests."""
    return (_advect(nq, nelmt, [np.asarray(b, dtype=dt) for b in bases], derivs, df, w, c, x, dt, mutate),
            _advect(nq, nelmt, [_abs(b, dt) for b in bases], [_abs(d, dt) for d in derivs], _abs(df, dt), _abs(w, dt),
                    [_abs(v, dt) for v in _fields(c)], [_abs(v, dt) for v in _fields(x)], dt))


def advect_excess(got, ref, absref, nq, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    gN = gamma(advect_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def dense_advect(nq, bases, derivs, df_e, w_e, c_e, x_e):
    """out of ONE element and ONE field by dense point x mode matrices, in np.longdouble: an independent restatement of
    the operator, out = E^T diag(w) sum_b diag(beta_b) G_b x with E the point x mode matrix of B.  Shape (nm^d,)."""
    ld = np.longdouble
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    nm = [q - 1 for q in nq]
    B = [np.asarray(bases[d], dtype=ld).reshape(nm[d], nq[d]) for d in range(dim)]
    D = [np.asarray(derivs[d], dtype=ld).reshape(nq[d], nq[d]) for d in range(dim)]
    npt = int(np.prod(nq))

    def matrix(f):
        if dim == 3:
            return np.einsum("pi,qj,rk->kjirqp", f[0], f[1], f[2]).reshape(npt, -1)          # points x modes
        return np.einsum("pi,qj->jiqp", f[0], f[1]).reshape(npt, -1)

    E = matrix(B)
    G = [matrix([B[d] @ D[d].T if d == b else B[d] for d in range(dim)]) for b in range(dim)]
    dd = np.asarray(df_e, dtype=ld).reshape(dim * dim, npt)
    cc = np.asarray(c_e, dtype=ld).reshape(dim, npt)
    x = np.asarray(x_e, dtype=ld).reshape(-1)
    r = np.zeros(npt, dtype=ld)
    for b in range(dim):
        beta = sum(cc[j] * dd[j * dim + b] for j in range(dim))
        r = r + beta * (G[b] @ x)
    return E.T @ (np.asarray(w_e, dtype=ld).reshape(-1) * r)
