"""Reference and error bounds of IProductWRTDerivBase (include/sumfact.h sf_iprodderiv_*) for
tests/test_iprodderiv_cpu.py and tests/test_gpu_iprodderiv.py.  Imports nothing of the product.

    g_b = w * sum_a df[e][a d + b] f_a   (per point),     out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p]

B the tensor-product BwdTrans basis (bases nm x nq row-major), D_b row-major nq x nq with (D_b u)[i] = sum_m D_b[i][m]
u[m], df[e][c][k][j][i] the d*d planes of sf_physderiv_*, c = a d + b (None: g_b = w f_b), w one plane per element
(None: no weight), f of shape (d, nelmt * nq^d): row a is f_a.  Results hold nelmt * nm^d modes.

The reference runs sweep by sweep in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is negligible against
the bound.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),

    N = sum_d nq_d + max_d nq_d + 2 d

-- the d-term product sum over a (d), the weight (1), one transposed derivative inner product (<= max nq_d), the sum of
the d terms (d - 1), the chain of transposed sweeps (sum nq_d); relative errors of chained operations compose
additively, as in tests/helm_ref.py -- u = 2^-53 (fp64) or 2^-24 (fp32), absref = the same operator applied to |B|,
|D|, |df|, |w| and |f|.  The bound is derived, not tuned, holds for any summation order, and is kept for df = None and
w = None, where some of the operations do not happen.  A zero bound needs a zero error.
"""
import math

import numpy as np

from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, unit_roundoff  # noqa: F401


def iprodderiv_n(nq):
    nq = [int(q) for q in nq]
    return sum(nq) + max(nq) + 2 * len(nq)


def _apply(a, M, f):
    """(M f) along direction a: out[.., i_a, ..] = sum_m M[i_a][m] f[.., m, ..]"""
    axis = f.ndim - 1 - a
    return np.moveaxis(np.moveaxis(f, axis, -1) @ M.T, -1, axis)


def _iprodderiv(nq, nelmt, bases, derivs, df, w, f, dt):
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    fa = [np.asarray(f[a], dtype=dt).reshape(shape) for a in range(dim)]
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    if df is None:
        t = fa
    else:
        dd = np.asarray(df, dtype=dt).reshape((nelmt, dim * dim) + shape[1:])
        t = []
        for b in range(dim):
            s = None
            for a in range(dim):
                term = dd[:, a * dim + b] * fa[a]
                s = term if s is None else s + term
            t.append(s)
    if w is not None:
        ww = np.asarray(w, dtype=dt).reshape(shape)
        t = [ww * s for s in t]
    v = None
    for b in range(dim):
        s = _apply(b, D[b].T, t[b])
        v = s if v is None else v + s
    return _transposed_sweeps(nq, nelmt, bases, np.ascontiguousarray(v).reshape(-1), dt)


def _abs(a, dt):
    return None if a is None else np.abs(np.asarray(a, dtype=dt))


def _rows(f):
    return [np.asarray(r) for r in f]


def ref_iprodderiv(nq, nelmt, bases, derivs, df, w, f):
    """(ref, absref) in np.longdouble, each nelmt * nm^d long.  df and w may be None; f has d rows."""
    ld = np.longdouble
    f = _rows(f)
    ref = _iprodderiv(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], derivs, df, w, f, ld)
    absref = _iprodderiv(nq, nelmt, [_abs(b, ld) for b in bases], [_abs(d, ld) for d in derivs], _abs(df, ld), _abs(w, ld),
                         [_abs(r, ld) for r in f], ld)
    return ref, absref


def iprodderiv_f64(nq, nelmt, bases, derivs, df, w, f):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    t = np.float64
    f = _rows(f)
    return (_iprodderiv(nq, nelmt, bases, derivs, df, w, f, t),
            _iprodderiv(nq, nelmt, [_abs(b, t) for b in bases], [_abs(d, t) for d in derivs], _abs(df, t), _abs(w, t),
                        [_abs(r, t) for r in f], t))


def iprodderiv_excess(got, ref, absref, nq, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    gN = gamma(iprodderiv_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def dense_iprodderiv(nq, bases, derivs, df_e, w_e, f_e):
    """The nm^d modes of ONE element by einsum over dense point x mode matrices, in np.longdouble: the transpose of the
    matrices of physderiv_ref.dense_physderiv (E_b = the points x modes matrix of D_b B), restated independently.
    f_e has shape (d, nq^d)."""
    ld = np.longdouble
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    nm = [q - 1 for q in nq]
    B = [np.asarray(bases[d], dtype=ld).reshape(nm[d], nq[d]) for d in range(dim)]
    D = [np.asarray(derivs[d], dtype=ld).reshape(nq[d], nq[d]) for d in range(dim)]
    npt = int(np.prod(nq))
    f = np.asarray(f_e, dtype=ld).reshape(dim, npt)
    dd = None if df_e is None else np.asarray(df_e, dtype=ld).reshape(dim * dim, npt)
    ww = None if w_e is None else np.asarray(w_e, dtype=ld).reshape(npt)
    out = 0
    for b in range(dim):
        m = [B[d] @ D[d].T if d == b else B[d] for d in range(dim)]
        if dim == 3:
            E = np.einsum("pi,qj,rk->kjirqp", m[0], m[1], m[2]).reshape(npt, -1)          # points x modes
        else:
            E = np.einsum("pi,qj->jiqp", m[0], m[1]).reshape(npt, -1)
        g = f[b] if dd is None else sum(dd[a * dim + b] * f[a] for a in range(dim))
        if ww is not None:
            g = ww * g
        out = out + E.T @ g
    return out
