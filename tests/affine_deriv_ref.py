"""References and error bounds of the gradient and the weak divergence on affine elements (include/sumfact.h
sf_aff_physderiv_*, sf_aff_iprodderiv_*) for tests/test_affine_deriv_cpu.py, tests/test_gpu_affine_physderiv.py and
tests/test_gpu_affine_iprodderiv.py.  Imports nothing of the product.

    gradient:         u = B x_e,  du_b = D_b u,  out_a[e][k][j][i] = sum_b dfe[e][a d + b] du_b[e][k][j][i]
    weak divergence:  t_b = sum_a dfe[e][a d + b] in_a,  q = qw2[k] (qw1[j] qw0[i]),  g_b = (je[e] q) t_b,
                      out_e = sum_b B^T D_b^T g_b                                      (je None: g_b = t_b)

dfe[e][c] the d*d constants of the element's inverse Jacobian, c = a d + b for d xi_b / d x_a (the order of the planes of
sf_physderiv_*'s df; not symmetric), je[e] one scalar per element, qw_d the one-dimensional quadrature weights.  The
evaluations below broadcast the constants of an element over its points and run sweep by sweep in a dtype of the caller's
choice: np.longdouble for the reference (80-bit on x86-64, eps 2^-63: its own error is negligible against the bound),
np.float64 for long batches.  They do not call tests/physderiv_ref.py or tests/iprodderiv_ref.py: the CPU tests compare
the two restatements on expanded planes.

Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),

    gradient:         N = physderiv_n(nq) = sum_d nq_d + max_d nq_d + d          (the operations of the deformed call)
    weak divergence:  N = iprodderiv_n(nq) + d = sum_d nq_d + max_d nq_d + 3 d

-- iprodderiv_n counts ONE rounding for the weight w; here the weight is formed in the working precision from d + 1
numbers: d - 1 products for q, one for je q, and the product with t_b that iprodderiv_n already holds, hence d more --
the step affine_n takes over helm_n.  u = 2^-53 (fp64) or 2^-24 (fp32); absref = the same operator applied to the
absolute values of everything.  Derived, not tuned; holds for any summation order; kept for je = None, where the weight
operations do not happen.  A zero bound needs a zero error.
"""
import math

import numpy as np

from affine_ref import point_weights
from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, unit_roundoff  # noqa: F401
from iprodderiv_ref import iprodderiv_n
from mass_ref import _forward_sweeps
from physderiv_ref import physderiv_n


def affine_physderiv_n(nq):
    return physderiv_n(nq)


def affine_iprodderiv_n(nq):
    return iprodderiv_n(nq) + len(nq)


def _apply(a, M, f):
    """(M f) along direction a: out[.., i_a, ..] = sum_m M[i_a][m] f[.., m, ..]"""
    axis = f.ndim - 1 - a
    return np.moveaxis(np.moveaxis(f, axis, -1) @ M.T, -1, axis)


def _consts(dfe, nelmt, dim, dt):
    """dfe as [e][c] broadcastable over the points of an element."""
    return np.asarray(dfe, dtype=dt).reshape((nelmt, dim * dim) + (1,) * dim)


def affine_physderiv_eval(nq, nelmt, bases, derivs, dfe, x, dt):
    """The d outputs in dtype dt, shape (d, nelmt * nq^d)."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    u = _forward_sweeps(nq, nelmt, [np.asarray(b, dtype=dt) for b in bases], np.asarray(x, dtype=dt), dt).reshape(shape)
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    du = [_apply(a, D[a], u) for a in range(dim)]
    dd = _consts(dfe, nelmt, dim, dt)
    out = []
    for a in range(dim):
        f = None
        for b in range(dim):
            term = dd[:, a * dim + b] * du[b]
            f = term if f is None else f + term
        out.append(np.ascontiguousarray(f).reshape(-1))
    return np.stack(out)


def affine_iprodderiv_eval(nq, nelmt, bases, derivs, qws, dfe, je, f, dt):
    """The nelmt * nm^d modes in dtype dt; je None: no weight, qws is not looked at."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))
    fa = [np.asarray(f[a], dtype=dt).reshape(shape) for a in range(dim)]
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    dd = _consts(dfe, nelmt, dim, dt)
    t = []
    for b in range(dim):
        s = None
        for a in range(dim):
            term = dd[:, a * dim + b] * fa[a]
            s = term if s is None else s + term
        t.append(s)
    if je is not None:
        w = np.asarray(je, dtype=dt).reshape((nelmt,) + (1,) * dim) * point_weights(nq, qws, dt)[None]
        t = [w * s for s in t]
    v = None
    for b in range(dim):
        s = _apply(b, D[b].T, t[b])
        v = s if v is None else v + s
    return _transposed_sweeps(nq, nelmt, [np.asarray(b, dtype=dt) for b in bases], np.ascontiguousarray(v).reshape(-1), dt)


def _abs(a):
    return None if a is None else np.abs(np.asarray(a))


def _absl(seq):
    return None if seq is None else [_abs(a) for a in seq]


def ref_affine_physderiv(nq, nelmt, bases, derivs, dfe, x, dt=np.longdouble):
    """(ref, absref) in np.longdouble (or dt), each of shape (d, nelmt * nq^d)."""
    return (affine_physderiv_eval(nq, nelmt, bases, derivs, dfe, x, dt),
            affine_physderiv_eval(nq, nelmt, _absl(bases), _absl(derivs), _abs(dfe), _abs(x), dt))


def ref_affine_iprodderiv(nq, nelmt, bases, derivs, qws, dfe, je, f, dt=np.longdouble):
    """(ref, absref) in np.longdouble (or dt), each nelmt * nm^d long.  je may be None; f has d rows."""
    f = [np.asarray(r) for r in f]
    qa = None if je is None else _absl(qws)
    return (affine_iprodderiv_eval(nq, nelmt, bases, derivs, qws, dfe, je, f, dt),
            affine_iprodderiv_eval(nq, nelmt, _absl(bases), _absl(derivs), qa, _abs(dfe), _abs(je), _absl(f), dt))


def _excess(got, ref, absref, gN, factor):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def affine_physderiv_excess(got, ref, absref, nq, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    return _excess(got, ref, absref, gamma(affine_physderiv_n(nq), u), factor)


def affine_iprodderiv_excess(got, ref, absref, nq, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref), N = iprodderiv_n + d; <= 1 passes."""
    return _excess(got, ref, absref, gamma(affine_iprodderiv_n(nq), u), factor)


def expand_df(nq, nelmt, dfe, dt=np.longdouble):
    """The planes df[e][c][k][j][i] = dfe[e][c] of sf_physderiv_* / sf_iprodderiv_*, flat, in dtype dt."""
    dim, npt = len(nq), int(np.prod([int(q) for q in nq]))
    dd = np.asarray(dfe, dtype=dt).reshape(nelmt, dim * dim, 1)
    return np.ascontiguousarray(np.broadcast_to(dd, (nelmt, dim * dim, npt))).reshape(-1)


def expand_w(nq, nelmt, qws, je, dt=np.longdouble):
    """The weight plane w[e][k][j][i] = je[e] * (qw2[k] * (qw1[j] * qw0[i])) of sf_iprodderiv_*, flat, in dtype dt, with
    exactly this association (each product rounded to dt); None when je is None."""
    if je is None:
        return None
    nq = tuple(int(q) for q in nq)
    q = point_weights(nq, qws, dt).reshape(1, -1)
    return (np.asarray(je, dtype=dt).reshape(nelmt, 1) * q).reshape(-1)
