"""Reference and error bounds of the fused mass operator (include/sumfact.h sf_mass_*) for tests/test_mass_cpu.py and
tests/test_gpu_mass.py.  Imports nothing of the product.

    3D: out[e][r'][q'][p'] = sum_kji B0[p'][i] B1[q'][j] B2[r'][k] w[e][k][j][i] (sum_rqp in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k])
    2D: out[e][q'][p']     = sum_ji  B0[p'][i] B1[q'][j]           w[e][j][i]    (sum_qp  in[e][q][p]    B0[p][i] B1[q][j])

The reference runs sweep by sweep in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is negligible against
the bounds.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),
N = 2 (nq0 + nq1 [+ nq2]) + 1 -- the forward chain of inner products, one multiply, the transposed chain; relative
errors of chained inner products compose additively (the standard forward bound tests/iprod_ref.py uses, applied twice
plus one) -- u = 2^-53 (fp64) or 2^-24 (fp32), absref = the same operator applied to |B|, |w| and |x|.  The bound is
derived, not tuned, and holds for any summation order.  A zero bound needs a zero error.
"""
import math

import numpy as np

from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, per_element_dots, unit_roundoff  # noqa: F401


def mass_n(nq):
    return 2 * sum(int(q) for q in nq) + 1


def _forward_sweeps(nq, nelmt, bases, x, dt):
    """BwdTrans in dtype dt: x holds nelmt * prod(nm) modes, bases are nm x nq row-major; returns [e][k][j][i] flat."""
    nq = tuple(int(q) for q in nq)
    nm = [q - 1 for q in nq]
    b = [np.asarray(bases[d], dtype=dt).reshape(nm[d], nq[d]) for d in range(len(nq))]
    x = np.asarray(x, dtype=dt)
    if len(nq) == 3:
        u = x.reshape(nelmt, nm[2], nm[1], nm[0])
        w1 = u @ b[0]                                                # [e][r][q][i]
        w2 = b[1].T @ w1                                             # [e][r][j][i]
        out = b[2].T @ w2.reshape(nelmt, nm[2], nq[1] * nq[0])       # [e][k][(j,i)]
    else:
        u = x.reshape(nelmt, nm[1], nm[0])
        w1 = u @ b[0]                                                # [e][q][i]
        out = b[1].T @ w1                                            # [e][j][i]
    return np.ascontiguousarray(out).reshape(-1)


def _mass(nq, nelmt, bases, w, x, dt):
    pts = _forward_sweeps(nq, nelmt, bases, x, dt) * np.asarray(w, dtype=dt).reshape(-1)
    return _transposed_sweeps(nq, nelmt, bases, pts, dt)


def ref_mass(nq, nelmt, bases, w, x):
    """(ref, absref) in np.longdouble."""
    ld = np.longdouble
    ref = _mass(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], w, x, ld)
    absref = _mass(nq, nelmt, [np.abs(np.asarray(b, dtype=ld)) for b in bases], np.abs(np.asarray(w, dtype=ld)),
                   np.abs(np.asarray(x, dtype=ld)), ld)
    return ref, absref


def mass_f64(nq, nelmt, bases, w, x):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    f = np.float64
    return (_mass(nq, nelmt, bases, w, x, f),
            _mass(nq, nelmt, [np.abs(np.asarray(b, dtype=f)) for b in bases], np.abs(np.asarray(w, dtype=f)),
                  np.abs(np.asarray(x, dtype=f)), f))


def mass_excess(got, ref, absref, nq, u, factor=1.0):
    """max over elements of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    g = gamma(mass_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * g * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def symmetry_bound(nq, u):
    """2 (gamma_N + gamma_m), m = nm^d the dot-product length: the factor on sum_e <|M||x|, |y|>_e."""
    m = int(np.prod([int(q) - 1 for q in nq]))
    return 2 * (gamma(mass_n(nq), u) + gamma(m, u))
