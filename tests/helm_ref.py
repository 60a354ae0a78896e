"""Reference and error bounds of the fused Helmholtz operator (include/sumfact.h sf_helmholtz_*) for
tests/test_helmholtz_cpu.py and tests/test_gpu_helmholtz.py.  Imports nothing of the product.

    y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e

B the tensor-product BwdTrans basis (bases nm x nq row-major), D_a row-major nq x nq with (D_a u)[i] = sum_m D_a[i][m]
u[m], g[e][c][k][j][i] the component planes of the symmetric metric (3D c = 00, 01, 02, 11, 12, 22; 2D 00, 01, 11),
w[e][k][j][i] the mass weight (None with lambda == 0).

The reference runs sweep by sweep in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is negligible against
the bound.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),

    N = 2 sum_d nq_d + 2 max_d nq_d + 2 d + 3

-- the forward chain of inner products (sum nq_d), one derivative inner product (max nq_d), the d-term metric sum (d),
the mass term (2: lambda w, then times u), one transposed derivative inner product (max nq_d), the sum over a and the
mass term (d + 1), the transposed chain (sum nq_d); relative errors of chained operations compose additively, as in
tests/mass_ref.py -- u = 2^-53 (fp64) or 2^-24 (fp32), absref = the same operator applied to |B|, |D|, |g|, |w|,
|lambda| and |x|.  The bound is derived, not tuned, and holds for any summation order.  A zero bound needs a zero error.
"""
import math

import numpy as np
from numpy.polynomial import legendre as _leg

from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, per_element_dots, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps

COMPONENTS = {3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), 2: ((0, 0), (0, 1), (1, 1))}


def helm_n(nq):
    nq = [int(q) for q in nq]
    return 2 * sum(nq) + 2 * max(nq) + 2 * len(nq) + 3


def _helm(nq, nelmt, bases, derivs, g, w, lam, x, dt):
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    u = _forward_sweeps(nq, nelmt, bases, x, dt).reshape(shape)
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    gg = np.asarray(g, dtype=dt).reshape((nelmt, len(COMPONENTS[dim])) + shape[1:])

    def apply(a, M, f):
        """(M f) along direction a: out[.., i_a, ..] = sum_m M[i_a][m] f[.., m, ..]"""
        axis = f.ndim - 1 - a
        return np.moveaxis(np.moveaxis(f, axis, -1) @ M.T, -1, axis)

    du = [apply(a, D[a], u) for a in range(dim)]
    G = {}
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        G[(a, b)] = G[(b, a)] = gg[:, c]
    v = None
    if w is not None:
        v = (dt(lam) * np.asarray(w, dtype=dt).reshape(shape)) * u
    for a in range(dim):
        f = None
        for b in range(dim):
            term = G[(a, b)] * du[b]
            f = term if f is None else f + term
        t = apply(a, D[a].T, f)
        v = t if v is None else v + t
    return _transposed_sweeps(nq, nelmt, bases, np.ascontiguousarray(v).reshape(-1), dt)


def _abs(a, dt):
    return None if a is None else np.abs(np.asarray(a, dtype=dt))


def ref_helmholtz(nq, nelmt, bases, derivs, g, w, lam, x):
    """(ref, absref) in np.longdouble.  w may be None when lam == 0."""
    ld = np.longdouble
    assert w is not None or lam == 0
    ref = _helm(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], derivs, g, w if lam != 0 else None, lam, x, ld)
    absref = _helm(nq, nelmt, [_abs(b, ld) for b in bases], [_abs(d, ld) for d in derivs], _abs(g, ld),
                   _abs(w, ld) if lam != 0 else None, abs(lam), _abs(x, ld), ld)
    return ref, absref


def helmholtz_f64(nq, nelmt, bases, derivs, g, w, lam, x):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    f = np.float64
    return (_helm(nq, nelmt, bases, derivs, g, w if lam != 0 else None, lam, x, f),
            _helm(nq, nelmt, [_abs(b, f) for b in bases], [_abs(d, f) for d in derivs], _abs(g, f),
                  _abs(w, f) if lam != 0 else None, abs(lam), _abs(x, f), f))


def helm_excess(got, ref, absref, nq, u, factor=1.0):
    """max over elements of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    gN = gamma(helm_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def symmetry_bound(nq, u):
    """2 (gamma_N + gamma_m), m = nm^d the dot-product length: the factor on sum_e <|A||x|, |y|>_e."""
    m = int(np.prod([int(q) - 1 for q in nq]))
    return 2 * (gamma(helm_n(nq), u) + gamma(m, u))


def dense_operator(nq, bases, derivs, g_e, w_e, lam):
    """The nm^d x nm^d matrix of ONE element by einsum, in np.longdouble: an independent restatement of the operator."""
    ld = np.longdouble
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    nm = [q - 1 for q in nq]
    B = [np.asarray(bases[d], dtype=ld).reshape(nm[d], nq[d]) for d in range(dim)]
    D = [np.asarray(derivs[d], dtype=ld).reshape(nq[d], nq[d]) for d in range(dim)]
    gg = np.asarray(g_e, dtype=ld).reshape((len(COMPONENTS[dim]),) + tuple(reversed(nq)))
    eye = [np.eye(q, dtype=ld) for q in nq]
    if dim == 3:
        E = np.einsum("pi,qj,rk->kjirqp", B[0], B[1], B[2]).reshape(int(np.prod(nq)), -1)          # points x modes
        grad = [np.einsum("im,jn,ko->kjionm", *[D[d] if d == a else eye[d] for d in range(3)]).reshape(E.shape[0], -1)
                for a in range(3)]
    else:
        E = np.einsum("pi,qj->jiqp", B[0], B[1]).reshape(int(np.prod(nq)), -1)
        grad = [np.einsum("im,jn->jinm", *[D[d] if d == a else eye[d] for d in range(2)]).reshape(E.shape[0], -1)
                for a in range(2)]
    K = np.zeros((E.shape[0], E.shape[0]), dtype=ld)
    if w_e is not None and lam != 0:
        K += np.diag(ld(lam) * np.asarray(w_e, dtype=ld).reshape(-1))
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        Gd = np.diag(gg[c].reshape(-1))
        K += grad[a].T @ Gd @ grad[b]
        if a != b:
            K += grad[b].T @ Gd @ grad[a]
    return E.T @ K @ E


# ---- Gauss-Lobatto-Legendre data for the physics checks --------------------------------------------------------------
def gll(nq):
    """(points, weights, differentiation matrix D[i][m] = l'_m(xi_i)) of the nq Gauss-Lobatto-Legendre points."""
    n = nq - 1
    Pn = _leg.Legendre.basis(n)
    xi = np.concatenate(([-1.0], np.sort(np.real(Pn.deriv().roots())), [1.0])) if n > 1 else np.array([-1.0, 1.0])
    for _ in range(3):          # Newton on (1 - x^2) P_n'(x) for the interior points
        if n > 1:
            x = xi[1:-1]
            d1, d2 = Pn.deriv()(x), Pn.deriv(2)(x)
            xi[1:-1] = x - (1 - x * x) * d1 / (-2 * x * d1 + (1 - x * x) * d2)
    pn = Pn(xi)
    wts = 2.0 / (n * (n + 1) * pn * pn)
    D = np.zeros((nq, nq))
    for i in range(nq):
        for m in range(nq):
            if i != m:
                D[i, m] = pn[i] / pn[m] / (xi[i] - xi[m])
    D[0, 0], D[n, n] = -n * (n + 1) / 4.0, n * (n + 1) / 4.0
    return xi, wts, D


def legendre_basis(nq):
    """Modal basis B[p][i] = P_p(xi_i), p < nq - 1, at the GLL points: row-major nm x nq, flat."""
    xi, _, _ = gll(nq)
    return np.stack([_leg.Legendre.basis(p)(xi) for p in range(nq - 1)]).reshape(-1)


def gll_setup(nq_iso, dim, nelmt):
    """(bases, derivs, g, w) of the reference element with G = I * (tensor GLL weight), w the same weight."""
    xi, wts, D = gll(nq_iso)
    b = legendre_basis(nq_iso)
    W = wts
    for _ in range(dim - 1):
        W = np.multiply.outer(wts, W)
    W = W.reshape(-1)
    ncomp = len(COMPONENTS[dim])
    ge = np.zeros((ncomp, W.size))
    for c, (a, bb) in enumerate(COMPONENTS[dim]):
        if a == bb:
            ge[c] = W
    g = np.tile(ge.reshape(-1), nelmt)
    return [b] * dim, [D.reshape(-1)] * dim, g, np.tile(W, nelmt)


def exact_energy(nq_iso, dim, x_e):
    """int |grad u|^2 over [-1,1]^d for u = sum x[r][q][p] P_p P_q P_r, from Gauss-Legendre integrals (exact)."""
    nm = nq_iso - 1
    xg, wg = _leg.leggauss(nm + 2)
    P = np.stack([_leg.Legendre.basis(p)(xg) for p in range(nm)])
    dP = np.stack([_leg.Legendre.basis(p).deriv()(xg) for p in range(nm)])
    Mm = (P * wg) @ P.T
    Km = (dP * wg) @ dP.T
    x = np.asarray(x_e, dtype=np.float64).reshape((nm,) * dim)
    total = 0.0
    for a in range(dim):
        y = x
        for d in range(dim):
            axis = dim - 1 - d
            y = np.moveaxis(np.moveaxis(y, axis, -1) @ (Km if d == a else Mm).T, -1, axis)
        total += float(np.sum(x * y))
    return total
