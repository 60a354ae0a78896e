"""Reference and error bounds of the fused Helmholtz operator on affine elements (include/sumfact.h
sf_affine_helmholtz_*) for tests/test_affine_cpu.py and tests/test_gpu_affine.py.  Imports nothing of the product.

    G_ab,e[k][j][i] = ge[e][ab] q2[k] q1[j] q0[i]        w_e[k][j][i] = je[e] q2[k] q1[j] q0[i]
    y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e

The reference expands ge, je and the one-dimensional weights to the planes g and w of sf_helmholtz_* in np.longdouble
and calls tests/helm_ref.py's long-double reference on them.  Elementwise bound of a computed result:

    |got - ref| <= gamma_N' * absref,    N' = helm_n(nq) + d,    gamma_N = N u / (1 - N u)

u = 2^-53 (fp64) or 2^-24 (fp32).  The extra d on helm_n: d - 1 products that form the point weight q and one product
of q with the metric sum; the mass term (lambda je) q u gains the same d.  absref is the operator applied to the
absolute values of everything.  Derived, not tuned; it holds for any summation order.
"""
import math

import numpy as np
from numpy.polynomial import legendre as _leg

from helm_ref import COMPONENTS, gamma, gll, helm_n, legendre_basis, ref_helmholtz
from iprod_ref import _sweeps as _transposed_sweeps
from mass_ref import _forward_sweeps


def affine_n(nq):
    return helm_n(nq) + len(nq)


def point_weights(nq, qws, dt=np.longdouble):
    """q[k][j][i] = qw2[k] (qw1[j] qw0[i]) (2D: q[j][i] = qw1[j] qw0[i]) in dtype dt, shaped like one element's points."""
    q = np.asarray(qws[0], dtype=dt).reshape(-1)
    assert q.size == nq[0]
    for d in range(1, len(nq)):
        qd = np.asarray(qws[d], dtype=dt).reshape(-1)
        assert qd.size == nq[d]
        q = np.multiply.outer(qd, q)
    return q


def expand(nq, nelmt, qws, ge, je, dt=np.longdouble):
    """(g, w) of sf_helmholtz_*, flat, in dtype dt: g[e][c][k][j][i] = ge[e][c] q[k][j][i], w[e][k][j][i] = je[e]
    q[k][j][i] (w None when je is None)."""
    nq = tuple(int(x) for x in nq)
    ncomp = len(COMPONENTS[len(nq)])
    q = point_weights(nq, qws, dt).reshape(-1)
    g = np.asarray(ge, dtype=dt).reshape(nelmt, ncomp, 1) * q.reshape(1, 1, -1)
    w = None if je is None else np.asarray(je, dtype=dt).reshape(nelmt, 1) * q.reshape(1, -1)
    return g.reshape(-1), None if w is None else w.reshape(-1)


def ref_affine(nq, nelmt, bases, derivs, qws, ge, je, lam, x):
    """(ref, absref) in np.longdouble.  je may be None when lam == 0."""
    assert je is not None or lam == 0
    g, w = expand(nq, nelmt, qws, ge, je if lam != 0 else None)
    return ref_helmholtz(nq, nelmt, bases, derivs, g, w, lam, x)


def affine_eval(nq, nelmt, bases, derivs, qws, ge, je, lam, x, dt):
    """The documented order of operations in dtype dt with numpy (reshaped matmuls for the sums)."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))
    bases = [np.asarray(b, dtype=dt) for b in bases]
    u = _forward_sweeps(nq, nelmt, bases, np.asarray(x, dtype=dt), dt).reshape(shape)
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    q = point_weights(nq, qws, dt)[None]
    gg = np.asarray(ge, dtype=dt).reshape((nelmt, len(COMPONENTS[dim])) + (1,) * dim)

    def apply(a, M, f):
        axis = f.ndim - 1 - a
        return np.moveaxis(np.moveaxis(f, axis, -1) @ M.T, -1, axis)

    du = [apply(a, D[a], u) for a in range(dim)]
    G = {}
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        G[(a, b)] = G[(b, a)] = gg[:, c]
    v = None
    if je is not None and lam != 0:
        lj = (dt(lam) * np.asarray(je, dtype=dt)).reshape((nelmt,) + (1,) * dim)
        v = (lj * q) * u
    for a in range(dim):
        f = None
        for b in range(dim):
            term = G[(a, b)] * du[b]
            f = term if f is None else f + term
        t = apply(a, D[a].T, q * f)
        v = t if v is None else v + t
    assert v.dtype == dt
    return _transposed_sweeps(nq, nelmt, bases, np.ascontiguousarray(v).reshape(-1), dt)


def affine_excess(got, ref, absref, nq, u, factor=1.0):
    """max over elements of |got - ref| / (factor * gamma_N' * absref); <= 1 passes.  Zero bound needs zero error."""
    gN = gamma(affine_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


# ---- affine geometry for the physics checks ---------------------------------------------------------------------------
def affine_geometry(dim, nelmt, seed):
    """Seeded Jacobians J_e = I + 0.3 U(-1, 1) and what the operator takes of them: (J, ge, je) with
    ge[e] = |det J_e| J_e^-1 J_e^-T in the component order of g, je[e] = |det J_e|."""
    rng = np.random.default_rng(seed)
    J = np.eye(dim)[None] + 0.3 * rng.uniform(-1, 1, (nelmt, dim, dim))
    det = np.abs(np.linalg.det(J))
    Ji = np.linalg.inv(J)
    K = det[:, None, None] * (Ji @ np.swapaxes(Ji, 1, 2))
    ge = np.stack([K[:, a, b] for a, b in COMPONENTS[dim]], axis=1)
    return J, np.ascontiguousarray(ge).reshape(-1), det


def gll_affine_setup(nq_iso, dim):
    """(bases, derivs, qws): Legendre modal basis at the GLL points, the GLL differentiation matrix and weights."""
    _, wts, D = gll(nq_iso)
    b = legendre_basis(nq_iso)
    return [b] * dim, [D.reshape(-1)] * dim, [wts] * dim


def exact_energy_affine(nq_iso, dim, x_e, J_e):
    """int |grad u|^2 over the physical element x = J_e xi + c, u = sum x[r][q][p] P_p P_q P_r on [-1,1]^d:
    sum_ab K_ab int d_a u d_b u dxi with K = |det J| J^-1 J^-T, the mixed terms included, from Gauss-Legendre integrals
    of Legendre polynomials and their derivatives (exact)."""
    nm = nq_iso - 1
    xg, wg = _leg.leggauss(nm + 2)
    P = np.stack([_leg.Legendre.basis(p)(xg) for p in range(nm)])
    dP = np.stack([_leg.Legendre.basis(p).deriv()(xg) for p in range(nm)])
    Mm = (P * wg) @ P.T            # int P_p P_q
    Km = (dP * wg) @ dP.T          # int P_p' P_q'
    Cm = (dP * wg) @ P.T           # int P_p' P_q
    Ji = np.linalg.inv(J_e)
    K = abs(np.linalg.det(J_e)) * (Ji @ Ji.T)
    x = np.asarray(x_e, dtype=np.float64).reshape((nm,) * dim)
    total = 0.0
    for a in range(dim):
        for b in range(dim):
            y = x
            for d in range(dim):
                if d == a and d == b:
                    mat = Km
                elif d == a:
                    mat = Cm       # row index differentiated
                elif d == b:
                    mat = Cm.T
                else:
                    mat = Mm
                axis = dim - 1 - d
                # y[.., p, ..] = sum_q mat[p][q] x[.., q, ..]
                y = np.moveaxis(np.moveaxis(y, axis, -1) @ mat.T, -1, axis)
            total += K[a, b] * float(np.sum(x * y))
    return total
