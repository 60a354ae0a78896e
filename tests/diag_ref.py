"""Reference and error bound of the diagonal of the fused Helmholtz operator (include/sumfact.h sf_diag_helmholtz_*,
sf_diag_tables_*) for tests/test_diag_cpu.py and tests/test_gpu_diag.py.  Imports nothing of the product.

    diag_e = diag( B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B )

With E_d = B_d D_d^T (E_d[p][i] = sum_m D_d[i][m] B_d[p][m], the derivative of mode p at point i) and the three tables
per direction T_d^0 = B_d o B_d, T_d^1 = E_d o B_d, T_d^2 = E_d o E_d (row-major nm_d x nq_d each):

    diag_e[r][q][p] = sum_kji lambda w_e[k][j][i] T_0^0[p][i] T_1^0[q][j] T_2^0[r][k]
                    + sum_c f_c sum_kji g_e[c][k][j][i] T_0^{s0}[p][i] T_1^{s1}[q][j] T_2^{s2}[r][k]

c over the planes of g in helm_ref.COMPONENTS order; for the plane (a, b): s_d = [d == a] + [d == b], f_c = 1 if a == b,
else 2.  Seven terms in 3D, four in 2D (which drops k / r).

The reference evaluates this term by term, sweep by sweep (k, then j, then i), in np.longdouble (80-bit on x86-64): its
own error is negligible against the bound.  Elementwise bound of a computed result:

    |got - ref| <= gamma_N * absref,      gamma_N = N u / (1 - N u),      N = 3 sum_d nq_d + d + 2 + M,  M = 6 (3D), 3 (2D)

absref = the same formula on |B|, |D|, |g|, |w|, |lambda| with the tables formed from the absolute values (|B| o |B|,
(|B||D|^T) o |B|, (|B||D|^T)^2).  Derivation: a computed value is a sum of products, each carrying a product of factors
(1 + delta), |delta| <= u; N counts the factors of the longest chain and relative errors of chained operations compose
additively (Higham, Accuracy and Stability, lemma 3.1 / 3.3), as in tests/mass_ref.py and tests/helm_ref.py:
  * a table entry of direction d: E is an inner product of length nq_d (nq_d factors: the products and nq_d - 1 additions,
    fewer with FMAs), the worst table E o E squares it and multiplies once: 2 nq_d + 1.  The error of E is relative to
    |B||D|^T, not to |E|: hence the tables of absolute values in absref.                              sum_d (2 nq_d + 1)
  * the sweep of direction d: one product with the table entry and nq_d - 1 additions.                        sum_d nq_d
  * lambda rounded to the scalar type, and the product lambda w.                                                       2
  * the sums over the terms: seven terms in 3D are joined by six additions, four in 2D by three, and no value passes
    through more than that whatever the tree.  Doubling the off-diagonal planes is exact.                              M
Nothing here depends on the order of a sum or on where the merges sit: the bound holds for any summation order.  It is
derived, not tuned.  A zero bound needs a zero error.  (8^3: N = 83; 4 x 9: N = 46.)
The tables alone (sf_diag_tables_*): |tab - ref| <= gamma_{2 nq + 1} * abstab.
"""
import math

import numpy as np

from helm_ref import COMPONENTS, gamma, unit_roundoff  # noqa: F401


def diag_n(nq):
    nq = [int(q) for q in nq]
    return 3 * sum(nq) + len(nq) + 2 + (6 if len(nq) == 3 else 3)


def tables(nq_d, basis, deriv, dt=np.longdouble, absolute=False):
    """(3, nm, nq) array of T^0, T^1, T^2 of one direction in `dt`; absolute: from |basis|, |deriv|."""
    nq_d = int(nq_d)
    B = np.asarray(basis, dtype=dt).reshape(nq_d - 1, nq_d)
    D = np.asarray(deriv, dtype=dt).reshape(nq_d, nq_d)
    if absolute:
        B, D = np.abs(B), np.abs(D)
    E = B @ D.T
    return np.stack([B * B, E * B, E * E])


def _sweep(x, d, T):
    """Contract direction d of x[e][..] (direction 0 is the last axis) with T[p][i]: out[.., p, ..] = sum_i x[.., i, ..] T[p][i]."""
    axis = x.ndim - 1 - d
    return np.moveaxis(np.moveaxis(x, axis, -1) @ T.T, -1, axis)


def _diag(nq, nelmt, tabs, g, w, lam, dt):
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    gg = np.asarray(g, dtype=dt).reshape((nelmt, len(COMPONENTS[dim])) + shape[1:])
    terms = []
    if w is not None:
        terms.append((dt(lam) * np.asarray(w, dtype=dt).reshape(shape), (0,) * dim))
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        s = tuple(int(d == a) + int(d == b) for d in range(dim))
        terms.append((gg[:, c] if a == b else dt(2) * gg[:, c], s))
    out = None
    for x, s in terms:
        for d in reversed(range(dim)):                            # k -> r, j -> q, i -> p
            x = _sweep(x, d, tabs[d][s[d]])
        out = x if out is None else out + x
    return np.ascontiguousarray(out).reshape(-1)


def ref_diag(nq, nelmt, bases, derivs, g, w, lam):
    """(ref, absref) in np.longdouble, flat [e][r][q][p].  w may be None when lam == 0."""
    ld = np.longdouble
    assert w is not None or lam == 0
    nq = tuple(int(q) for q in nq)
    t = [tables(q, b, d, ld) for q, b, d in zip(nq, bases, derivs)]
    ta = [tables(q, b, d, ld, absolute=True) for q, b, d in zip(nq, bases, derivs)]
    on = lam != 0
    ref = _diag(nq, nelmt, t, g, w if on else None, lam, ld)
    absref = _diag(nq, nelmt, ta, np.abs(np.asarray(g, dtype=ld)), np.abs(np.asarray(w, dtype=ld)) if on else None,
                   abs(lam), ld)
    return ref, absref


def diag_np(nq, nelmt, bases, derivs, g, w, lam, dt):
    """(out, absout) with the tables and the sweeps evaluated in `dt` (reshaped matmuls)."""
    nq = tuple(int(q) for q in nq)
    on = lam != 0
    t = [tables(q, b, d, dt) for q, b, d in zip(nq, bases, derivs)]
    ta = [tables(q, b, d, dt, absolute=True) for q, b, d in zip(nq, bases, derivs)]
    return (_diag(nq, nelmt, t, g, w if on else None, lam, dt),
            _diag(nq, nelmt, ta, np.abs(np.asarray(g, dtype=dt)), np.abs(np.asarray(w, dtype=dt)) if on else None,
                  abs(lam), dt))


def diag_f64(nq, nelmt, bases, derivs, g, w, lam):
    """The fp64 numpy form, for batches where long double is too slow."""
    return diag_np(nq, nelmt, bases, derivs, g, w, lam, np.float64)


def diag_excess(got, ref, absref, nq, u, factor=1.0):
    """max over entries of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  Zero bound needs zero error."""
    return _excess(got, ref, absref, factor * gamma(diag_n(nq), u))


def tables_excess(got, ref, absref, nq_d, u):
    """The same for one direction's tables against gamma_{2 nq + 1} * abstab."""
    return _excess(got, ref, absref, gamma(2 * int(nq_d) + 1, u))


def _excess(got, ref, absref, gN):
    err = np.abs(np.asarray(got, dtype=np.longdouble).reshape(-1) - np.asarray(ref, dtype=np.longdouble).reshape(-1))
    bound = gN * np.asarray(absref, dtype=np.longdouble).reshape(-1)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def gll_exact_diag(nq_iso, dim, lam):
    """The diagonal on helm_ref.gll_setup() data (Legendre modes at the GLL points, G = I * weight, w = weight), in closed
    form: lam prod_d m[p_d] + sum_a s[p_a] prod_{d != a} m[p_d], m[p] = 2 / (2p + 1) = int P_p^2, s[p] = p (p + 1) =
    int P_p'^2 (both integrands are of degree <= 2 nq - 4: the nq-point GLL rule is exact).  One element, flat [r][q][p]."""
    p = np.arange(nq_iso - 1, dtype=np.float64)
    m, s = 2.0 / (2.0 * p + 1.0), p * (p + 1.0)
    out = 0.0
    for a in range(-1, dim):
        fac = [(s if d == a else m) for d in range(dim)]          # direction 0 is the last axis
        term = fac[dim - 1]
        for d in reversed(range(dim - 1)):
            term = np.multiply.outer(term, fac[d])
        out = out + (lam * term if a < 0 else term)
    return np.asarray(out).reshape(-1)
