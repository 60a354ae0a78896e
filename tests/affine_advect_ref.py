"""Reference and error bound of the weak advection term on affine elements (include/sumfact.h sf_aff_advect_*) for
tests/test_affine_advect_cpu.py and tests/test_gpu_affine_advect.py.  Imports nothing of the product.

    u_a = B in_a,   J[a][b] = D_b u_a,   beta_b = sum_j c_j dfe[e][j d + b],   q = qw2[k] (qw1[j] qw0[i]),
    r_a = (je[e] q) (sum_b beta_b J[a][b]),   out_a = B^T r_a                  (je None: r_a = sum_b beta_b J[a][b])

dfe[e][c] the d*d constants of the element's inverse Jacobian, c = a d + b for d xi_b / d x_a (the order of the planes of
sf_advect_*'s df; not symmetric), je[e] one scalar per element, qw_d the one-dimensional quadrature weights, c_j[e][k][j][i]
the d planes of the advecting velocity.  `x` holds the nf fields, shape (nf, nelmt * nm^d) or a sequence of nf flat arrays;
results have the shape (nf, nelmt * nm^d): row a is out_a.  The evaluation below broadcasts the constants of an element
over its points and runs step by step, in the order above, in a dtype of the caller's choice: np.longdouble for the
reference (80-bit on x86-64, eps 2^-63: its own error is negligible against the bound).  It does not call
tests/advect_ref.py's _advect: the CPU tests compare the two restatements on expanded planes.

Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,  gamma_N = N u / (1 - N u),

    N = advect_n(nq) + d = 2 sum_d nq_d + max_d nq_d + 3 d + 1

-- advect_n counts ONE rounding for the weight w (the product with the sum); here the weight is formed in the working
precision from d + 1 numbers: d - 1 products for q, one for je q, and the product with the sum that advect_n already
holds, hence d more -- the step affine_iprodderiv_n takes over iprodderiv_n.  u = 2^-53 (fp64) or 2^-24 (fp32); absref =
the same operator applied to the absolute values of everything.  Derived, not tuned; holds for any summation order; kept
for je = None, where the weight operations do not happen.  A zero bound needs a zero error.
"""
import math

import numpy as np

from advect_ref import _fields, advect_n
from affine_deriv_ref import _apply, _consts, expand_df, expand_w  # noqa: F401  (the expansions: for the callers)
from affine_ref import point_weights
from iprod_ref import U32, U64, _sweeps as _transposed_sweeps, gamma, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps


def affine_advect_n(nq, with_je=True):
    """The count of the bound; the same with and without je (without, d + 1 of the counted operations do not happen)."""
    del with_je
    return advect_n(nq) + len(nq)


def affine_advect_eval(nq, nelmt, bases, derivs, qws, dfe, je, c, x, dt, mutate=None):
    """The nf outputs in dtype dt, shape (nf, nelmt * nm^d); je None: no weight, qws is not looked at.
    mutate: None, or a deliberately wrong variant for the tests of the bound -- "dfe-transposed" (dfe[b d + j] in the
    place of dfe[j d + b]), "weight-short" (q without the last direction), "qw-swapped" (the weights of the first two
    directions of equal extent exchanged), "weight-left" (the weight formed as ((je qw2) qw1) qw0: right within rounding,
    other bits)."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))                        # [e][k][j][i] / [e][j][i]
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    dd = _consts(dfe, nelmt, dim, dt)
    cs = [np.asarray(v, dtype=dt).reshape(shape) for v in _fields(c)]
    assert len(cs) == dim
    beta = []
    for b in range(dim):
        s = None
        for j in range(dim):
            const = dd[:, b * dim + j] if mutate == "dfe-transposed" else dd[:, j * dim + b]
            term = cs[j] * const
            s = term if s is None else s + term
        beta.append(s)
    w = None
    if je is not None:
        q = [np.asarray(v, dtype=dt) for v in qws]
        jee = np.asarray(je, dtype=dt).reshape((nelmt,) + (1,) * dim)
        if mutate == "weight-short":
            q = q[:-1] + [np.ones_like(q[-1])]
        if mutate == "qw-swapped":
            a, b = next((a, b) for a in range(dim) for b in range(a + 1, dim) if nq[a] == nq[b])
            q[a], q[b] = q[b], q[a]
        if mutate == "weight-left":
            w = jee
            for d in reversed(range(dim)):
                w = w * q[d].reshape((1,) + tuple(-1 if a == dim - 1 - d else 1 for a in range(dim)))
        else:
            w = jee * point_weights(nq, q, dt)[None]
    bs = [np.asarray(b, dtype=dt) for b in bases]
    xs = _fields(x)
    assert len(xs) in (1, dim)
    J = []
    for xa in xs:
        u = _forward_sweeps(nq, nelmt, bs, np.asarray(xa, dtype=dt), dt).reshape(shape)
        J.append([_apply(b, D[b], u) for b in range(dim)])
    out = []
    for a in range(len(xs)):
        s = None
        for b in range(dim):
            term = beta[b] * J[a][b]
            s = term if s is None else s + term
        r = s if w is None else w * s
        out.append(_transposed_sweeps(nq, nelmt, bs, np.ascontiguousarray(r).reshape(-1), dt))
    return np.stack(out)


def _abs(a):
    return None if a is None else np.abs(np.asarray(a))


def _absl(seq):
    return None if seq is None else [_abs(a) for a in seq]


def ref_affine_advect(nq, nelmt, bases, derivs, qws, dfe, je, c, x, dt=np.longdouble):
    """(ref, absref) in np.longdouble (or dt), each of shape (nf, nelmt * nm^d).  je may be None."""
    qa = None if je is None else _absl(qws)
    return (affine_advect_eval(nq, nelmt, bases, derivs, qws, dfe, je, c, x, dt),
            affine_advect_eval(nq, nelmt, _absl(bases), _absl(derivs), qa, _abs(dfe), _abs(je), _absl(_fields(c)),
                               _absl(_fields(x)), dt))


def affine_advect_excess(got, ref, absref, nq, u, factor=1.0, with_je=True):
    """max over values of |got - ref| / (factor * gamma_N * absref), N = advect_n + d; <= 1 passes.  Zero bound needs
    zero error."""
    gN = gamma(affine_advect_n(nq, with_je), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0
