"""Reference and error bounds of the gradient, divergence and curl of a vector field (include/sumfact.h sf_vecgrad_*) for
tests/test_vecgrad_cpu.py and tests/test_gpu_vecgrad.py.  Imports nothing of the product.

    u_a = B in_a,   J[a][b] = D_b u_a,   grad[a][j] = sum_b df[j d + b] J[a][b],
    div = sum_a grad[a][a],   3D: curl = (grad[2][1] - grad[1][2], grad[0][2] - grad[2][0], grad[1][0] - grad[0][1]),
    2D: curl = grad[1][0] - grad[0][1]                                                       (a, b, j = 0 .. d-1)

B the tensor-product BwdTrans basis (bases nm x nq row-major), D_b row-major nq x nq with (D_b u)[i] = sum_m D_b[i][m]
u[m], df[e][c][k][j][i] the d*d planes of the inverse Jacobian, c = a d + b for d xi_b / d x_a.  `x` holds the d fields,
shape (d, nelmt * nm^d) or a sequence of d flat arrays.  A result is a dict: "grad" flat in the layout of the device,
[e][c][point] with c = a d + j; "div" flat, [e][point]; "curl" of shape (3, nelmt * nq^3) in 3D and flat in 2D.

The reference runs step by step, in the order above, in np.longdouble (80-bit on x86-64, eps 2^-63): its own error is
negligible against the bound.  Elementwise bound of a computed result:  |got - ref| <= gamma_N * absref,
gamma_N = N u / (1 - N u), with

    N_grad = sum_d nq_d + max_d nq_d + d           (physderiv_n: the entry is an output of sf_physderiv_* on in_a)
    N_div  = N_grad + d - 1                        (d - 1 additions)   on   sum_a absref[a][a]
    N_curl = N_grad + 1                            (one subtraction)   on   the sum of the two absref entries

u = 2^-53 (fp64) or 2^-24 (fp32), absref of grad = the same operator applied to |B|, |D|, |df| and |x|.  The bounds are
derived, not tuned, and hold for any summation order.  A zero bound needs a zero error.
"""
import math

import numpy as np

from iprod_ref import U32, U64, gamma, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps
from physderiv_ref import _apply, physderiv_n

OUTPUTS = ("grad", "div", "curl")
CURL_PAIRS = {2: (((1, 0), (0, 1)),), 3: (((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))}


def vecgrad_n(nq, name):
    """The count N of the bound of output `name`."""
    n = physderiv_n(nq)
    return {"grad": n, "div": n + len(nq) - 1, "curl": n + 1}[name]


def _fields(x):
    if isinstance(x, np.ndarray):
        return [x[a] for a in range(x.shape[0])]
    return list(x)


def _grad(nq, nelmt, bases, derivs, df, x, dt, mutate=None):
    """g[a][j] as arrays of shape [e][k][j][i]."""
    nq = tuple(int(q) for q in nq)
    dim = len(nq)
    shape = (nelmt,) + tuple(reversed(nq))
    D = [np.asarray(derivs[d], dtype=dt).reshape(nq[d], nq[d]) for d in range(dim)]
    dd = np.asarray(df, dtype=dt).reshape((nelmt, dim * dim) + shape[1:])
    xs = _fields(x)
    assert len(xs) == dim
    g = []
    for a in range(dim):
        u = _forward_sweeps(nq, nelmt, bases, xs[a], dt).reshape(shape)
        J = [_apply(b, D[b], u) for b in range(dim)]
        row = []
        for j in range(dim):
            s = None
            for b in range(dim):
                plane = dd[:, b * dim + j] if mutate == "df-transposed" else dd[:, j * dim + b]
                term = plane * J[b]
                s = term if s is None else s + term
            row.append(s)
        g.append(row)
    return g


def _assemble(g, nelmt, absolute, mutate=None):
    """The dict of outputs from g[a][j]; absolute: the entries are absref, differences become sums."""
    dim = len(g)
    n = g[0][0].size
    stored = [[g[j][a] if mutate == "grad-transposed" else g[a][j] for j in range(dim)] for a in range(dim)]
    grad = np.stack([stored[c // dim][c % dim].reshape(nelmt, -1) for c in range(dim * dim)], axis=1).reshape(-1)
    if mutate == "div-row":
        terms = [g[0][j] for j in range(dim)]
    else:
        terms = [g[a][a] for a in range(dim)]
    div = terms[0]
    for t in terms[1:]:
        div = div + t
    curl = []
    for (p, q), (r, s) in CURL_PAIRS[dim]:
        c = g[p][q] + g[r][s] if absolute else g[p][q] - g[r][s]
        curl.append((-c if mutate == "curl-sign" and not absolute else c).reshape(-1))
    curl = np.stack(curl) if dim == 3 else curl[0]
    assert div.size == n
    return {"grad": grad, "div": np.ascontiguousarray(div).reshape(-1), "curl": curl}


def _abs(a, dt):
    return np.abs(np.asarray(a, dtype=dt))


def ref_vecgrad(nq, nelmt, bases, derivs, df, x):
    """(ref, absref): two dicts of np.longdouble arrays."""
    ld = np.longdouble
    ref = _assemble(_grad(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], derivs, df, x, ld), nelmt, False)
    absref = _assemble(_grad(nq, nelmt, [_abs(b, ld) for b in bases], [_abs(d, ld) for d in derivs], _abs(df, ld),
                             [_abs(v, ld) for v in _fields(x)], ld), nelmt, True)
    return ref, absref


def vecgrad_eval(nq, nelmt, bases, derivs, df, x, dt=np.float64, mutate=None):
    """The outputs with every step in dt (reshaped matmuls): an evaluation in working precision, and the deliberately
    wrong variants of the CPU tests -- "df-transposed" (df[b d + j] in the place of df[j d + b]), "grad-transposed"
    (grad[j][a] stored as plane a d + j), "curl-sign" (the curl negated), "div-row" (the divergence sums row 0 of grad
    instead of the diagonal)."""
    return _assemble(_grad(nq, nelmt, [np.asarray(b, dtype=dt) for b in bases], derivs, df, x, dt, mutate), nelmt, False,
                     mutate)


def output_excess(got, ref, absref, nq, u, name, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref) of one output; <= 1 passes.  Zero bound needs zero
    error."""
    gN = gamma(vecgrad_n(nq, name), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * gN * np.asarray(absref, dtype=np.longdouble)
    assert err.shape == bound.shape, (name, err.shape, bound.shape)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def vecgrad_excess(got, ref, absref, nq, u, factor=1.0):
    """{name: output_excess} over the outputs that `got` holds."""
    return {name: output_excess(got[name], ref[name], absref[name], nq, u, name, factor) for name in got}
