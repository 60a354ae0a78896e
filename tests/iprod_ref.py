"""Reference and error bounds of IProductWRTBase for tests/test_iproduct_cpu.py and tests/test_gpu_iproduct.py.

    3D: out[e][r][q][p] = sum_k sum_j sum_i in[e][k][j][i] B0[p][i] B1[q][j] B2[r][k]
    2D: out[e][q][p]    = sum_j sum_i       in[e][j][i]    B0[p][i] B1[q][j]

The reference runs sweep by sweep (i -> p, j -> q, k -> r) in np.longdouble (80-bit on x86-64, eps 2^-63), so its own
error is negligible against the bounds.  Elementwise bound of a computed result (the standard forward bound of chained
inner products, with or without FMA):  |gpu - ref| <= gamma_n * absref,  gamma_n = n u / (1 - n u),  n = nq0 + nq1
(+ nq2), u = 2^-53 (fp64) or 2^-24 (fp32), absref = the same contraction applied to |B| and |x|.
"""
import math

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24


def gamma(n, u):
    return n * u / (1.0 - n * u)


def unit_roundoff(dtype_name):
    return U32 if dtype_name == "float32" else U64


def f64_factor(n, u):
    """The factor on gamma_n(u) absref64 for a result of unit roundoff u against an fp64 reference of the same n.  The
    result is within gamma_n(u) and the reference within gamma_n(u64) of the truth, both times the exact absolute operator,
    and that is at most (1 + gamma_n) absref64: (1 + gamma_n(u64) / gamma_n(u)) (1 + gamma_n(u)).  For an fp64 result this
    is the 2 (1 + gamma_n) of the families' large-batch tests; for a float32 one it is 1 + 2e-9 times (1 + gamma_n)."""
    return (1 + gamma(n, U64) / gamma(n, u)) * (1 + gamma(n, u))


def _sweeps(nq, nelmt, bases, x, dt):
    """Sweeps in dtype dt; x holds nelmt * prod(nq) points, bases are nm x nq row-major."""
    nq = tuple(int(q) for q in nq)
    nm = [q - 1 for q in nq]
    b = [np.asarray(bases[d], dtype=dt).reshape(nm[d], nq[d]) for d in range(len(nq))]
    x = np.asarray(x, dtype=dt)
    if len(nq) == 3:
        u = x.reshape(nelmt, nq[2], nq[1], nq[0])
        w1 = u @ b[0].T                                              # [e][k][j][p]
        w2 = b[1] @ w1                                               # [e][k][q][p]
        out = b[2] @ w2.reshape(nelmt, nq[2], nm[1] * nm[0])         # [e][r][(q,p)]
    else:
        u = x.reshape(nelmt, nq[1], nq[0])
        w1 = u @ b[0].T                                              # [e][j][p]
        out = b[1] @ w1                                              # [e][q][p]
    return np.ascontiguousarray(out).reshape(-1)


def ref_iprod(nq, nelmt, bases, x):
    """(ref, absref) in np.longdouble."""
    ld = np.longdouble
    ref = _sweeps(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], np.asarray(x, dtype=ld), ld)
    absref = _sweeps(nq, nelmt, [np.abs(np.asarray(b, dtype=ld)) for b in bases], np.abs(np.asarray(x, dtype=ld)), ld)
    return ref, absref


def iprod_f64(nq, nelmt, bases, x):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    f = np.float64
    return (_sweeps(nq, nelmt, bases, np.asarray(x, dtype=f), f),
            _sweeps(nq, nelmt, [np.abs(np.asarray(b, dtype=f)) for b in bases], np.abs(np.asarray(x, dtype=f)), f))


def elementwise_excess(got, ref, absref, nq, u, factor=1.0):
    """max over elements of |got - ref| / (factor * gamma_n * absref); <= 1 passes.  Zero bound needs zero error."""
    g = gamma(sum(int(q) for q in nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * g * np.asarray(absref, dtype=np.longdouble)
    if np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def adjoint_bound(nq, u):
    """(2 gamma_n + 2 gamma_m), m = max(nq^d, nm^d): the adjointness bound's factor on sum_e <|B||x|, |y|>_e."""
    nq = [int(q) for q in nq]
    n = sum(nq)
    m = max(int(np.prod(nq)), int(np.prod([q - 1 for q in nq])))
    return 2 * gamma(n, u) + 2 * gamma(m, u)


def per_element_dots(a, b, nelmt):
    """fp64 dot product of every element's rows of a and b."""
    a = np.asarray(a, dtype=np.float64).reshape(nelmt, -1)
    b = np.asarray(b, dtype=np.float64).reshape(nelmt, -1)
    return np.einsum("ef,ef->e", a, b)
