"""Reference and error bound of the tensor-product apply with independent input / output extents (include/sumfact.h
sf_tensor_*) for tests/test_tensor_cpu.py and tests/test_gpu_tensor.py.  Imports nothing of the product.

    3D: out[e][k][j][i] = sum_r sum_q sum_p in[e][r][q][p] M0(p,i) M1(q,j) M2(r,k)
    2D: out[e][j][i]    = sum_q sum_p       in[e][q][p]    M0(p,i) M1(q,j)
    trans = 0: M_d(a,b) = m_d[a*no_d + b] (row-major ni_d x no_d);  trans = 1: M_d(a,b) = m_d[b*ni_d + a] (no_d x ni_d)

The reference runs sweep by sweep (direction 0, then 1, then 2) in np.longdouble (80-bit on x86-64, eps 2^-63), so its own
error is negligible against the bound.

The bound is the derivation of bwd_ref.py with nm_d replaced by ni_d.  The sweep of direction d is an inner product of
ni_d terms; computed in any order, with or without FMA, it carries at most ni_d rounding errors on any one product, so
|fl(sum) - sum| <= gamma_{ni_d} sum |a_m| |b_m| with gamma_n = n u / (1 - n u).  The next sweep takes the computed values
as data, relative errors of chained inner products compose, (1 + gamma_a)(1 + gamma_b) <= 1 + gamma_{a + b}, hence

    |got - ref| <= gamma_N absref,   N = tensor_n(ni) = sum_d ni_d,   absref = the same sweeps on |M| and |x|,

u = 2^-53 (fp64) or 2^-24 (fp32).  ni_d = 1 is one multiplication and counts 1.  Derived, not tuned; a zero bound needs a
zero error.
"""
import math

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24


def gamma(n, u):
    return n * u / (1.0 - n * u)


def unit_roundoff(dtype_name):
    return U32 if str(dtype_name).endswith("float32") else U64


def tensor_n(ni):
    """N of the bound: sum_d ni_d, one rounding per term of each sweep's inner product."""
    return sum(int(a) for a in ni)


def matrices(ni, no, trans, mats, dt):
    """M_d as ni_d x no_d arrays of dtype dt, from the flat arrays the C call takes."""
    out = []
    for a, b, m in zip(ni, no, mats):
        m = np.asarray(m, dtype=dt).reshape(-1)
        assert m.size == a * b, (m.size, a, b)
        out.append(m.reshape(b, a).T if trans else m.reshape(a, b))
    return out


def sweeps(ni, no, nelmt, M, x, dt):
    """The sweeps in dtype dt, direction 0 first; M_d is ni_d x no_d; x holds nelmt * prod(ni) values."""
    ni, no = [int(a) for a in ni], [int(b) for b in no]
    x = np.asarray(x, dtype=dt)
    if len(ni) == 3:
        u = x.reshape(nelmt, ni[2], ni[1], ni[0])
        w1 = u @ M[0]                                                        # [e][r][q][i]
        w2 = M[1].T @ w1                                                     # [e][r][j][i]
        out = M[2].T @ w2.reshape(nelmt, ni[2], no[1] * no[0])               # [e][k][(j,i)]
    else:
        u = x.reshape(nelmt, ni[1], ni[0])
        w1 = u @ M[0]                                                        # [e][q][i]
        out = M[1].T @ w1                                                    # [e][j][i]
    return np.ascontiguousarray(out).reshape(-1)


def ref_tensor(ni, no, trans, nelmt, mats, x):
    """(ref, absref) in np.longdouble."""
    ld = np.longdouble
    M = matrices(ni, no, trans, mats, ld)
    xl = np.asarray(x, dtype=ld)
    return sweeps(ni, no, nelmt, M, xl, ld), sweeps(ni, no, nelmt, [np.abs(m) for m in M], np.abs(xl), ld)


def dense_tensor(ni, no, trans, nelmt, mats, x, dt=np.longdouble):
    """The same operator as one einsum contraction over all directions at once (no sweeps)."""
    M = matrices(ni, no, trans, mats, dt)
    x = np.asarray(x, dtype=dt)
    if len(ni) == 3:
        out = np.einsum("erqp,pi,qj,rk->ekji", x.reshape(nelmt, ni[2], ni[1], ni[0]), M[0], M[1], M[2])
    else:
        out = np.einsum("eqp,pi,qj->eji", x.reshape(nelmt, ni[1], ni[0]), M[0], M[1])
    return np.ascontiguousarray(out).reshape(-1)


def tensor_excess(got, ref, absref, ni, u, factor=1.0):
    """max over values of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  A NaN error gives inf, and so does a
    nonzero error where the bound is zero."""
    g = gamma(tensor_n(ni), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * g * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def adjoint_bound(ni, no, u):
    """The factor on sum_e <|A||x|, |y|>_e within which <A x, y> and <x, A^T y> agree when both applies and both dot
    products are computed with unit roundoff u: each apply errs by gamma_N (N = sum ni, resp. sum no) times the absolute
    operator, each dot product of m terms by gamma_m, and <|A||x|, |y|> = <|x|, |A^T||y|>."""
    m = max(int(np.prod([int(a) for a in ni])), int(np.prod([int(b) for b in no])))
    return gamma(tensor_n(ni), u) + gamma(tensor_n(no), u) + 2 * gamma(m, u)


def per_element_dots(a, b, nelmt):
    """fp64 dot product of every element's rows of a and b."""
    a = np.asarray(a, dtype=np.float64).reshape(nelmt, -1)
    b = np.asarray(b, dtype=np.float64).reshape(nelmt, -1)
    return np.einsum("ef,ef->e", a, b)
