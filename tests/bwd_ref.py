"""Reference and error bounds of BwdTrans (include/sumfact.h sf_bwdtrans_*) for tests/test_bwdtrans_cpu.py and
tests/test_gpu_bwdtrans_bounds.py.  Imports nothing of the product.

    3D: out[e][k][j][i] = sum_r sum_q sum_p in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k]
    2D: out[e][j][i]    = sum_q sum_p       in[e][q][p]    B0[p][i] B1[q][j]

The reference runs sweep by sweep (p -> i, q -> j, r -> k: mass_ref._forward_sweeps) in np.longdouble (80-bit on x86-64,
eps 2^-63), so its own error is negligible against the bounds.

The bound.  Each sweep is an inner product of nm_d = nq_d - 1 terms, sum_m a_m b_m.  Computed in any order of summation,
with or without FMA, it carries at most nm_d rounding errors on any one product (one multiplication and at most nm_d - 1
additions, or nm_d fused operations), so  |fl(sum) - sum| <= gamma_{nm_d} sum |a_m| |b_m|  with gamma_n = n u / (1 - n u)
(the standard forward bound of an inner product).  The next sweep takes these computed values as data: relative errors of
chained inner products compose, (1 + gamma_a)(1 + gamma_b) <= 1 + gamma_{a + b}, so after all sweeps

    |got - ref| <= gamma_N absref,   N = bwd_n(nq) = sum_d (nq_d - 1),   absref = the same sweeps on |B| and |x|,

u = 2^-53 (fp64) or 2^-24 (fp32).  A contraction zero-padded to a tile grid (the matrix-core kernels) adds exact zeros
-- 0 * finite = 0 and s + 0 = s without rounding -- so padding leaves N as it is.  nq_d = 2 has one mode: the "inner
product" is one multiplication, N counts it as 1.  The bound is derived, not tuned; a zero bound needs a zero error.

The one assumption: every multiply-add rounds once, to nearest.  That is IEEE for the vector ALU and taken as given for
the fp64 matrix instructions.  For v_mfma_f32_16x16x4_f32 (quad_mfma_kernel / hex_mfma_kernel with T = float: what fp32
AUTO runs at 2D nq 25..32 and 3D nq 13..16) it was measured instead: over every case of
tests/test_gpu_bwdtrans_bounds.py at those orders the worst |err| / (gamma_N absref) against the long-double reference
is 0.0182 (2D nq 26, 19 elements; 0.0177 between NaN bands at 2D nq 30 -- profiles/r17/bwdtrans_bounds.log), below what
the fp64 matrix kernels show (0.20), so no kernel gets a factor: all are held to gamma_N itself.
"""
import math

import numpy as np

from iprod_ref import U32, U64, f64_factor, gamma, unit_roundoff  # noqa: F401
from mass_ref import _forward_sweeps


def bwd_n(nq):
    """N of the bound: sum_d (nq_d - 1), one rounding per term of each sweep's inner product (module docstring)."""
    return sum(int(q) - 1 for q in nq)


def ref_bwdtrans(nq, nelmt, bases, x):
    """(ref, absref) in np.longdouble."""
    ld = np.longdouble
    ref = _forward_sweeps(nq, nelmt, [np.asarray(b, dtype=ld) for b in bases], np.asarray(x, dtype=ld), ld)
    absref = _forward_sweeps(nq, nelmt, [np.abs(np.asarray(b, dtype=ld)) for b in bases], np.abs(np.asarray(x, dtype=ld)), ld)
    return ref, absref


def bwd_f64(nq, nelmt, bases, x):
    """(out, absout) with fp64 sweeps (reshaped matmuls): for batches where long double is too slow."""
    f = np.float64
    return (_forward_sweeps(nq, nelmt, bases, np.asarray(x, dtype=f), f),
            _forward_sweeps(nq, nelmt, [np.abs(np.asarray(b, dtype=f)) for b in bases], np.abs(np.asarray(x, dtype=f)), f))


def bwd_f64_factor(nq, u):
    """The factor on gamma_N(u) absref64 for a result of unit roundoff u against bwd_f64: iprod_ref.f64_factor, the
    formula fused_families.Problem.f64_factor derives, at N = bwd_n(nq)."""
    return f64_factor(bwd_n(nq), u)


def bwd_excess(got, ref, absref, nq, u, factor=1.0):
    """max over elements of |got - ref| / (factor * gamma_N * absref); <= 1 passes.  A NaN error gives inf, and so does a
    nonzero error where the bound is zero."""
    g = gamma(bwd_n(nq), u)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bound = factor * g * np.asarray(absref, dtype=np.longdouble)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0
