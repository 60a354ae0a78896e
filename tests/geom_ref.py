"""Reference, running error bound and test inputs of the geometric factors (include/sumfact.h sf_geom_*, sf_geom_affine_*)
for tests/test_geom_cpu.py and tests/test_gpu_geom.py.  Imports nothing of the product.

    X_a = B x_a,  J[a][b] = D_b X_a,  cof, det, r = 1 / det,  df[a d + b] = cof[a][b] r,  w = |det| q,
    G_ab = w sum_x df[x d + a] df[x d + b]

in the order of operations the header states.  The reference runs in np.longdouble (80-bit on x86-64, eps 2^-63): its own
error is negligible against the bound.

The bound.  Next to every value the reference carries a FIRST-ORDER running bound e(.) of the error of a result computed
with unit roundoff u (2^-53 or 2^-24) in any association and with or without fused multiply-adds: every product and
every sum or difference is charged one rounding, u times the magnitude of its result.
  J       e(J) = gamma_N(u) absJ, N = physderiv_n(nq) (tests/physderiv_ref.py: the forward chain and one derivative sum),
          absJ the same sums over |B|, |D|, |x|.
  cof     3D  c = p q - r s:  e(c) = |q| e(p) + |p| e(q) + |s| e(r) + |r| e(s) + u (|p q| + |r s| + |c|)
          2D  c = +-J entry:  e(c) = e(J)
  det     t_0 = J00 c00, t_b = t_(b-1) + J0b c0b:
          e(t_b) = e(t_(b-1)) + |c0b| e(J0b) + |J0b| e(c0b) + u (|J0b c0b| + |t_b|)          (b = 0: no sum, u |t_0| once)
  r       e(r) = e(det) / det^2 + u |r|
  df      e(df) = |r| e(c) + |c| e(r) + u |df|
  q       e(q) = (d - 1) u |q|                                     (the weights are inputs: d - 1 products)
  w       e(w) = |q| e(det) + |det| e(q) + u |w|
  G       s_0 = df_0a df_0b, s_x = s_(x-1) + df_xa df_xb:
          e(s_x) = e(s_(x-1)) + |df_xb| e(df_xa) + |df_xa| e(df_xb) + u (|df_xa df_xb| + |s_x|)
          e(G) = |s| e(w) + |w| e(s) + u |G|
The assertion on a computed result is elementwise |got - ref| <= 2 e: the factor 2 covers the second-order terms that
the propagation drops.  That is valid while the relative errors stay small, which the reference asserts on every input
it is given (GeomRef.check_condition): e(det) <= 2^-10 |det| at every point.  The affine form has w = |det| (no q):
je with e(je) = e(det), ge with e(w) replaced by it.

Inputs (deformed()).  Per element A = I + 0.3 U(-1, 1)^(d x d) on the linear modes plus 0.1 U(-1, 1) (1 + sum_d m_d)^-3
on every mode, in the Legendre modal basis at the Gauss-Lobatto points (helm_ref.gll / legendre_basis) with the GLL
differentiation matrix and weights.  Measured in numpy at nq 3 / 5 / 8: det / det A in [0.88, 1.12], det A in
[0.48, 1.76], so the condition holds with a wide margin.  nq = 2 has one mode per direction and no linear mode: the
Jacobian of an isoparametric element with one mode is singular whatever the input, the condition cannot hold and the
bound says nothing there.
"""
import numpy as np

from helm_ref import COMPONENTS, gll, legendre_basis
from iprod_ref import U32, U64, gamma, unit_roundoff  # noqa: F401
from physderiv_ref import _physderiv, physderiv_n

LD = np.longdouble
OUTPUTS = ("df", "w", "g", "detj")
AFFINE_OUTPUTS = ("dfe", "ge", "je")


def sizes(nq):
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def gll_operands(nq):
    """(bases, derivs, qws) per direction: Legendre modes at the GLL points, differentiation matrix, weights."""
    out = [], [], []
    for q in nq:
        _, wts, D = gll(int(q))
        out[0].append(legendre_basis(int(q)))
        out[1].append(D.reshape(-1))
        out[2].append(wts)
    return out


def deformed(nq, nelmt, seed, affine=False):
    """(xs, A): xs[a] the nelmt * nm^d modes of coordinate a, A[e] the linear part.  affine: the linear modes only."""
    nq = tuple(int(q) for q in nq)
    d = len(nq)
    nm = [q - 1 for q in nq]
    rng = np.random.default_rng(seed)
    A = np.eye(d)[None] + 0.3 * rng.uniform(-1, 1, (nelmt, d, d))
    shape = tuple(reversed(nm))                                    # [r][q][p]
    idx = np.indices(shape)
    order = sum(idx[len(shape) - 1 - b] for b in range(d))          # sum_d m_d of every mode
    decay = (1.0 + order) ** -3.0
    xs = []
    for a in range(d):
        x = 0.1 * rng.uniform(-1, 1, (nelmt,) + shape) * decay
        if affine:
            x[:] = 0.0
            x.reshape(nelmt, -1)[:, 0] = rng.uniform(-1, 1, nelmt)      # a translation: it does not enter J
        for b in range(d):
            if nm[b] < 2:
                continue                                            # no linear mode in this direction
            at = [0] * d
            at[d - 1 - b] = 1
            x[(slice(None),) + tuple(at)] = (0.0 if affine else x[(slice(None),) + tuple(at)]) + A[:, a, b]
        xs.append(np.ascontiguousarray(x).reshape(-1))
    return xs, A


class GeomRef:
    """The reference values and their running bounds: .val[name], .err[name] for name in OUTPUTS + AFFINE_OUTPUTS, flat in
    the layouts of the C call, np.longdouble."""

    def __init__(self, nq, nelmt, bases, derivs, qws, xs, u):
        nq = tuple(int(q) for q in nq)
        d, nqt = len(nq), int(np.prod(nq))
        self.nq, self.nelmt, self.u, self.d, self.nqt = nq, nelmt, u, d, nqt
        gN = gamma(physderiv_n(nq), u)
        ab = lambda v: np.abs(np.asarray(v, dtype=LD))      # noqa: E731
        J, eJ = [], []
        for a in range(d):
            J.append(_physderiv(nq, nelmt, [np.asarray(b, dtype=LD) for b in bases], derivs, None, xs[a], LD)
                     .reshape(d, nelmt, nqt))
            eJ.append(gN * _physderiv(nq, nelmt, [ab(b) for b in bases], [ab(m) for m in derivs], None, ab(xs[a]), LD)
                      .reshape(d, nelmt, nqt))
        self.J, self.eJ = J, eJ                                     # J[a][b][e][point]
        cof = [[None] * d for _ in range(d)]
        ec = [[None] * d for _ in range(d)]
        if d == 3:
            for a in range(3):
                for b in range(3):
                    a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
                    p, q, r, s = J[a1][b1], J[a2][b2], J[a1][b2], J[a2][b1]
                    c = p * q - r * s
                    cof[a][b] = c
                    ec[a][b] = (np.abs(q) * eJ[a1][b1] + np.abs(p) * eJ[a2][b2] + np.abs(s) * eJ[a1][b2]
                                + np.abs(r) * eJ[a2][b1] + u * (np.abs(p * q) + np.abs(r * s) + np.abs(c)))
        else:
            cof[0][0], cof[0][1], cof[1][0], cof[1][1] = J[1][1], -J[1][0], -J[0][1], J[0][0]
            ec[0][0], ec[0][1], ec[1][0], ec[1][1] = eJ[1][1], eJ[1][0], eJ[0][1], eJ[0][0]
        det = J[0][0] * cof[0][0]
        edet = np.abs(cof[0][0]) * eJ[0][0] + np.abs(J[0][0]) * ec[0][0] + u * np.abs(det)
        for b in range(1, d):
            term = J[0][b] * cof[0][b]
            det = det + term
            edet = edet + np.abs(cof[0][b]) * eJ[0][b] + np.abs(J[0][b]) * ec[0][b] + u * (np.abs(term) + np.abs(det))
        self.det, self.edet = det, edet
        with np.errstate(divide="ignore", invalid="ignore"):
            r = 1 / det
            er = edet / (det * det) + u * np.abs(r)
            df = np.empty((nelmt, d * d, nqt), dtype=LD)
            edf = np.empty_like(df)
            for a in range(d):
                for b in range(d):
                    df[:, a * d + b] = cof[a][b] * r
                    edf[:, a * d + b] = np.abs(r) * ec[a][b] + np.abs(cof[a][b]) * er + u * np.abs(df[:, a * d + b])
            if qws is not None:
                qv = np.asarray(qws[0], dtype=LD)
                for b in range(1, d):
                    qv = np.multiply.outer(np.asarray(qws[b], dtype=LD), qv)
                qv = qv.reshape(1, nqt)
                eq = (d - 1) * u * np.abs(qv)
            else:
                qv, eq = np.ones((1, nqt), dtype=LD), np.zeros((1, nqt), dtype=LD)
            w = np.abs(det) * qv
            ew = np.abs(qv) * edet + np.abs(det) * eq + (u * np.abs(w) if qws is not None else 0)
            comps = COMPONENTS[d]
            g = np.empty((nelmt, len(comps), nqt), dtype=LD)
            eg = np.empty_like(g)
            for c, (a, b) in enumerate(comps):
                s = es = None
                for x in range(d):
                    fa, fb, ea, eb = df[:, x * d + a], df[:, x * d + b], edf[:, x * d + a], edf[:, x * d + b]
                    term = fa * fb
                    eterm = np.abs(fb) * ea + np.abs(fa) * eb
                    if s is None:
                        s, es = term, eterm + u * np.abs(term)
                    else:
                        s = s + term
                        es = es + eterm + u * (np.abs(term) + np.abs(s))
                g[:, c] = w * s
                eg[:, c] = np.abs(s) * ew + np.abs(w) * es + u * np.abs(g[:, c])
        flat = lambda v: np.ascontiguousarray(v).reshape(-1)      # noqa: E731
        self.val = {"df": flat(df), "w": flat(w), "g": flat(g), "detj": flat(det)}
        self.err = {"df": flat(edf), "w": flat(ew), "g": flat(eg), "detj": flat(edet)}
        if qws is None:                                             # the affine form: point 0 of every element
            self.val.update(dfe=flat(df[:, :, 0]), ge=flat(g[:, :, 0]), je=flat(np.abs(det)[:, 0]))
            self.err.update(dfe=flat(edf[:, :, 0]), ge=flat(eg[:, :, 0]), je=flat(edet[:, 0]))

    def check_condition(self, limit=2.0 ** -10):
        """The condition under which 2 e bounds the error: e(det) <= 2^-10 |det| at every point.  Returns the largest
        e(det) / |det|."""
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(self.det != 0, self.edet / np.abs(self.det), np.inf)
        worst = float(np.max(q))
        assert worst <= limit, f"the inputs are too close to singular for the bound: e(det) / |det| = {worst:.3g}"
        return worst

    def excess(self, name, got, elements=None):
        """max |got - ref| / (2 e) of output `name` (of the elements `elements` only); <= 1 passes.  A zero bound needs a
        zero error; a NaN fails."""
        ref, err = self.val[name], self.err[name]
        if elements is not None:
            per = ref.size // self.nelmt
            ref, err = ref.reshape(self.nelmt, per)[elements].reshape(-1), err.reshape(self.nelmt, per)[elements].reshape(-1)
        got = np.asarray(got, dtype=LD).reshape(-1)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        diff = np.abs(got - ref)
        if np.any(np.isnan(diff)) or np.any((err == 0) & (diff > 0)):
            return np.inf
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err > 0, diff / (2 * err), 0.0)
        return float(np.max(q)) if q.size else 0.0


def ref_geom(nq, nelmt, bases, derivs, qws, xs, u, affine=False, limit=2.0 ** -10):
    """GeomRef of a case, with the condition asserted.  affine: the reference of sf_geom_affine_* (no weights)."""
    ref = GeomRef(nq, nelmt, bases, derivs, None if affine else qws, xs, u)
    ref.check_condition(limit)
    return ref


def geom_eval(nq, nelmt, bases, derivs, qws, xs, dt, mutant=None):
    """The documented order of operations in dtype dt with numpy (each product and each sum rounded once: numpy has no
    fused multiply-add, and the bound charges both roundings), as a dict of flat arrays in the layouts of the C call.
    mutant: one of the deliberate errors the bound has to catch -- "transposed-cofactor", "g-order", "no-q", "signed-w",
    "c-order"."""
    nq = tuple(int(q) for q in nq)
    d, nqt = len(nq), int(np.prod(nq))
    cast = lambda v: np.asarray(v, dtype=dt)      # noqa: E731
    J = [_physderiv(nq, nelmt, [cast(b) for b in bases], derivs, None, xs[a], dt).reshape(d, nelmt, nqt) for a in range(d)]
    cof = [[None] * d for _ in range(d)]
    if d == 3:
        for a in range(3):
            for b in range(3):
                a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
                cof[a][b] = J[a1][b1] * J[a2][b2] - J[a1][b2] * J[a2][b1]
    else:
        cof[0][0], cof[0][1], cof[1][0], cof[1][1] = J[1][1], -J[1][0], -J[0][1], J[0][0]
    det = J[0][0] * cof[0][0]
    for b in range(1, d):
        det = det + J[0][b] * cof[0][b]
    r = dt(1) / det
    df = np.empty((nelmt, d * d, nqt), dtype=dt)
    for a in range(d):
        for b in range(d):
            c = cof[b][a] if mutant == "transposed-cofactor" else cof[a][b]
            df[:, (b * d + a) if mutant == "c-order" else (a * d + b)] = c * r
    qv = cast(qws[0])
    for b in range(1, d):
        qv = np.multiply.outer(cast(qws[b]), qv)
    qv = qv.reshape(1, nqt)
    if mutant == "no-q":
        qv = np.ones_like(qv)
    w = (det if mutant == "signed-w" else np.abs(det)) * qv
    comps = COMPONENTS[d]
    g = np.empty((nelmt, len(comps), nqt), dtype=dt)
    good = df if mutant != "c-order" else df.reshape(nelmt, d, d, nqt).transpose(0, 2, 1, 3).reshape(nelmt, d * d, nqt)
    for c, (a, b) in enumerate(comps):
        s = good[:, a] * good[:, b]
        for x in range(1, d):
            s = s + good[:, x * d + a] * good[:, x * d + b]
        g[:, c] = w * s
    if mutant == "g-order":
        g = g[:, ::-1]
    flat = lambda v: np.ascontiguousarray(v).reshape(-1)      # noqa: E731
    return {"df": flat(df), "w": flat(w), "g": flat(g), "detj": flat(det)}
