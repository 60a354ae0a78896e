"""CPU tests of the gradient and the weak divergence on affine elements (include/sumfact.h sf_aff_physderiv_*,
sf_aff_iprodderiv_*): the references of tests/affine_deriv_ref.py against the deformed references on expanded planes
and against the dense restatement, the transpose identity in long double, wrong component orders that must exceed the
bound (the tests can fail), the bound constants, the binding's symbol table and the header's text, and the registers of
every wave instantiation.  No GPU.
"""
import math
import os
import re

import numpy as np
import pytest

from affine_deriv_ref import (affine_iprodderiv_eval, affine_iprodderiv_excess, affine_iprodderiv_n, affine_physderiv_eval,
                              affine_physderiv_excess, affine_physderiv_n, expand_df, expand_w, ref_affine_iprodderiv,
                              ref_affine_physderiv)
from iprod_ref import U32, U64, gamma
from iprodderiv_ref import iprodderiv_n, ref_iprodderiv
from physderiv_ref import analytic_case, dense_physderiv, physderiv_n, ref_physderiv
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")
ULD = float(np.finfo(np.longdouble).eps) / 2                    # unit roundoff of the reference's own arithmetic
SHAPES = [(8, 8, 8), (3, 3, 3), (6, 4, 5), (2, 3, 2), (12, 12), (4, 9), (2, 2)]
STEMS = ("aff_physderiv", "aff_iprodderiv")
NEW = [f"sf_{stem}_{shape}_{sfx}" for stem in STEMS for shape in ("hex", "quad") for sfx in ("f64", "f64_variant", "f32")]


def _case(nq, nelmt, seed):
    rng = np.random.default_rng(seed)
    d, npt = len(nq), int(np.prod(nq))
    u = lambda n: rng.uniform(-1, 1, n)      # noqa: E731
    return dict(bases=[u((q - 1) * q) for q in nq], derivs=[u(q * q) for q in nq], qws=[u(q) for q in nq],
                dfe=u(nelmt * d * d), je=u(nelmt), x=u(nelmt * int(np.prod([q - 1 for q in nq]))), f=u((d, nelmt * npt)))


@pytest.mark.parametrize("nq", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_reference_is_the_deformed_one_on_expanded_planes(nq):
    """Long double against long double: the two restatements do the same operations, so they agree within the rounding of
    the reference's own arithmetic, gamma_N(2^-64) absref."""
    nelmt, c = 7, _case(nq, 7, 1)
    ref, absref = ref_affine_physderiv(nq, nelmt, c["bases"], c["derivs"], c["dfe"], c["x"])
    want, wabs = ref_physderiv(nq, nelmt, c["bases"], c["derivs"], expand_df(nq, nelmt, c["dfe"]), c["x"])
    assert ref.shape == want.shape == (len(nq), nelmt * int(np.prod(nq)))
    assert affine_physderiv_excess(ref, want, wabs, nq, ULD) <= 1.0
    assert affine_physderiv_excess(absref, wabs, wabs, nq, ULD) <= 1.0
    assert float(np.max(np.abs(want))) > 0
    for e in (0, nelmt - 1):                                    # and the dense restatement, element by element
        npt, nmt, dd = int(np.prod(nq)), int(np.prod([q - 1 for q in nq])), len(nq) ** 2
        dense = dense_physderiv(nq, c["bases"], c["derivs"], expand_df(nq, 1, c["dfe"][e * dd:(e + 1) * dd]),
                                c["x"][e * nmt:(e + 1) * nmt])
        assert affine_physderiv_excess(ref[:, e * npt:(e + 1) * npt], dense, absref[:, e * npt:(e + 1) * npt], nq, ULD,
                                       factor=2.0) <= 1.0      # each side within gamma_N of the truth


@pytest.mark.parametrize("with_je", [True, False], ids=["je", "no-je"])
@pytest.mark.parametrize("nq", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weak_divergence_reference_is_the_deformed_one_on_expanded_planes(nq, with_je):
    nelmt, c = 7, _case(nq, 7, 2)
    je = c["je"] if with_je else None
    ref, absref = ref_affine_iprodderiv(nq, nelmt, c["bases"], c["derivs"], c["qws"], c["dfe"], je, c["f"])
    want, wabs = ref_iprodderiv(nq, nelmt, c["bases"], c["derivs"], expand_df(nq, nelmt, c["dfe"]),
                                expand_w(nq, nelmt, c["qws"], je), c["f"])
    assert affine_iprodderiv_excess(ref, want, wabs, nq, ULD) <= 1.0
    assert affine_iprodderiv_excess(absref, wabs, wabs, nq, ULD) <= 1.0
    assert float(np.max(np.abs(want))) > 0


@pytest.mark.parametrize("nq", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transpose_identity_in_long_double(nq):
    """<affine_iprodderiv(f; je = None), x> = <f, affine_physderiv(x)> within (gamma_N1 + gamma_N2 + gamma_n) at the
    reference's roundoff times <|f|, |A| |x|>; n the length of the dot products."""
    nelmt, c = 5, _case(nq, 5, 3)
    atf, _ = ref_affine_iprodderiv(nq, nelmt, c["bases"], c["derivs"], None, c["dfe"], None, c["f"])
    ax, absax = ref_affine_physderiv(nq, nelmt, c["bases"], c["derivs"], c["dfe"], c["x"])
    ld = np.longdouble
    lhs, rhs = np.sum(atf * c["x"].astype(ld)), np.sum(c["f"].astype(ld) * ax)
    slack = np.sum(np.abs(c["f"]).astype(ld) * absax)
    n = max(atf.size, ax.size)
    bound = (gamma(affine_iprodderiv_n(nq), ULD) + gamma(affine_physderiv_n(nq), ULD) + 2 * gamma(n, ULD)) * slack
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0
    # the weighted call is the transpose of the gradient followed by the weight: diag(w) enters linearly
    w = expand_w(nq, nelmt, c["qws"], c["je"])
    wf, _ = ref_affine_iprodderiv(nq, nelmt, c["bases"], c["derivs"], c["qws"], c["dfe"], c["je"], c["f"])
    rhs_w = np.sum((w[None] * c["f"].astype(ld)) * ax)
    slack_w = np.sum(np.abs(w)[None] * np.abs(c["f"]).astype(ld) * absax)
    assert abs(np.sum(wf * c["x"].astype(ld)) - rhs_w) <= bound / slack * slack_w + gamma(len(nq) + 1, ULD) * slack_w


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 4, 3), (12, 12), (4, 9)], ids=lambda s: "x".join(map(str, s)))
def test_fp64_and_fp32_evaluations_meet_the_bound_and_wrong_orders_do_not(nq):
    """The documented order of operations in fp64 and fp32 (numpy) is inside gamma_N absref of the long-double
    reference; a transposed dfe, a dfe read with the column index first, swapped quadrature weights or a weight that
    leaves one direction out are outside it by orders of magnitude: the bound can tell."""
    nelmt, c = 9, _case(nq, 9, 4)
    d = len(nq)
    B, D, Q, f = c["bases"], c["derivs"], c["qws"], c["f"]
    gref, gabs = ref_affine_physderiv(nq, nelmt, B, D, c["dfe"], c["x"])
    wref, wabs = ref_affine_iprodderiv(nq, nelmt, B, D, Q, c["dfe"], c["je"], f)
    for dt, u in ((np.float64, U64), (np.float32, U32)):
        r = lambda a: [np.asarray(v, dtype=dt).astype(np.float64) for v in a]      # noqa: E731  inputs rounded to dt
        rb, rd, rq = r(B), r(D), r(Q)
        rdfe, rje, rx, rf = (np.asarray(v, dtype=dt).astype(np.float64) for v in (c["dfe"], c["je"], c["x"], f))
        gr, ga = ref_affine_physderiv(nq, nelmt, rb, rd, rdfe, rx)
        wr, wa = ref_affine_iprodderiv(nq, nelmt, rb, rd, rq, rdfe, rje, rf)
        g = affine_physderiv_eval(nq, nelmt, rb, rd, rdfe, rx, dt)
        w = affine_iprodderiv_eval(nq, nelmt, rb, rd, rq, rdfe, rje, rf, dt)
        assert g.dtype == dt and w.dtype == dt
        qg, qw = affine_physderiv_excess(g, gr, ga, nq, u), affine_iprodderiv_excess(w, wr, wa, nq, u)
        print(f"{nq} {np.dtype(dt).name}: gradient {qg:.3g}, weak divergence {qw:.3g}")
        assert qg <= 1.0 and qw <= 1.0
    dfe_t = c["dfe"].reshape(nelmt, d, d).transpose(0, 2, 1).reshape(-1)
    bad = affine_physderiv_eval(nq, nelmt, B, D, dfe_t, c["x"], np.float64)
    assert affine_physderiv_excess(bad, gref, gabs, nq, U64) > 1e6
    bad = affine_iprodderiv_eval(nq, nelmt, B, D, Q, dfe_t, c["je"], f, np.float64)
    assert affine_iprodderiv_excess(bad, wref, wabs, nq, U64) > 1e6
    if len(set(nq[:2])) == 1:                                   # swapped weights of two directions of the same extent
        bad = affine_iprodderiv_eval(nq, nelmt, B, D, [Q[1], Q[0]] + Q[2:], c["dfe"], c["je"], f, np.float64)
        assert affine_iprodderiv_excess(bad, wref, wabs, nq, U64) > 1e6
    ones = [Q[0]] + [np.ones_like(q) for q in Q[1:]]            # q = qw0[i] alone
    bad = affine_iprodderiv_eval(nq, nelmt, B, D, ones, c["dfe"], c["je"], f, np.float64)
    assert affine_iprodderiv_excess(bad, wref, wabs, nq, U64) > 1e6


def test_weight_association_defines_the_bits():
    """w = je * (qw2 * (qw1 * qw0)) in the working precision: another association rounds differently somewhere, so the
    bit-equality tests of the GPU files depend on this one (and can fail)."""
    nq, nelmt = (8, 8, 8), 11
    c = _case(nq, nelmt, 5)
    for dt in (np.float64, np.float32):
        q = [np.asarray(v, dtype=dt) for v in c["qws"]]
        je = np.asarray(c["je"], dtype=dt)
        w = expand_w(nq, nelmt, q, je, dt)
        assert w.dtype == dt
        k, j, i = 5, 3, 6
        assert w.reshape(nelmt, 8, 8, 8)[4, k, j, i] == je[4] * (q[2][k] * (q[1][j] * q[0][i]))
        other = ((je.reshape(-1, 1, 1, 1) * q[2].reshape(1, -1, 1, 1)) * q[1].reshape(1, 1, -1, 1)) * q[0].reshape(1, 1, 1, -1)
        assert not np.array_equal(w, other.reshape(-1))
        assert np.max(np.abs(w - other.reshape(-1)) / np.abs(w)) <= 4 * np.finfo(dt).eps


@pytest.mark.parametrize("dim,nq", [(3, 6), (2, 9)], ids=["3d-nq6", "2d-nq9"])
def test_analytic_gradient_on_affine_elements(dim, nq):
    """analytic_case of tests/physderiv_ref.py with dfe taken from its A_e^-1: the reference is within 0.5 gamma_N absref
    of the exact gradient of the polynomial."""
    nelmt, ext = 5, (nq,) * dim
    bases, derivs, df, x, exact = analytic_case(nq, dim, nelmt)
    planes = df.reshape(nelmt, dim * dim, -1)
    assert np.array_equal(planes, np.broadcast_to(planes[:, :, :1], planes.shape))      # affine: constant planes
    dfe = np.ascontiguousarray(planes[:, :, 0]).reshape(-1)
    ref, absref = ref_affine_physderiv(ext, nelmt, bases, derivs, dfe, x)
    assert affine_physderiv_excess(ref, exact, absref, ext, U64) <= 0.5
    assert float(np.max(np.abs(exact))) > 0.1


def test_bound_constants():
    assert affine_physderiv_n((8, 8, 8)) == physderiv_n((8, 8, 8)) == 24 + 8 + 3
    assert affine_iprodderiv_n((8, 8, 8)) == iprodderiv_n((8, 8, 8)) + 3 == 24 + 8 + 9
    assert affine_iprodderiv_n((4, 9)) == 13 + 9 + 6
    assert math.isinf(affine_physderiv_excess(np.ones(1), np.zeros(1), np.zeros(1), (8, 8), U64))
    assert math.isinf(affine_iprodderiv_excess(np.ones(1), np.zeros(1), np.zeros(1), (8, 8), U64))


def test_binding_and_header_name_the_new_symbols():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_capi_text", os.path.join(PKG, "capi.py"))
    capi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(capi)
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS, name
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(capi.SYMBOLS[name][1]), (name, params)
    declared = set(re.findall(r"\b(sf_aff_(?:physderiv|iprodderiv)_\w+)\s*\(", text))
    assert declared == set(NEW) == {n for n in capi.SYMBOLS if re.match(r"sf_aff_(physderiv|iprodderiv)_", n)}
    three_d = capi.SYMBOLS["sf_aff_iprodderiv_hex_f64_variant"][1]
    assert len(three_d) == 1 + 3 + 1 + 9 + 2 + 3 + 1 + 1            # variant, nq, nelmt, bases derivs qw, dfe je, in_a, out, stream
    assert len(capi.SYMBOLS["sf_aff_physderiv_quad_f32"][1]) == 2 + 1 + 4 + 1 + 1 + 2 + 1
    for needle in ("out_a[e][k][j][i] = sum_b dfe[e][a*d + b] * du_b[e][k][j][i]", "dfe is required",
                   "g_b = (je[e] * q) * t_b", "q   = qw2[k] * (qw1[j] * qw0[i])", "w = je * (qw2 * (qw1 * qw0))",
                   "je and every qw_d are then never read (nor validated)", "overlapping any in_a, `dfe` or `je`",
                   "any out_a overlapping `in`, `dfe` or another out_b"):
        assert needle in text, needle


NAME = re.compile(r"(hex|quad)_affine_(physderiv|iprodderiv)_wave_kernel<(\d+), .*(float|double)>")


def test_wave_instantiations_use_no_scratch():
    """Every wave instantiation of the two families: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq
    2..8 and 2D nq 2..16 for double and float, the gradient once and the weak divergence with and without je (132).
    Prints VGPRs / occupancy per kernel (the table of DESIGN.md s4.17)."""
    got = set()
    for src, r in kernel_resources(("affine_deriv.hip", "affine_deriv_f32.hip"), "deriv_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, op, nq, t = 3 if m.group(1) == "hex" else 2, m.group(2), int(m.group(3)), m.group(4)
        flag = re.search(r", (true|false), (?:float|double)>$", r.name)
        assert (flag is not None) == (op == "iprodderiv"), r.name
        assert (t == "float") == (src == "affine_deriv_f32.hip"), (src, r.name)
        got.add((op, dim, nq, t, flag.group(1) == "true" if flag else None))
        print(f"{op:10s} {dim}D nq {nq:2d} {t:6s} {'' if not flag else 'je' if flag.group(1) == 'true' else '--'}: "
              f"{r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(op, d, n, t, h) for d, n in orders for t in ("double", "float")
            for op, hs in (("physderiv", (None,)), ("iprodderiv", (True, False))) for h in hs}
    assert len(want) == 132 and got == want, sorted(map(str, want ^ got))
