"""GPU tests of the weak advection term on affine elements (include/sumfact.h sf_aff_advect_*) against the long-double
reference and its derived bound (tests/affine_advect_ref.py: elementwise |got - ref| <= gamma_N absref, N = advect_n + d),
and bit for bit against sf_advect_* on planes expanded on the device, on the seeded per-value-distinct data of
tests/affine_advect_families.py.  No tolerance is introduced anywhere: comparisons are bit for bit, against the derived
bound, or against the sum of two such bounds.  The SF_ENOTBUILT refusals, stream capture, the first call inside a capture
(and eagerly) and two streams in flight are the family's cases of tests/test_gpu_multifield_common.py.
"""
import numpy as np
import pytest

from advect_ref import advect_n, gamma, ref_advect
from affine_advect_families import (END_TO_END, FALLBACK, GUARD, MISALIGNED, NO_JE, POISON, RAGGED_BOUND, SCALAR, WAVE_COUNT,
                                    WAVE_ORDERS, AffineAdvectProblem)
from affine_advect_ref import affine_advect_n, ref_affine_advect, unit_roundoff
from fused_families import F32, F64, RAGGED, Banded, case_id, sf, to_host, torch_mod  # noqa: F401
from geom_families import GeomProblem
from iprod_ref import ref_iprod
from multifield_common import ids, odd, rows, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_within_the_bound_and_the_bits_of_the_deformed_call(sf, torch_mod, nq, dtype_name):
    """nf = d with je through AUTO (the wave kernel: the rows are aligned) against long double at every value, and bit
    for bit sf_advect_* on the expanded planes; in float64 "wave" and "generic" equal AUTO bit for bit, and each the
    deformed call on its own route."""
    p = AffineAdvectProblem(sf, torch_mod, nq, WAVE_COUNT, dtype_name, 5)
    auto = p.run()
    assert same_bits(torch_mod, auto, p.deformed()), nq
    if dtype_name == F64:
        assert same_bits(torch_mod, auto, p.run(variant="wave")), nq
        assert same_bits(torch_mod, auto, p.run(variant="generic")), nq
        assert same_bits(torch_mod, auto, p.deformed(variant="generic")), nq
    p.check(auto, "auto")


@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_through_auto_on_ragged_counts(sf, torch_mod, nq):
    """AUTO on prefixes of one problem at the ragged counts equals "generic" bit for bit; the first 257 elements are held
    to the bound once."""
    p = AffineAdvectProblem(sf, torch_mod, nq, max(RAGGED), F64, 3)
    for n in RAGGED:
        auto, generic = p.run(n), p.run(n, variant="generic")
        assert auto.shape == (p.d, n * p.nmt)
        assert same_bits(torch_mod, auto, generic), (nq, n)
        if n == RAGGED_BOUND:
            p.check(auto, f"ragged (first {n})", elements=np.arange(n))


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", NO_JE, ids=ids(NO_JE))
def test_no_je_never_reads_je_or_qw(sf, torch_mod, nq, nelmt, dtype_name):
    """je = None: bit for bit sf_advect_* with w a plane of ones; the same bits with the quadrature weights NaN-filled
    and, through the C call, with je and every qw_d NULL.  Within the bound, and not the weighted result."""
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, dtype_name, 31)
    plain = p.run(je=None)
    assert same_bits(torch_mod, plain, p.deformed(je=None)), nq
    nan = [torch_mod.full_like(t, float("nan")) for t in p.qs]
    assert same_bits(torch_mod, plain, p.run(je=None, qs=nan)), nq
    assert same_bits(torch_mod, plain, p.run(je=None, qs=[None] * p.d)), nq
    out = rows(torch_mod, p.d, nelmt * p.nmt, p.dtype, fill=0.0)
    rc = p.raw(p.d, [None] * p.d, p.dfe, None, [p.c[j] for j in range(p.d)], [p.x[a] for a in range(p.d)],
               [out[a] for a in range(p.d)])
    torch_mod.cuda.synchronize()
    assert rc == 0 and same_bits(torch_mod, out, plain), nq
    one = p.run(je=None, field=1)
    assert same_bits(torch_mod, one[0], plain[1]), nq
    p.check(plain, "no je", je=None)
    assert not same_bits(torch_mod, plain, p.run()) and not bool(torch_mod.isnan(plain).any())


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", SCALAR, ids=ids(SCALAR))
def test_scalar_transport_equals_the_vector_kernel(sf, torch_mod, nq, nelmt, dtype_name):
    """nf = 1 with in = in_a equals out_a of the nf = d call bit for bit, for every a; (8, 8, 8) runs one element per
    chunk: the constants through the scalar path."""
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, dtype_name, 9)
    vec = p.run()
    for a in range(p.d):
        one = p.run(field=a)
        assert one.shape == (1, nelmt * p.nmt)
        assert same_bits(torch_mod, one[0], vec[a]), (nq, a)
    assert same_bits(torch_mod, vec, p.deformed()) and float(vec.abs().max()) > 0


@pytest.mark.parametrize("nf", ["d", 1])
@pytest.mark.parametrize("nq,nelmt", FALLBACK, ids=ids(FALLBACK))
def test_fallback_shapes_within_the_bound(sf, torch_mod, nq, nelmt, nf):
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, F64, nelmt % 101)
    field = None if nf == "d" else p.d - 1
    auto, generic = p.run(field=field), p.run(field=field, variant="generic")
    assert same_bits(torch_mod, auto, generic)
    assert same_bits(torch_mod, generic, p.deformed(field=field, variant="generic"))
    p.check(generic, "generic", fields=None if field is None else [field])


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=ids(GUARD))
def test_guard_bands_and_nan_bands(sf, torch_mod, nq, nelmt):
    """Every out_a between guard words, every input -- dfe, je and the quadrature weights too -- between NaN bands:
    nothing is written outside the outputs, nothing read outside the inputs reaches a result.  With nf = 1 the slots
    out1.. of the C call are never written."""
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, F64, 17)
    clean = p.run()
    guard = -777.25
    band = lambda t: Banded.of(torch_mod, t)                                   # noqa: E731
    bs, ds, qs = [band(t) for t in p.bs], [band(t) for t in p.ds], [band(t) for t in p.qs]
    dfe, je = band(p.dfe), band(p.je)
    cs, xs = [band(p.c[j]) for j in range(p.d)], [band(p.x[a]) for a in range(p.d)]
    outs = [Banded(torch_mod, p.dtype, nelmt * p.nmt, 0, guard, lines=4) for _ in range(p.d)]
    over = dict(bs=[b.view for b in bs], ds=[b.view for b in ds], qs=[b.view for b in qs], dfe=dfe.view,
                c=[b.view for b in cs], x=[b.view for b in xs])
    got = p.run(je=je.view, out=[o.view for o in outs], **over)
    torch_mod.cuda.synchronize()
    assert all(o.bands_intact(torch_mod) for o in outs)
    assert all(b.bands_intact(torch_mod) for b in bs + ds + qs + [dfe, je] + cs + xs)
    for a in range(p.d):
        assert same_bits(torch_mod, got[a], clean[a]), (nq, a)
    assert not bool(torch_mod.isnan(clean).any()) and float(clean.abs().max()) > 0
    # nf = 1 through the C call with every slot filled: out1.. keep their guard words
    for o in outs:
        o.reset()
    rc = p.raw(1, [b.view for b in qs], dfe.view, je.view, [b.view for b in cs], [b.view for b in xs], [o.view for o in outs])
    torch_mod.cuda.synchronize()
    assert rc == 0
    assert same_bits(torch_mod, outs[0].view, clean[0]) and outs[0].bands_intact(torch_mod)
    for o in outs[1:]:
        assert bool((o.buf == guard).all())


@pytest.mark.parametrize("nq,nelmt", POISON, ids=ids(POISON))
def test_poison_in_the_constants_stays_in_its_element(sf, torch_mod, nq, nelmt):
    """NaN in one element's dfe, and separately in one element's je: only that element's outputs are NaN, in every field;
    everything else keeps its bits.  The last element of the batch is the one the clamped constant loads of a ragged
    last chunk read; the others sit inside a chunk."""
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, F64, 23)
    clean = p.run().reshape(p.d, nelmt, p.nmt)
    assert not bool(torch_mod.isnan(clean).any())
    for victim in (nelmt - 1, nelmt // 2, 1):
        keep = [e for e in range(nelmt) if e != victim]
        dfe = p.dfe.clone()
        dfe.reshape(nelmt, p.d * p.d)[victim] = float("nan")
        je = p.je.clone()
        je[victim] = float("nan")
        for what, kw in (("dfe", dict(dfe=dfe)), ("je", dict(je=je))):
            for variant in ("wave", "generic"):
                got = p.run(variant=variant, **kw).reshape(p.d, nelmt, p.nmt)
                nan = torch_mod.isnan(got)
                assert bool(nan[:, victim].all()) and int(nan.sum()) == p.d * p.nmt, (nq, victim, what, variant)
                assert same_bits(torch_mod, got[:, keep], clean[:, keep]), (nq, victim, what, variant)
        one = p.run(field=0, dfe=dfe).reshape(nelmt, p.nmt)
        assert bool(torch_mod.isnan(one[victim]).all()) and same_bits(torch_mod, one[keep], clean[0][keep])


def test_refusals(sf, torch_mod):
    """nf = 2 in 3D, nf = 0, a NULL dfe and too few fields: SF_EINVAL; a NULL qw_d with je: SF_EINVAL, without: fine."""
    c = sf.capi
    p = AffineAdvectProblem(sf, torch_mod, (4, 4, 4), 5, F64, 2)
    outs = [torch_mod.zeros(5 * p.nmt, dtype=p.dtype, device="cuda") for _ in range(3)]
    cs, xs = [p.c[j] for j in range(3)], [p.x[a] for a in range(3)]
    assert p.raw(2, p.qs, p.dfe, p.je, cs, xs, outs) == c.SF_EINVAL
    assert p.raw(0, p.qs, p.dfe, p.je, cs, xs, outs) == c.SF_EINVAL
    assert p.raw(3, p.qs, None, p.je, cs, xs, outs) == c.SF_EINVAL
    assert p.raw(3, [p.qs[0], None, p.qs[2]], p.dfe, p.je, cs, xs, outs) == c.SF_EINVAL
    assert p.raw(3, [p.qs[0], None, p.qs[2]], p.dfe, None, cs, xs, outs) == c.SF_OK
    assert p.raw(3, p.qs, p.dfe, p.je, cs, xs, outs) == c.SF_OK
    with pytest.raises(c.SumfactError) as ei:
        p.run(x=p.x[:2])
    assert ei.value.rc == c.SF_EINVAL


@pytest.mark.parametrize("nq,nelmt", MISALIGNED, ids=ids(MISALIGNED))
def test_misaligned_operands(sf, torch_mod, nq, nelmt):
    """dfe, je, qw_d and c_j at an odd scalar offset (8-byte aligned only) still take the wave route and give the same
    bits.  With in / out only 8-byte aligned AUTO takes "generic" and "wave" answers SF_EALIGN."""
    p = AffineAdvectProblem(sf, torch_mod, nq, nelmt, F64, 29)
    clean = p.run(variant="wave")
    odd_ = lambda t: odd(torch_mod, t)                                         # noqa: E731
    for field in (None, 0):
        got = p.run(field=field, variant="wave", dfe=odd_(p.dfe), je=odd_(p.je), qs=[odd_(t) for t in p.qs],
                    c=[odd_(p.c[j]) for j in range(p.d)])
        want = clean if field is None else clean[:1]
        assert same_bits(torch_mod, got, want), (nq, field)
    assert float(clean.abs().max()) > 0
    generic = p.run(variant="generic")
    xs = [odd_(p.x[a]) for a in range(p.d)]
    for kw in (dict(x=xs), dict(out=[odd_(clean[a]).zero_() for a in range(p.d)]),
               dict(x=[p.x[0], xs[1]] + [p.x[a] for a in range(2, p.d)])):
        got = p.run(**kw)
        assert same_bits(torch_mod, torch_mod.stack(list(got)), generic), (nq, list(kw))
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(variant="wave", **kw)
        assert ei.value.rc == sf.capi.SF_EALIGN, (nq, list(kw))


def _affine_geometry(sf, torch_mod, nq, nelmt, dtype_name):
    """Parallelepipeds / parallelograms with a distinct Jacobian per element, their factors from both geometry calls and
    a seeded advecting velocity."""
    g = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 6, affine=True)
    assert len({tuple(np.round(a.reshape(-1), 12)) for a in g.A}) == nelmt          # distinct Jacobians
    d, nqt = g.d, int(np.prod(nq))
    c = rows(torch_mod, d, nelmt * nqt, g.dtype)
    for j in range(d):
        c[j].copy_(sf.fill_random(nelmt * nqt, 77 + j, dtype=g.dtype))
    host = lambda ts: [to_host(t) for t in ts]                                      # noqa: E731
    return g, g.run_affine(), c, host


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", END_TO_END, ids=ids(END_TO_END))
def test_end_to_end_against_the_deformed_path(sf, torch_mod, nq, nelmt, dtype_name):
    """sf_geom_affine_* -> sf_aff_advect_* against sf_geom_* -> sf_advect_* on the same coordinates and fields: each is
    within its bound of its own long-double reference on the factors it was given, and the two are held within the sum
    of the two bounds of each other."""
    g, aff, c, host = _affine_geometry(sf, torch_mod, nq, nelmt, dtype_name)
    d, nmt = g.d, int(np.prod([q - 1 for q in nq]))
    x = rows(torch_mod, d, nelmt * nmt, g.dtype)
    for a in range(d):
        x[a].copy_(sf.fill_random(nelmt * nmt, 88 + a, dtype=g.dtype))
    full = g.run(outputs=("df", "w"))
    hexa = d == 3
    got = (sf.affine_advect_hex if hexa else sf.affine_advect_quad)(nq, *g.bs, *g.ds, *g.qs, aff["dfe"], aff["je"], c, x)
    want = (sf.advect_hex if hexa else sf.advect_quad)(nq, *g.bs, *g.ds, full["df"], full["w"], c, x)
    B, D, Q = host(g.bs), host(g.ds), host(g.qs)
    cs, xs = [to_host(c[j]) for j in range(d)], [to_host(x[a]) for a in range(d)]
    _, abs_a = ref_affine_advect(nq, nelmt, B, D, Q, to_host(aff["dfe"]), to_host(aff["je"]), cs, xs)
    _, abs_d = ref_advect(nq, nelmt, B, D, to_host(full["df"]), to_host(full["w"]), cs, xs)
    u = unit_roundoff(dtype_name)
    tol = gamma(affine_advect_n(nq), u) * abs_a + gamma(advect_n(nq), u) * abs_d
    err = np.abs(to_host(got).astype(np.longdouble) - to_host(want).astype(np.longdouble))
    q = float(np.max(err / tol))
    print(f"end to end: affine advect vs deformed {nq} {dtype_name} nelmt={nelmt}: max |a - b| / (sum of the bounds) = {q:.3g}")
    assert np.all(err <= tol) and float(want.abs().max()) > 0


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", END_TO_END, ids=ids(END_TO_END))
def test_closed_form_on_the_elements_own_coordinates(sf, torch_mod, nq, nelmt, dtype_name):
    """The fields are the element's own coordinates: grad x_a = e_a, so out_a = B^T (w c_a) with w = je (qw2 (qw1 qw0)),
    which sf_iproduct_* computes from the plane formed on the device; held within the sum of the two bounds."""
    g, aff, c, host = _affine_geometry(sf, torch_mod, nq, nelmt, dtype_name)
    d, nqt = g.d, int(np.prod(nq))
    hexa = d == 3
    got = (sf.affine_advect_hex if hexa else sf.affine_advect_quad)(nq, *g.bs, *g.ds, *g.qs, aff["dfe"], aff["je"], c, g.xs)
    q = g.qs[0]
    for t in g.qs[1:]:
        q = t.reshape(-1, *([1] * q.dim())) * q.unsqueeze(0)
    w = (aff["je"].reshape(nelmt, 1) * q.reshape(1, nqt)).reshape(-1)
    B, D, Q = host(g.bs), host(g.ds), host(g.qs)
    cs, xs = [to_host(c[j]) for j in range(d)], [to_host(g.xs[a]) for a in range(d)]
    _, abs_a = ref_affine_advect(nq, nelmt, B, D, Q, to_host(aff["dfe"]), to_host(aff["je"]), cs, xs)
    u = unit_roundoff(dtype_name)
    worst = 0.0
    for a in range(d):
        r = (w * c[a]).contiguous()
        want = (sf.iproduct_hex if hexa else sf.iproduct_quad)(nq, *g.bs, r)
        _, abs_i = ref_iprod(nq, nelmt, B, to_host(r))
        tol = gamma(affine_advect_n(nq), u) * abs_a[a] + gamma(sum(nq), u) * abs_i
        err = np.abs(to_host(got[a]).astype(np.longdouble) - to_host(want).astype(np.longdouble))
        worst = max(worst, float(np.max(err / tol)))
        assert float(want.abs().max()) > 0
    print(f"closed form: affine advect {nq} {dtype_name} nelmt={nelmt}: max |out_a - B^T (w c_a)| / (sum of the bounds) = "
          f"{worst:.3g}")
    assert worst <= 1.0
