"""GPU tests of the weak advection term (include/sumfact.h sf_advect_*) against the long-double reference and its derived
bound (tests/advect_ref.py: elementwise |got - ref| <= gamma_N absref, N = 2 sum nq_d + max nq_d + 2 d + 1), on the seeded
per-value-distinct data of tests/advect_families.py.  No tolerance is introduced anywhere else: routes are compared bit
for bit, and the comparison with the chain sf_physderiv_* -> torch -> sf_iproduct_* uses the sum of the two bounds.
The SF_ENOTBUILT refusals, stream capture, the first call inside a capture and two streams in flight are the family's
cases of tests/test_gpu_multifield_common.py.
"""
import ctypes

import numpy as np
import pytest

from advect_families import (CHAIN, END_TO_END, FALLBACK, GUARD, MISALIGNED, POISON, RAGGED_BOUND, SCALAR, WAVE_COUNT, WAVE_ORDERS,
                             AdvectProblem)
from advect_ref import advect_excess, advect_n, ref_advect, unit_roundoff
from fused_families import F32, F64, RAGGED, Banded, case_id, sf, to_host, torch_mod  # noqa: F401
from geom_families import GeomProblem
from multifield_common import ids, odd, rows, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_within_the_bound(sf, torch_mod, nq, dtype_name):
    """nf = d through AUTO (the wave kernel: the rows are aligned) against long double at every value; in float64 "wave"
    and "generic" equal AUTO bit for bit."""
    p = AdvectProblem(sf, torch_mod, nq, WAVE_COUNT, dtype_name, 5)
    auto = p.run()
    if dtype_name == F64:
        assert same_bits(torch_mod, auto, p.run(variant="wave")), nq
        assert same_bits(torch_mod, auto, p.run(variant="generic")), nq
    p.check(auto, "auto")


@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_through_auto_on_ragged_counts(sf, torch_mod, nq):
    """AUTO on prefixes of one problem at the ragged counts equals "generic" bit for bit; the first 257 elements are held
    to the bound once."""
    p = AdvectProblem(sf, torch_mod, nq, max(RAGGED), F64, 3)
    for n in RAGGED:
        auto, generic = p.run(n), p.run(n, variant="generic")
        assert auto.shape == (p.d, n * p.nmt)
        assert same_bits(torch_mod, auto, generic), (nq, n)
        if n == RAGGED_BOUND:
            p.check(auto, f"ragged (first {n})", elements=np.arange(n))


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", SCALAR, ids=ids(SCALAR))
def test_scalar_transport_equals_the_vector_kernel(sf, torch_mod, nq, nelmt, dtype_name):
    """nf = 1 with in = in_a equals out_a of the nf = d call bit for bit, for every a: the lane -> element -> field map of
    both fronts."""
    p = AdvectProblem(sf, torch_mod, nq, nelmt, dtype_name, 9)
    vec = p.run()
    for a in range(p.d):
        one = p.run(field=a)
        assert one.shape == (1, nelmt * p.nmt)
        assert same_bits(torch_mod, one[0], vec[a]), (nq, a)
    assert float(vec.abs().max()) > 0


@pytest.mark.parametrize("nf", ["d", 1])
@pytest.mark.parametrize("nq,nelmt", FALLBACK, ids=ids(FALLBACK))
def test_fallback_shapes_within_the_bound(sf, torch_mod, nq, nelmt, nf):
    p = AdvectProblem(sf, torch_mod, nq, nelmt, F64, nelmt % 101)
    field = None if nf == "d" else p.d - 1
    auto, generic = p.run(field=field), p.run(field=field, variant="generic")
    assert same_bits(torch_mod, auto, generic)
    p.check(generic, "generic", fields=None if field is None else [field])


@pytest.mark.parametrize("nq,nelmt", CHAIN, ids=ids(CHAIN))
def test_against_the_chain_on_the_device(sf, torch_mod, nq, nelmt):
    """sf_physderiv_* per field, the dot product with c and the weight in torch, sf_iproduct_* per field.  The chain makes
    the operations that advect_n counts (physderiv_n + d for the dot product + 1 for the weight + sum nq_d for the
    projection = N) on the same absolute operator, so each result is within gamma_N absref of the truth and the two are
    within the sum of the two bounds of each other."""
    p = AdvectProblem(sf, torch_mod, nq, nelmt, F64, 21)
    fused = p.run()
    hexa = p.d == 3
    pd, ip = (sf.physderiv_hex, sf.iproduct_hex) if hexa else (sf.physderiv_quad, sf.iproduct_quad)
    chain = []
    for a in range(p.d):
        grad = pd(nq, *p.bs, *p.ds, p.df, p.x[a].contiguous())
        r = p.w * sum(p.c[j] * grad[j] for j in range(p.d))
        chain.append(ip(nq, *p.bs, r.contiguous()))
    _, absref = p.reference()
    q = advect_excess(np.stack([to_host(t) for t in chain]), to_host(fused), absref, nq, unit_roundoff(F64), factor=2.0)
    print(f"chain: advect {nq} nelmt={nelmt}: max |fused - chain| / (2 gamma_N absref) = {q:.3g}")
    assert q <= 1.0
    p.check(fused, "fused")


def _raw_call(sf, p, nf, df, w, cs, ins, outs, variant="auto"):
    """The C entry point with every in_a / out_a slot filled (those beyond nf too)."""
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    fn = getattr(sf.capi.lib(), f"sf_advect_{'hex' if p.d == 3 else 'quad'}_f64_variant")
    return fn(sf.VARIANTS[variant], *p.nq, p.nelmt, nf, *(ptr(t) for t in p.bs), *(ptr(t) for t in p.ds), ptr(df), ptr(w),
              *(ptr(t) for t in cs), *(ptr(t) for t in ins), *(ptr(t) for t in outs),
              ctypes.c_void_p(p.torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=ids(GUARD))
def test_guard_bands_and_nan_bands(sf, torch_mod, nq, nelmt):
    """Every out_a between guard words, every input between NaN bands: nothing is written outside the outputs, nothing
    read outside the inputs reaches a result.  With nf = 1 the slots out1.. of the C call are never written."""
    p = AdvectProblem(sf, torch_mod, nq, nelmt, F64, 17)
    clean = p.run()
    guard = -777.25
    band = lambda t: Banded.of(torch_mod, t)                                   # noqa: E731
    bs, ds = [band(t) for t in p.bs], [band(t) for t in p.ds]
    df, w = band(p.df), band(p.w)
    cs, xs = [band(p.c[j]) for j in range(p.d)], [band(p.x[a]) for a in range(p.d)]
    outs = [Banded(torch_mod, p.dtype, nelmt * p.nmt, 0, guard, lines=4) for _ in range(p.d)]
    got = p.run(bs=[b.view for b in bs], ds=[b.view for b in ds], df=df.view, w=w.view, c=[b.view for b in cs],
                x=[b.view for b in xs], out=[o.view for o in outs])
    torch_mod.cuda.synchronize()
    assert all(o.bands_intact(torch_mod) for o in outs)
    assert all(b.bands_intact(torch_mod) for b in bs + ds + [df, w] + cs + xs)
    for a in range(p.d):
        assert same_bits(torch_mod, got[a], clean[a]), (nq, a)
    assert not bool(torch_mod.isnan(clean).any()) and float(clean.abs().max()) > 0
    # nf = 1 through the C call with every slot filled: out1.. keep their guard words
    for o in outs:
        o.reset()
    rc = _raw_call(sf, p, 1, df.view, w.view, [b.view for b in cs], [b.view for b in xs], [o.view for o in outs])
    torch_mod.cuda.synchronize()
    assert rc == 0
    assert same_bits(torch_mod, outs[0].view, clean[0]) and outs[0].bands_intact(torch_mod)
    for o in outs[1:]:
        assert bool((o.buf == guard).all())


@pytest.mark.parametrize("nq,nelmt", POISON, ids=ids(POISON))
def test_poison_stays_in_its_element(sf, torch_mod, nq, nelmt):
    """NaN in one element's c: only that element's outputs are NaN, in every field.  NaN in one element's in_1: only that
    element's field 1.  Everything else keeps its bits."""
    p = AdvectProblem(sf, torch_mod, nq, nelmt, F64, 23)
    clean = p.run()
    assert not bool(torch_mod.isnan(clean).any())
    for victim in (0, nelmt // 2, nelmt - 1):
        c = p.c.clone(memory_format=torch_mod.contiguous_format)
        c.reshape(p.d, nelmt, p.nqt)[:, victim] = float("nan")
        got = p.run(c=c).reshape(p.d, nelmt, p.nmt)
        nan = torch_mod.isnan(got)
        assert bool(nan[:, victim].all()) and int(nan.sum()) == p.d * p.nmt, (nq, victim)
        keep = [e for e in range(nelmt) if e != victim]
        assert same_bits(torch_mod, got[:, keep], clean.reshape(p.d, nelmt, p.nmt)[:, keep])
        x = rows(torch_mod, p.d, nelmt * p.nmt, p.dtype)
        x.copy_(p.x)
        x[1].reshape(nelmt, p.nmt)[victim] = float("nan")
        got = p.run(x=x).reshape(p.d, nelmt, p.nmt)
        nan = torch_mod.isnan(got)
        assert bool(nan[1, victim].all()) and int(nan.sum()) == p.nmt, (nq, victim)
        assert same_bits(torch_mod, got[0], clean.reshape(p.d, nelmt, p.nmt)[0])
        assert same_bits(torch_mod, got[1][keep], clean.reshape(p.d, nelmt, p.nmt)[1][keep])


def test_refusals(sf, torch_mod):
    """nf = 2 in 3D, nf = 0, a NULL df and too few fields: SF_EINVAL."""
    c = sf.capi
    p = AdvectProblem(sf, torch_mod, (4, 4, 4), 5, F64, 2)
    outs = [torch_mod.zeros(5 * p.nmt, dtype=p.dtype, device="cuda") for _ in range(3)]
    cs, xs = [p.c[j] for j in range(3)], [p.x[a] for a in range(3)]
    assert _raw_call(sf, p, 2, p.df, p.w, cs, xs, outs) == c.SF_EINVAL
    assert _raw_call(sf, p, 0, p.df, p.w, cs, xs, outs) == c.SF_EINVAL
    assert _raw_call(sf, p, 3, None, p.w, cs, xs, outs) == c.SF_EINVAL
    assert _raw_call(sf, p, 3, p.df, p.w, cs, xs, outs) == c.SF_OK
    with pytest.raises(c.SumfactError) as ei:
        p.run(x=p.x[:2])
    assert ei.value.rc == c.SF_EINVAL


@pytest.mark.parametrize("nq,nelmt", MISALIGNED, ids=ids(MISALIGNED))
def test_misaligned_point_operands_take_the_wave_route(sf, torch_mod, nq, nelmt):
    """df, w and c_j at an odd scalar offset (8-byte aligned only) still take the wave route and give the same bits."""
    p = AdvectProblem(sf, torch_mod, nq, nelmt, F64, 29)
    clean = p.run(variant="wave")
    odd_ = lambda t: odd(torch_mod, t)                                         # noqa: E731
    for field in (None, 0):
        got = p.run(field=field, variant="wave", df=odd_(p.df), w=odd_(p.w), c=[odd_(p.c[j]) for j in range(p.d)])
        want = clean if field is None else clean[:1]
        assert same_bits(torch_mod, got, want), (nq, field)
    assert float(clean.abs().max()) > 0


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", END_TO_END, ids=ids(END_TO_END))
def test_end_to_end_with_the_geometric_factors(sf, torch_mod, nq, nelmt, dtype_name):
    """sf_geom_* on deformed elements, its df and w into sf_advect_* with the coordinates as the fields; the result against
    the long-double reference evaluated on those very device arrays."""
    g = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 6)
    geo = g.run(outputs=("df", "w"))
    d, nqt = g.d, int(np.prod(nq))
    c = rows(torch_mod, d, nelmt * nqt, g.dtype)
    for j in range(d):
        c[j].copy_(sf.fill_random(nelmt * nqt, 77 + j, dtype=g.dtype))
    fn = sf.advect_hex if d == 3 else sf.advect_quad
    got = fn(nq, *g.bs, *g.ds, geo["df"], geo["w"], c, g.xs)
    ref, absref = ref_advect(nq, nelmt, [to_host(t) for t in g.bs], [to_host(t) for t in g.ds], to_host(geo["df"]),
                             to_host(geo["w"]), [to_host(c[j]) for j in range(d)], [to_host(g.xs[a]) for a in range(d)])
    q = advect_excess(to_host(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"end to end: advect {nq} {dtype_name} nelmt={nelmt} N={advect_n(nq)}: max |err| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0 and float(np.max(np.abs(ref))) > 0
