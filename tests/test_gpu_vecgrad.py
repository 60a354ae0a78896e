"""GPU tests of the gradient, divergence and curl of a vector field (include/sumfact.h sf_vecgrad_*) against the
long-double reference and its derived bounds (tests/vecgrad_ref.py: elementwise |got - ref| <= gamma_N absref with
N_grad = sum nq_d + max nq_d + d, N_div = N_grad + d - 1, N_curl = N_grad + 1), on the seeded per-value-distinct data of
tests/vecgrad_families.py.  No tolerance is introduced anywhere else: routes, sf_physderiv_* and the sums and differences
of the returned planes are compared bit for bit.  The SF_ENOTBUILT refusals, stream capture, the first call inside a
capture and two streams in flight are the family's cases of tests/test_gpu_multifield_common.py.
"""
import ctypes

import numpy as np
import pytest

from fused_families import F32, F64, RAGGED, Banded, case_id, sf, to_host, torch_mod  # noqa: F401
from geom_families import GeomProblem
from multifield_common import ids, odd, planes, rows, same_bits
from vecgrad_families import (END_TO_END, FALLBACK, GUARD, MISALIGNED, PHYSDERIV, POISON, RAGGED_BOUND, SUBSET_SHAPES, SUBSETS,
                              WAVE_COUNT, WAVE_ORDERS, VecgradProblem, banded_outputs, host_outputs, per_element)
from vecgrad_ref import CURL_PAIRS, OUTPUTS, output_excess, ref_vecgrad, unit_roundoff, vecgrad_n

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_within_the_bounds(sf, torch_mod, nq, dtype_name):
    """All outputs through AUTO (the wave kernel: every stream is aligned) against long double at every value; in
    float64 "wave" and "generic" equal AUTO bit for bit."""
    p = VecgradProblem(sf, torch_mod, nq, WAVE_COUNT, dtype_name, 5)
    auto = p.run()
    assert tuple(auto) == OUTPUTS
    if dtype_name == F64:
        assert same_bits(torch_mod, auto, p.run(variant="wave")), nq
        assert same_bits(torch_mod, auto, p.run(variant="generic")), nq
    p.check(auto, "auto")


@pytest.mark.parametrize("nq", WAVE_ORDERS, ids=case_id)
def test_every_wave_order_through_auto_on_ragged_counts(sf, torch_mod, nq):
    """AUTO on prefixes of one problem at the ragged counts equals "generic" bit for bit; the first 257 elements are held
    to the bounds once."""
    p = VecgradProblem(sf, torch_mod, nq, max(RAGGED), F64, 3)
    per, _ = per_element(p.nq)
    for n in RAGGED:
        auto, generic = p.run(n), p.run(n, variant="generic")
        assert auto["grad"].shape == (n * per["grad"],) and auto["div"].shape == (n * per["div"],)
        assert same_bits(torch_mod, auto, generic), (nq, n)
        if n == RAGGED_BOUND:
            p.check(auto, f"ragged (first {n})", n=n, elements=np.arange(n))


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", PHYSDERIV, ids=ids(PHYSDERIV))
def test_grad_equals_physderiv_and_div_curl_equal_their_planes(sf, torch_mod, nq, nelmt, dtype_name):
    """Plane a d + j of grad equals output j of sf_physderiv_* on in_a bit for bit; div and curl equal the torch sums and
    differences of the returned grad planes, in the order of steps 4 and 5, bit for bit."""
    p = VecgradProblem(sf, torch_mod, nq, nelmt, dtype_name, 9)
    d = p.d
    got = p.run()
    grad = got["grad"].reshape(nelmt, d * d, p.nqt)
    for a in range(d):
        pd = p.physderiv(a)
        for j in range(d):
            assert same_bits(torch_mod, grad[:, a * d + j], pd[j].reshape(nelmt, p.nqt)), (nq, a, j)
    g = lambda a, j: grad[:, a * d + j].reshape(-1)                                 # noqa: E731
    div = torch_mod.empty_like(got["div"])
    torch_mod.add(g(0, 0), g(1, 1), out=div)
    if d == 3:
        torch_mod.add(div, g(2, 2), out=div)
    assert same_bits(torch_mod, got["div"], div), nq
    for n, ((q, r), (s, t)) in enumerate(CURL_PAIRS[d]):
        c = torch_mod.empty_like(div)
        torch_mod.sub(g(q, r), g(s, t), out=c)
        assert same_bits(torch_mod, planes(got["curl"])[n], c), (nq, n)
    assert float(got["grad"].abs().max()) > 0 and float(div.abs().max()) > 0


@pytest.mark.parametrize("names", SUBSETS, ids=["+".join(s) for s in SUBSETS])
@pytest.mark.parametrize("nq,nelmt", SUBSET_SHAPES, ids=ids(SUBSET_SHAPES))
def test_output_subsets(sf, torch_mod, nq, nelmt, names):
    """Every non-empty subset of the outputs: each output asked for sits between guard words and equals the full call bit
    for bit."""
    p = VecgradProblem(sf, torch_mod, nq, nelmt, F64, 13)
    full = p.run()
    out, bands = banded_outputs(torch_mod, p, names, nelmt, -777.25)
    got = p.run(outputs=names, out=out)
    torch_mod.cuda.synchronize()
    assert tuple(got) == names
    assert all(b.bands_intact(torch_mod) for b in bands)
    assert same_bits(torch_mod, got, {k: full[k] for k in names}), (nq, names)
    assert all(float(t.abs().max()) > 0 for k in names for t in planes(got[k]))


@pytest.mark.parametrize("nq,nelmt", FALLBACK, ids=ids(FALLBACK))
def test_fallback_shapes_within_the_bounds(sf, torch_mod, nq, nelmt):
    p = VecgradProblem(sf, torch_mod, nq, nelmt, F64, nelmt % 101)
    auto, generic = p.run(), p.run(variant="generic")
    assert same_bits(torch_mod, auto, generic)
    p.check(generic, "generic")


def _raw_call(sf, p, df, xs, grad, div, curl, variant="auto"):
    """The C entry point with every slot as given (None: NULL)."""
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    fn = getattr(sf.capi.lib(), f"sf_vecgrad_{'hex' if p.d == 3 else 'quad'}_f64_variant")
    return fn(sf.VARIANTS[variant], *p.nq, p.nelmt, *(ptr(t) for t in p.bs), *(ptr(t) for t in p.ds), ptr(df),
              *(ptr(t) for t in xs), ptr(grad), ptr(div), *(ptr(t) for t in curl),
              ctypes.c_void_p(p.torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=ids(GUARD))
def test_guard_bands_and_nan_bands(sf, torch_mod, nq, nelmt):
    """Every output between guard words, every input between NaN bands: nothing is written outside the outputs, nothing
    read outside the inputs reaches a result."""
    p = VecgradProblem(sf, torch_mod, nq, nelmt, F64, 17)
    clean = p.run()
    band = lambda t: Banded.of(torch_mod, t)                                   # noqa: E731
    bs, ds, df = [band(t) for t in p.bs], [band(t) for t in p.ds], band(p.df)
    xs = [band(p.x[a]) for a in range(p.d)]
    out, bands = banded_outputs(torch_mod, p, OUTPUTS, nelmt, -777.25)
    got = p.run(bs=[b.view for b in bs], ds=[b.view for b in ds], df=df.view, x=[b.view for b in xs], out=out)
    torch_mod.cuda.synchronize()
    assert all(b.bands_intact(torch_mod) for b in bands)
    assert all(b.bands_intact(torch_mod) for b in bs + ds + [df] + xs)
    assert same_bits(torch_mod, got, clean), nq
    for t in (t for v in clean.values() for t in planes(v)):
        assert not bool(torch_mod.isnan(t).any()) and float(t.abs().max()) > 0


@pytest.mark.parametrize("nq,nelmt", POISON, ids=ids(POISON))
def test_poison_stays_in_its_element(sf, torch_mod, nq, nelmt):
    """NaN in one element's in_1 reaches only that element: in grad only the planes of row 1 (c = d + j), in div the
    element, in curl the element's planes that take an entry of row 1 (3D: curl0 and curl2; curl1 = grad[0][2] -
    grad[2][0] keeps every bit).  Everything else keeps its bits."""
    p = VecgradProblem(sf, torch_mod, nq, nelmt, F64, 23)
    d = p.d
    clean = p.run()
    for victim in (0, nelmt // 2, nelmt - 1):
        x = rows(torch_mod, d, nelmt * p.nmt, p.dtype)
        x.copy_(p.x)
        x[1].reshape(nelmt, p.nmt)[victim] = float("nan")
        got = p.run(x=x)
        keep = [e for e in range(nelmt) if e != victim]
        grad, want = got["grad"].reshape(nelmt, d, d, p.nqt), clean["grad"].reshape(nelmt, d, d, p.nqt)
        nan = torch_mod.isnan(grad)
        assert bool(nan[victim, 1].all()) and int(nan.sum()) == d * p.nqt, (nq, victim)
        assert same_bits(torch_mod, grad[keep], want[keep])
        assert same_bits(torch_mod, grad[victim][[a for a in range(d) if a != 1]], want[victim][[a for a in range(d) if a != 1]])
        scalar = [("div", got["div"], clean["div"], True)]
        for n, pair in enumerate(CURL_PAIRS[d]):
            scalar.append((f"curl{n}", planes(got["curl"])[n], planes(clean["curl"])[n], any(a == 1 for a, _ in pair)))
        for name, t, w, hit in scalar:
            t, w = t.reshape(nelmt, p.nqt), w.reshape(nelmt, p.nqt)
            nan = torch_mod.isnan(t)
            if hit:
                assert bool(nan[victim].all()) and int(nan.sum()) == p.nqt, (nq, victim, name)
                assert same_bits(torch_mod, t[keep], w[keep]), (nq, victim, name)
            else:
                assert same_bits(torch_mod, t, w), (nq, victim, name)
    assert not any(bool(torch_mod.isnan(t).any()) for v in clean.values() for t in planes(v))


def test_refusals(sf, torch_mod):
    """The documented order through the C call on device arrays; with no curl asked for, and with a refused request for
    part of it, the curl arrays keep their guard words."""
    c = sf.capi
    p = VecgradProblem(sf, torch_mod, (4, 4, 4), 5, F64, 2)
    per, _ = per_element(p.nq)
    guard = -777.25
    new = lambda n: torch_mod.full((n,), guard, dtype=p.dtype, device="cuda")        # noqa: E731
    grad, div, curl = new(5 * per["grad"]), new(5 * per["div"]), [new(5 * per["curl"]) for _ in range(3)]
    xs, none = [p.x[a] for a in range(3)], [None] * 3
    assert _raw_call(sf, p, p.df, xs, None, None, none) == c.SF_EINVAL
    assert _raw_call(sf, p, None, xs, grad, div, curl) == c.SF_EINVAL
    assert _raw_call(sf, p, p.df, [xs[0], None, xs[2]], grad, div, curl) == c.SF_EINVAL
    for some in ([curl[0], None, None], [None, curl[1], curl[2]]):
        assert _raw_call(sf, p, p.df, xs, grad, div, some) == c.SF_EINVAL
    assert _raw_call(sf, p, p.df, xs, grad, grad[:5 * per["div"]], none) == c.SF_EINVAL          # div over grad
    assert _raw_call(sf, p, p.df, xs, p.df, None, none) == c.SF_EINVAL                          # grad over df
    assert _raw_call(sf, p, p.df, xs, grad, div, none, variant="mfma") == c.SF_ENOTBUILT
    torch_mod.cuda.synchronize()
    assert all(bool((t == guard).all()) for t in [grad, div] + curl)                            # nothing ran so far
    assert _raw_call(sf, p, p.df, xs, grad, div, none) == c.SF_OK
    torch_mod.cuda.synchronize()
    want = p.run(outputs=("grad", "div"))
    assert same_bits(torch_mod, grad, want["grad"]) and same_bits(torch_mod, div, want["div"])
    assert all(bool((t == guard).all()) for t in curl)
    with pytest.raises(c.SumfactError) as ei:
        p.run(outputs=())
    assert ei.value.rc == c.SF_EINVAL
    q = VecgradProblem(sf, torch_mod, (8, 8, 8), 3, F64, 2)                          # "wave" on a stream 8-byte aligned only
    off = torch_mod.empty(3 * per_element(q.nq)[0]["div"] + 3, dtype=q.dtype, device="cuda")[1:-2]
    assert off.data_ptr() % 16 == 8
    with pytest.raises(c.SumfactError) as ei:
        q.run(outputs=("div",), out={"div": off}, variant="wave")
    assert ei.value.rc == c.SF_EALIGN
    assert same_bits(torch_mod, q.run(outputs=("div",), out={"div": off})["div"], q.run(outputs=("div",), variant="generic")["div"])


@pytest.mark.parametrize("nq,nelmt", MISALIGNED, ids=ids(MISALIGNED))
def test_misaligned_df_takes_the_wave_route(sf, torch_mod, nq, nelmt):
    """df at an odd scalar offset (8-byte aligned only) still takes the wave route and gives the same bits."""
    p = VecgradProblem(sf, torch_mod, nq, nelmt, F64, 29)
    clean = p.run(variant="wave")
    assert same_bits(torch_mod, p.run(variant="wave", df=odd(torch_mod, p.df)), clean), nq
    assert float(clean["grad"].abs().max()) > 0


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", END_TO_END, ids=ids(END_TO_END))
def test_end_to_end_with_the_geometric_factors(sf, torch_mod, nq, nelmt, dtype_name):
    """sf_geom_* on deformed elements, its df into sf_vecgrad_* with seeded fields; the result against the long-double
    reference evaluated on those very device arrays, each output within its bound."""
    g = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 6)
    df = g.run(outputs=("df",))["df"]
    d, nmt = g.d, int(np.prod([q - 1 for q in nq]))
    x = rows(torch_mod, d, nelmt * nmt, g.dtype)
    for a in range(d):
        x[a].copy_(sf.fill_random(nelmt * nmt, 77 + a, dtype=g.dtype))
    fn = sf.vecgrad_hex if d == 3 else sf.vecgrad_quad
    got = fn(nq, *g.bs, *g.ds, df, x)
    ref, absref = ref_vecgrad(nq, nelmt, [to_host(t) for t in g.bs], [to_host(t) for t in g.ds], to_host(df),
                              [to_host(x[a]) for a in range(d)])
    for name, h in host_outputs(got, nelmt).items():
        q = output_excess(h, ref[name], absref[name], nq, unit_roundoff(dtype_name), name)
        print(f"end to end: vecgrad {nq} {dtype_name} nelmt={nelmt} {name} N={vecgrad_n(nq, name)}: "
              f"max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0 and float(np.max(np.abs(ref[name]))) > 0, name
