"""GPU tests of the geometric factors (include/sumfact.h sf_geom_*, sf_geom_affine_*) against the long-double reference and
its running bound (tests/geom_ref.py: elementwise |got - ref| <= 2 e, asserted by GeomRef.excess <= 1) on deformed
elements (tests/geom_families.py GeomProblem.prepare), never on raw random coordinates.

nq = 2.  An isoparametric element with one mode per direction has a Jacobian of rank <= 1 whatever its coefficients (with
the Legendre basis, whose only mode is the constant, J = 0 exactly): the reference's condition cannot hold and the
bound says nothing.  The nq = 2 shapes are kept for what they are there for, the lane -> element -> plane map of the rows
with many elements per wave: on the prescribed inputs detj = 0, w = 0, df = g = NaN and the routes agree bit for bit; on
random operands (test_nq2_lane_maps_on_random_operands) the wave kernel is compared bit for bit, NaN included, with the
fallback, which the other shapes hold to the bound -- the values are rounding residuals that differ from element to
element, so a wrong map shows.

The SF_ENOTBUILT refusals, stream capture, the first call inside a capture and two streams in flight are the family's cases
of tests/test_gpu_multifield_common.py.
"""
import itertools

import numpy as np
import pytest

from affine_ref import affine_n, ref_affine
from fused_families import F32, F64, RAGGED, Banded, case_id, sf, to_host, torch_mod  # noqa: F401
from geom_families import FALLBACK, SUBSETS, WAVE_2D, WAVE_3D, GeomProblem, per_element
from geom_ref import OUTPUTS, U64, gamma, sizes
from helm_ref import helm_n, ref_helmholtz
from multifield_common import bits, same_bits
from physderiv_ref import physderiv_n, ref_physderiv

pytestmark = pytest.mark.gpu
WAVE = WAVE_3D + WAVE_2D
ORDERS = [(n,) * 3 for n in range(2, 9)] + [(n,) * 2 for n in range(2, 17)]
ALL_SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(OUTPUTS, r)]


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq,nelmt", WAVE, ids=[case_id(s) + "-" + str(n) for s, n in WAVE])
def test_wave_orders_within_the_bound_and_equal_to_the_fallback(sf, torch_mod, nq, nelmt, dtype_name):
    """AUTO (the wave kernel: the buffers are aligned) within the bound at every value of every output; in float64 the
    explicit routes too, "wave" and "generic" bit for bit equal."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, nelmt % 101)
    auto = p.run()
    if dtype_name == F64:
        wave, generic = p.run(variant="wave"), p.run(variant="generic")
        assert same_bits(torch_mod, auto, wave) and same_bits(torch_mod, wave, generic), nq
    if nq[0] == 2:                                                  # singular by construction: see the module docstring
        assert bool((auto["detj"] == 0).all()) and bool((auto["w"] == 0).all())
        assert bool(torch_mod.isnan(auto["df"]).all()) and bool(torch_mod.isnan(auto["g"]).all())
        return
    p.check(auto, "auto")


@pytest.mark.parametrize("nq,nelmt", [((2, 2, 2), 33), ((2, 2, 2), 1001), ((2, 2), 259)], ids=["2x2x2-33", "2x2x2-1001", "2x2-259"])
def test_nq2_lane_maps_on_random_operands(sf, torch_mod, nq, nelmt):
    """nq = 2 with seeded random bases, derivative matrices and coordinates, so that the (meaningless) values differ from
    point to point and from element to element: the wave rows with the most elements per wave, bit for bit against the
    fallback."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 31)
    rnd = lambda n, seed: sf.fill_random(n, seed, dtype=p.dtype)      # noqa: E731
    p.bs, p.ds, p.qs = ([rnd(n, seed + a) for a in range(p.d)] for n, seed in ((2, 500), (4, 600), (2, 700)))
    xs = [rnd(nelmt, 90 + a) for a in range(p.d)]                   # one mode per element and coordinate
    wave, generic = p.run(xs=xs, variant="wave"), p.run(xs=xs, variant="generic")
    assert same_bits(torch_mod, wave, generic)
    det = to_host(wave["detj"])
    assert not np.any(np.isnan(det)) and len(set(det.tolist())) > 8           # rounding residuals, not one constant


@pytest.mark.parametrize("nq,nelmt", FALLBACK, ids=[case_id(s) + "-" + str(n) for s, n in FALLBACK])
def test_fallback_shapes_within_the_bound(sf, torch_mod, nq, nelmt):
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, nelmt % 101)
    auto, generic = p.run(), p.run(variant="generic")
    assert same_bits(torch_mod, auto, generic)
    p.check(generic, "generic")


@pytest.mark.parametrize("nq", ORDERS, ids=case_id)
def test_every_wave_order_through_auto_on_ragged_counts(sf, torch_mod, nq):
    """Every order of the table at the ragged element counts: AUTO on a prefix of the problem equals "generic" on it bit
    for bit; the first 257 elements are held to the bound once."""
    p = GeomProblem(sf, torch_mod, nq, max(RAGGED), F64, 3)
    nmt = sizes(nq)[0]
    for n in RAGGED:
        xs = p.xs[:, :n * nmt]
        auto, generic = p.run(xs=xs), p.run(xs=xs, variant="generic")
        assert all(t.numel() == n * per_element(nq)[k] for k, t in auto.items())
        assert same_bits(torch_mod, auto, generic), (nq, n)
        if n == 257 and nq[0] > 2:
            p.prefix(n).check(auto, "ragged")


@pytest.mark.parametrize("dtype_name,variant", [(F64, "auto"), (F64, "generic"), (F32, "auto")])
@pytest.mark.parametrize("nq,nelmt", SUBSETS, ids=[case_id(s) + "-" + str(n) for s, n in SUBSETS])
def test_every_subset_of_the_outputs_between_guard_words(sf, torch_mod, nq, nelmt, dtype_name, variant):
    """Every non-empty subset of (df, w, g, detj): the planes asked for are bit for bit those of the all-outputs call,
    the guard words around every output and the NaN bands around every input are intact, and the buffers of the outputs
    that were passed as NULL are untouched from end to end."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 5)
    per, guard = per_element(nq), -77.0
    rows = [Banded.of(torch_mod, p.xs[a]) for a in range(p.d)]
    consts = {k: [Banded.of(torch_mod, t) for t in getattr(p, k)] for k in ("bs", "ds", "qs")}
    p.bs, p.ds, p.qs = ([b.view for b in consts[k]] for k in ("bs", "ds", "qs"))
    xs = [r.view for r in rows]
    outs = {k: Banded(torch_mod, p.dtype, nelmt * per[k], 0, guard, lines=4) for k in OUTPUTS}
    full = p.run(xs=xs, variant=variant)
    for subset in ALL_SUBSETS:
        for b in outs.values():
            b.reset()
        got = p.run(subset, out={k: outs[k].view for k in subset}, xs=xs, variant=variant)
        torch_mod.cuda.synchronize()
        assert set(got) == set(subset)
        for k in OUTPUTS:
            if k in subset:
                assert torch_mod.equal(bits(torch_mod, got[k]), bits(torch_mod, full[k])), (subset, k)
                assert outs[k].bands_intact(torch_mod), (subset, k)
            else:
                assert bool((outs[k].buf == guard).all()), (subset, k)
        assert all(r.bands_intact(torch_mod) for r in rows) and all(b.bands_intact(torch_mod) for v in consts.values() for b in v)
    fn = sf.geom_hex if p.d == 3 else sf.geom_quad                  # the weights may be None when neither w nor g is asked
    got = fn(nq, *p.bs, *p.ds, *([None] * p.d), xs, outputs=("df", "detj"), variant=variant)
    assert torch_mod.equal(bits(torch_mod, got["df"]), bits(torch_mod, full["df"]))
    assert torch_mod.equal(bits(torch_mod, got["detj"]), bits(torch_mod, full["detj"]))
    p.check(full, "subsets", elements=[0, 1, nelmt // 2, nelmt - 1])


@pytest.mark.parametrize("nq,nelmt", [((5, 5, 5), 67), ((5, 5), 259), ((6, 6, 12), 13)], ids=["5x5x5", "5x5", "6x6x12"])
def test_inverted_elements_have_negative_detj_and_positive_w(sf, torch_mod, nq, nelmt):
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 9)
    xs = p.xs.clone()
    xs[1] = -xs[1]                                                  # a reflection: every element inverted
    got = p.run(xs=xs)
    assert bool((got["detj"] < 0).all()) and bool((got["w"] > 0).all())
    p.check(got, "inverted", ref=p.reference(xs=xs))


@pytest.mark.parametrize("variant", ["auto", "generic"])
@pytest.mark.parametrize("nq,nelmt", [((3, 3, 3), 1001), ((5, 5), 4099), ((8, 8, 8), 65)], ids=["3x3x3", "5x5", "8x8x8"])
def test_a_nan_coordinate_stays_in_its_element(sf, torch_mod, nq, nelmt, variant):
    """One mode of one coordinate of one element is NaN: every plane of that element is NaN, every other element is bit
    for bit what it is without it (chunks of 14, 8 and 1 elements)."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 13)
    clean = p.run(variant=variant)
    bad_e, nmt = nelmt // 2 + 1, sizes(nq)[0]
    xs = p.xs.clone()
    xs[1, bad_e * nmt + 1] = float("nan")
    got = p.run(xs=xs, variant=variant)
    for k in OUTPUTS:
        a, b = got[k].view(nelmt, -1), clean[k].view(nelmt, -1)
        assert bool(torch_mod.isnan(a[bad_e]).all()), k
        keep = torch_mod.arange(nelmt, device="cuda") != bad_e
        assert torch_mod.equal(a[keep], b[keep]), k


AFFINE_CASES = [((5, 5, 5), 67, F64), ((5, 5, 5), 67, F32), ((8, 8, 8), 65, F64), ((16, 16), 127, F64), ((5, 5), 259, F32),
                ((6, 6, 12), 13, F64), ((23, 5), 14, F64)]


@pytest.mark.parametrize("nq,nelmt,dtype_name", AFFINE_CASES, ids=[f"{case_id(s)}-{n}-{t}" for s, n, t in AFFINE_CASES])
def test_affine_form_is_point_zero_of_the_deformed_call(sf, torch_mod, nq, nelmt, dtype_name):
    """On the same (deformed) coordinates dfe and je are bit for bit df[e][c][0][0][0] and |detj[e][0][0][0]| of
    sf_geom_*; ge is within its bound, and so are dfe and je."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 17)
    full, aff = p.run(), p.run_affine()
    d, nqt = p.d, sizes(nq)[1]
    assert torch_mod.equal(aff["dfe"], full["df"].view(nelmt, d * d, nqt)[:, :, 0].reshape(-1))
    assert torch_mod.equal(aff["je"], full["detj"].view(nelmt, nqt)[:, 0].abs())
    p.check(aff, "affine", affine=True)


@pytest.mark.parametrize("nq,nelmt", [((5, 5, 5), 35), ((8, 8, 8), 17), ((9, 9), 131)], ids=["5x5x5", "8x8x8", "9x9"])
def test_end_to_end_gradient_of_a_linear_function(sf, torch_mod, nq, nelmt):
    """in = sum_a c_a x_a is c . x: sf_physderiv_* with the df of sf_geom_* returns c at every point of deformed elements.
    Tolerance: the gradient's bound gamma_N absref against its long-double reference on the same df, plus what the
    error of df (at most 2 e(df)) moves that reference, sum_b 2 e(df_ab) |du_b|, plus the rounding of `in` itself
    (one product and one sum per term: 8 u absref covers it)."""
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 21)
    d, nqt = p.d, sizes(nq)[1]
    c = [0.7, -1.3, 0.4][:d]
    inp = sum(ca * p.xs[a] for a, ca in enumerate(c)).contiguous()
    df = p.run(("df",))["df"]
    fn = sf.physderiv_hex if d == 3 else sf.physderiv_quad
    got = fn(nq, *p.bs, *p.ds, df, inp)
    B, D, _ = p.host_operands()
    _, absref = ref_physderiv(nq, nelmt, B, D, to_host(df), to_host(inp))
    du, _ = ref_physderiv(nq, nelmt, B, D, None, to_host(inp))
    edf = p.reference().err["df"].reshape(nelmt, d * d, nqt)
    dur = np.abs(du).reshape(d, nelmt, nqt)
    for a in range(d):
        tol = ((gamma(physderiv_n(nq), U64) + 8 * U64) * absref[a].reshape(nelmt, nqt)
               + sum(2 * edf[:, a * d + b] * dur[b] for b in range(d)))
        err = np.abs(to_host(got[a]).reshape(nelmt, nqt).astype(np.longdouble) - c[a])
        print(f"gradient of c.x {nq} a={a}: max err {float(np.max(err)):.3g}, max err / tol {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol), (a, float(np.max(err / tol)))


@pytest.mark.parametrize("nq,nelmt", [((5, 5, 5), 35), ((9, 9), 131), ((6, 6, 12), 9)], ids=["5x5x5", "9x9", "6x6x12"])
def test_end_to_end_helmholtz_on_affine_coordinates(sf, torch_mod, nq, nelmt):
    """On affine elements sf_helmholtz_* with (g, w) of sf_geom_* agrees with sf_affine_helmholtz_* with (ge, je) of
    sf_geom_affine_*.  Tolerance: the two operators' bounds against their long-double references (gamma_N absref each)
    plus what the errors of the metrics (at most 2 e each) move those references: both operators are linear in their
    metric, so that is the operator on |B|, |D|, |x| with 2 e in the place of the metric."""
    lam = 0.75
    p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 23, affine=True)
    x = sf.fill_random(nelmt * sizes(nq)[0], 77, dtype=p.dtype)
    full, aff = p.run(("g", "w")), p.run_affine()
    hex_ = p.d == 3
    a = (sf.helmholtz_hex if hex_ else sf.helmholtz_quad)(nq, *p.bs, *p.ds, full["g"], full["w"], lam, x)
    b = (sf.affine_helmholtz_hex if hex_ else sf.affine_helmholtz_quad)(nq, *p.bs, *p.ds, *p.qs, aff["ge"], aff["je"], lam, x)
    B, D, Q = p.host_operands()
    xh = to_host(x)
    _, abs_h = ref_helmholtz(nq, nelmt, B, D, to_host(full["g"]), to_host(full["w"]), lam, xh)
    _, abs_a = ref_affine(nq, nelmt, B, D, Q, to_host(aff["ge"]), to_host(aff["je"]), lam, xh)
    rf, ra = p.reference(), p.reference(affine=True)
    ab = lambda v: [np.abs(t) for t in v]      # noqa: E731
    moved_h, _ = ref_helmholtz(nq, nelmt, ab(B), ab(D), 2 * rf.err["g"], 2 * rf.err["w"], lam, np.abs(xh))
    moved_a, _ = ref_affine(nq, nelmt, ab(B), ab(D), ab(Q), 2 * ra.err["ge"], 2 * ra.err["je"], lam, np.abs(xh))
    tol = (gamma(helm_n(nq), U64) * np.asarray(abs_h).reshape(-1) + gamma(affine_n(nq), U64) * np.asarray(abs_a).reshape(-1)
           + np.asarray(moved_h).reshape(-1) + np.asarray(moved_a).reshape(-1))
    err = np.abs(to_host(a).astype(np.longdouble) - to_host(b).astype(np.longdouble))
    print(f"helmholtz vs affine {nq}: max err {float(np.max(err)):.3g}, max err / tol {float(np.max(err / tol)):.3g}")
    assert np.all(err <= tol) and float(a.abs().max()) > 0

