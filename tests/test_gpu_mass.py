"""GPU tests of the fused mass operator (include/sumfact.h sf_mass_*), y_e = B^T diag(w_e) B x_e in one kernel, that are
the family's own: scalar-aligned views, composition with the two existing operators, symmetry and positivity, the full
1 048 576-element batch and refused overlaps.  install() adds the family's cases of the parametrised tests the fused
families share (tests/fused_common.py: every wave order through AUTO, ragged counts, the fallback, explicit variants,
guard bands); refusals, stream capture and two streams in flight are tests/test_gpu_fused_common.py.

Reference and bounds: tests/mass_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double reference,
gamma_N = N u / (1 - N u), N = 2 (nq0 + nq1 [+ nq2]) + 1, u = 2^-53 (fp64) or 2^-24 (fp32); where long double would be
too slow, 2 gamma_N (1 + gamma_N) * absref64 against fp64 CPU sweeps.

That lanes without a point of the batch issue no weight load at all is a property of the code (load_weights() in
csrc/mass_wave.h: the loads sit inside `t < NP && e < evalid`) and of the ISA (the loads are under an exec mask); no test
can show it without provoking a fault, and none tries.
"""
import math

import pytest

from fused_common import install
from fused_families import BY_NAME, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from mass_ref import U64, gamma, mass_excess, mass_f64, mass_n, ref_mass, symmetry_bound, unit_roundoff

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["mass"])


def _bases(sf, torch_mod, nq, dtype_name, seed):
    dtype = getattr(torch_mod, dtype_name)
    return [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]


def _weights(sf, torch_mod, n, seed, dtype_name):
    return 0.25 + sf.fill_random(n, 7000 + seed, dtype=getattr(torch_mod, dtype_name)).abs()


def _mass(sf, nq, bs, w, x, **kw):
    return (sf.mass_hex if len(nq) == 3 else sf.mass_quad)(tuple(nq), *bs, w, x, **kw)


def _check(nq, nelmt, bs, w, x, got, dtype_name, what):
    ref, absref = ref_mass(nq, nelmt, [to_host(b) for b in bs], to_host(w), to_host(x))
    q = mass_excess(to_host(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"{what}: {nq} {dtype_name} nelmt={nelmt}: max |err| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0, (what, nq, dtype_name, nelmt, q)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """8-byte-aligned (fp32: 4-byte-aligned) views of in, out and w.  AUTO is correct through the fallback when in or out
    lacks 16-byte alignment, and through the wave kernel when only w does; guards on both sides of out are untouched;
    variant "wave" refuses in / out with SF_EALIGN."""
    nelmt = 333
    nmt, nqt = sizes(nq)
    cases = (("float64", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 1))), ("float32", ((2, 0, 0), (0, 2, 0), (0, 0, 1), (1, 3, 3))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 4)
        for off_in, off_out, off_w in offsets:
            xbuf = sf.fill_random(nelmt * nmt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nmt]
            wbuf = _weights(sf, torch_mod, nelmt * nqt + 8, off_w, dtype_name)
            w = wbuf[off_w:off_w + nelmt * nqt]
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            _mass(sf, nq, bs, w, x, out=o)
            torch_mod.cuda.synchronize()
            _check(nq, nelmt, bs, w, x, o, dtype_name, f"view {off_in}/{off_out}/{off_w}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                if off_in or off_out:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        _mass(sf, nq, bs, w, x, out=o, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                else:
                    # w needs only scalar alignment on the wave route
                    wave = _mass(sf, nq, bs, w, x, variant="wave")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(wave, o)


COMPOSE = [((8, 8, 8), 1003, "float64"), ((5, 5, 5), 1003, "float64"), ((11, 11, 11), 257, "float64"),
           ((12, 12), 1003, "float64"), ((7, 7), 1003, "float64"), ((6, 6, 12), 300, "float64"), ((23, 5), 300, "float64"),
           ((8, 8, 8), 1003, "float32"), ((16, 16), 1003, "float32")]


@pytest.mark.parametrize("nq,nelmt,dtype_name", COMPOSE, ids=[case_id(s) + "-" + d for s, _, d in COMPOSE])
def test_composition_with_bwdtrans_and_iproduct(sf, torch_mod, nq, nelmt, dtype_name):
    """The fused result against the three-launch chain iproduct(w * bwdtrans(x)) on the GPU, within
    2 gamma_N (1 + gamma_N) * absref, absref from the fused operator on absolute values.  The two orders of summation
    differ, so bit identity is not expected."""
    nmt, nqt = sizes(nq)
    bs = _bases(sf, torch_mod, nq, dtype_name, 6)
    x = sf.fill_random(nelmt * nmt, 61, dtype=getattr(torch_mod, dtype_name))
    w = _weights(sf, torch_mod, nelmt * nqt, 62, dtype_name)
    bwd, ipr = (sf.bwdtrans_hex, sf.iproduct_hex) if len(nq) == 3 else (sf.bwdtrans_quad, sf.iproduct_quad)
    fused = _mass(sf, nq, bs, w, x)
    chain = ipr(tuple(nq), *bs, w * bwd(tuple(nq), *bs, x))
    absref = _mass(sf, nq, [b.abs() for b in bs], w, x.abs())
    torch_mod.cuda.synchronize()
    u = unit_roundoff(dtype_name)
    g = gamma(mass_n(nq), u)
    q = mass_excess(to_host(fused), to_host(chain), to_host(absref), nq, u, factor=2 * (1 + g))
    print(f"composition {nq} {dtype_name}: max |fused - chain| / (2 gamma_N (1 + gamma_N) absref) = {q:.3g}")
    assert q <= 1.0
    assert float(absref.min()) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12)], ids=case_id)
def test_symmetry_and_positivity(sf, torch_mod, nq):
    """|<M x, y> - <x, M y>| <= 2 (gamma_N + gamma_m) sum_e <|M||x|, |y|>_e, m = nm^d, |M| the fused operator on absolute
    values, the sums with math.fsum per element; and <M x, x> > 0 for w > 0."""
    nelmt = 1003
    nmt, nqt = sizes(nq)
    bs = _bases(sf, torch_mod, nq, "float64", 12)
    x = sf.fill_random(nelmt * nmt, 121)
    y = sf.fill_random(nelmt * nmt, 122)
    w = _weights(sf, torch_mod, nelmt * nqt, 123, "float64")
    mx = _mass(sf, nq, bs, w, x)
    my = _mass(sf, nq, bs, w, y)
    mabs = _mass(sf, nq, [b.abs() for b in bs], w, x.abs())
    torch_mod.cuda.synchronize()

    def dots(a, b):
        a, b = to_host(a).reshape(nelmt, -1), to_host(b).reshape(nelmt, -1)
        return [math.fsum(a[e] * b[e]) for e in range(nelmt)]

    lhs, rhs = math.fsum(dots(mx, y)), math.fsum(dots(x, my))
    scale = math.fsum(dots(mabs, y.abs()))
    bound = symmetry_bound(nq, U64) * scale
    print(f"symmetry {nq}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    energy = dots(mx, x)
    assert min(energy) > 0 and math.fsum(energy) > 0


def test_full_batch_hex8(sf, torch_mod):
    """1 048 576 elements at 3D nq = 8: elementwise against fp64 CPU sweeps in slices (bound 2 gamma_N (1 + gamma_N)
    absref64); a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 1 << 20
    nmt, nqt = 343, 512
    bs = _bases(sf, torch_mod, nq, "float64", 8)
    bh = [to_host(b) for b in bs]
    x = sf.fill_random(nelmt * nmt, 1234)
    w = _weights(sf, torch_mod, nelmt * nqt, 1235, "float64")
    y = sf.mass_hex(nq, *bs, w, x)
    torch_mod.cuda.synchronize()
    g = gamma(mass_n(nq), U64)
    step, worst = 1 << 15, 0.0
    for lo in range(0, nelmt, step):
        out64, abs64 = mass_f64(nq, step, bh, to_host(w[lo * nqt:(lo + step) * nqt]), to_host(x[lo * nmt:(lo + step) * nmt]))
        worst = max(worst, mass_excess(to_host(y[lo * nmt:(lo + step) * nmt]), out64, abs64, nq, U64, factor=2 * (1 + g)))
    print(f"full batch: max |err| / (2 gamma_N (1 + gamma_N) absref64) = {worst:.3g}")
    assert worst <= 1.0
    again = sf.mass_hex(nq, *bs, w, x)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


def test_overlap_is_refused(sf, torch_mod):
    """out == in and out inside w: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    bs = _bases(sf, torch_mod, nq, "float64", 1)
    x = sf.fill_random(nelmt * 343, 1)
    w = _weights(sf, torch_mod, nelmt * 512, 1, "float64")
    keep = x.clone()
    for o in (x, w[:nelmt * 343]):
        with pytest.raises(sf.capi.SumfactError) as ei:
            sf.mass_hex(nq, *bs, w, x, out=o)
        assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(x, keep)
