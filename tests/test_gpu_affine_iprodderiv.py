"""GPU tests of the weak divergence on affine elements (include/sumfact.h sf_aff_iprodderiv_*) that are the family's
own: bit equality with sf_iprodderiv_* on expanded planes, je == NULL that never reads je or qw, every dfe component on
its own, scalar-aligned views of dfe / je / qw, the transpose identity with sf_aff_physderiv_* on the device, a 20 011
element batch, and the overlap and validation order of the C ABI case by case.  install() adds the family's cases of the
parametrised tests the fused families share (tests/fused_common.py); install_single() its cases of the tests of
tests/test_gpu_fused_common.py (tests/affine_deriv_families.py).

Reference and bound: tests/affine_deriv_ref.py.  Elementwise |gpu - ref| <= gamma_N absref against a long-double
reference, N = iprodderiv_n(nq) + d, u = 2^-53 (fp64) or 2^-24 (fp32).  Data: seeded, distinct per element and per value,
uniform in [-1, 1) -- the signs of qw, dfe and je included.
"""
import ctypes
import math

import numpy as np
import pytest

from affine_deriv_families import AFFINE_IPRODDERIV, AFFINE_PHYSDERIV, install_single
from affine_deriv_ref import (affine_iprodderiv_excess, affine_iprodderiv_n, affine_physderiv_n, ref_affine_iprodderiv,
                              ref_affine_physderiv)
from fused_common import install
from fused_families import F32, F64, Problem, case_id, own_problem, sf, sizes, to_host, torch_mod  # noqa: F401
from iprod_ref import U64, gamma, unit_roundoff

pytestmark = pytest.mark.gpu
FAM = AFFINE_IPRODDERIV
install(globals(), FAM)
install_single(globals(), FAM)

BIT_SHAPES = [(3, 3, 3), (6, 6, 6), (8, 8, 8), (5, 5), (16, 16), (6, 6, 12), (23, 5)]


def expand(torch_mod, p):
    """(df, w) of sf_iprodderiv_* on the device in the problem's precision: df[e][c][pt] = dfe[e][c] and w[e][k][j][i] =
    je[e] * (qw2[k] * (qw1[j] * qw0[i])), each product rounded once, in exactly this association."""
    dd, nqt = len(p.nq) ** 2, sizes(p.nq)[1]
    df = p.data["dfe"].view(-1, dd, 1).expand(-1, dd, nqt).contiguous().reshape(-1)
    q = p.consts["qs"][0]
    for qd in p.consts["qs"][1:]:
        q = (qd.view(-1, 1) * q.view(1, -1)).reshape(-1)              # qd[outer] * (q[inner])
    w = (p.data["je"].view(-1, 1) * q.view(1, -1)).reshape(-1).contiguous()
    return df, w


def deformed(sf, p, df, w, n, variant="auto"):
    d, nqt = len(p.nq), sizes(p.nq)[1]
    f = sf.iprodderiv_hex if d == 3 else sf.iprodderiv_quad
    ins = [p.data[f"in{a}"][:n * nqt] for a in range(d)]
    return f(p.nq, *p.consts["bs"], *p.consts["ds"], df[:n * d * d * nqt], None if w is None else w[:n * nqt], ins,
             variant=variant)


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq", BIT_SHAPES, ids=case_id)
def test_bits_of_the_deformed_call_on_expanded_planes(sf, torch_mod, nq, dtype_name):
    """On a route, sf_aff_iprodderiv_* is bit for bit sf_iprodderiv_* on df planes filled with the constants and w =
    je * (qw2 * (qw1 * qw0)) expanded in the working precision; without je, on the same df with w = NULL.  AUTO (the wave
    kernels on the table, the fallback off it) and, in fp64, the fallback by name, at 65 and 257 elements."""
    p = own_problem(FAM, sf, torch_mod, nq, 257, dtype_name, 17)
    df, w = expand(torch_mod, p)
    for n in (65, 257):
        for variant in ("auto",) + (("generic",) if dtype_name == F64 else ()):
            for present in FAM.modes:
                got = p.run(sf, n=n, present=present, variant=variant)[0]
                want = deformed(sf, p, df, w if present else None, n, variant)
                torch_mod.cuda.synchronize()
                assert np.array_equal(to_host(got), to_host(want)), (nq, dtype_name, n, variant, present)
                assert float(got.abs().max()) > 0
    p.check([got], "bits", present=())


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (3, 3), (6, 6, 12), (23, 5)], ids=case_id)
def test_no_je_never_reads_je_or_qw(sf, torch_mod, nq):
    """je=None with qw=None (null pointers) equals je=None with NaN-filled qw, bit for bit, in both precisions: neither
    je nor any qw_d is read or validated."""
    d = len(nq)
    for dtype_name in (F64, F32):
        p = own_problem(FAM, sf, torch_mod, nq, 301, dtype_name, 21)
        data = p.window(present=())
        assert data["je"] is None
        nulls = p.run(sf, data=data, consts=dict(p.consts, qs=[None] * d))[0]
        nans = p.run(sf, data=data, consts=dict(p.consts, qs=[torch_mod.full_like(q, float("nan")) for q in p.consts["qs"]]))[0]
        torch_mod.cuda.synchronize()
        assert not bool(torch_mod.isnan(nulls).any())
        assert torch_mod.equal(nulls, nans), (nq, dtype_name)
        p.check([nulls], "je=None", present=())
    p = own_problem(FAM, sf, torch_mod, nq, 5, F64, 21)                  # with je, a missing qw is refused
    with pytest.raises(TypeError):
        p.run(sf, consts=dict(p.consts, qs=[None] * d))


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (4, 9)], ids=case_id)
def test_each_dfe_component_alone(sf, torch_mod, nq):
    """One component of dfe non-zero: pins the order c = a d + b and that the sum runs over the ROW index a -- the result
    equals the call whose only non-zero input is in_a (a = c // d) with the full dfe column cleared likewise."""
    dim = len(nq)
    p = own_problem(FAM, sf, torch_mod, nq, 67, F64, 41)
    c_host = {k: [to_host(t) for t in v] for k, v in p.consts.items()}
    ins = [to_host(p.data[f"in{a}"]) for a in range(dim)]
    for c in range(dim * dim):
        dfe = torch_mod.zeros_like(p.data["dfe"]).view(p.nelmt, dim * dim)
        dfe[:, c] = p.data["dfe"].view(p.nelmt, dim * dim)[:, c]
        dfe = dfe.reshape(-1)
        got = p.run(sf, data=dict(p.window(), dfe=dfe))[0]
        torch_mod.cuda.synchronize()
        ref, absref = ref_affine_iprodderiv(nq, p.nelmt, c_host["bs"], c_host["ds"], c_host["qs"], to_host(dfe),
                                            to_host(p.data["je"]), ins)
        q = affine_iprodderiv_excess(to_host(got), ref, absref, nq, U64)
        print(f"component {c} {nq}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0 and float(got.abs().max()) > 0
        # only in_a, a = c // d, enters: the other inputs may be anything finite
        other = dict(p.window(), dfe=dfe, **{f"in{a}": torch_mod.ones_like(p.data[f"in{a}"]) for a in range(dim) if a != c // dim})
        again = p.run(sf, data=other)[0]
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(got, again), c


@pytest.mark.parametrize("nq", [(8, 8, 8), (3, 3, 3), (8, 8), (11, 11), (6, 6, 12)], ids=case_id)
def test_scalar_aligned_dfe_je_and_qw(sf, torch_mod, nq):
    """dfe, je and every qw_d at odd scalar offsets into NaN-filled buffers: the same route (WAVE on the table), the same
    bits as the aligned originals, in both precisions."""
    for dtype_name in (F64, F32):
        p = own_problem(FAM, sf, torch_mod, nq, 133, dtype_name, 4)
        base = p.run(sf)[0]

        def view(t, off):
            buf = torch_mod.full((t.numel() + 8,), float("nan"), dtype=p.dtype, device="cuda")
            buf[off:off + t.numel()] = t
            return buf[off:off + t.numel()]

        for off in (1, 3):
            data = dict(p.window(), dfe=view(p.data["dfe"], off), je=view(p.data["je"], off))
            consts = dict(p.consts, qs=[view(q, off) for q in p.consts["qs"]])
            assert data["dfe"].data_ptr() % 16 != 0
            got = p.run(sf, data=data, consts=consts)[0]
            torch_mod.cuda.synchronize()
            assert torch_mod.equal(got, base), (nq, dtype_name, off)
            if dtype_name == F64 and len(set(nq)) == 1:
                wave = p.run(sf, data=data, consts=consts, variant="wave")[0]
                torch_mod.cuda.synchronize()
                assert torch_mod.equal(wave, base)
        p.check([base], "aligned original")


def _dot(a, b):
    return math.fsum((np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).reshape(-1))


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), F64), ((3, 3, 3), F64), ((5, 5, 5), F32), ((12, 12), F64),
                                           ((6, 6, 12), F64), ((23, 5), F32)], ids=lambda v: case_id(v))
def test_transpose_identity(sf, torch_mod, nq, dtype_name):
    """<affine_iprodderiv(f; je = None), x> = <f, affine_physderiv(x)> on the device, within the sum of the two bounds:
    gamma_N(weak divergence) <|A|^T |f|, |x|> + gamma_N(gradient) <|f|, |A| |x|>, both brackets from the long-double
    reference on absolute values (u of the working precision; the dot products are exact sums of fp64 products)."""
    dim, nelmt = len(nq), 67
    p = own_problem(FAM, sf, torch_mod, nq, nelmt, dtype_name, 33)
    x = sf.fill_random(nelmt * sizes(nq)[0], 77, dtype=p.dtype)
    bs, ds, dfe = p.consts["bs"], p.consts["ds"], p.data["dfe"]
    ins = [p.data[f"in{a}"] for a in range(dim)]
    atf = p.run(sf, present=())[0]
    pd = sf.affine_physderiv_hex if dim == 3 else sf.affine_physderiv_quad
    ax = pd(nq, *bs, *ds, dfe, x)
    torch_mod.cuda.synchronize()
    hb, hd = [to_host(b) for b in bs], [to_host(d) for d in ds]
    _, absy = ref_affine_physderiv(nq, nelmt, hb, hd, to_host(dfe), to_host(x))
    _, abst = ref_affine_iprodderiv(nq, nelmt, hb, hd, None, to_host(dfe), None, [to_host(f) for f in ins])
    u = unit_roundoff(dtype_name)
    s1 = float(np.sum(abst * np.abs(to_host(x)).astype(np.longdouble)))
    s2 = float(np.sum(np.abs(np.stack([to_host(f) for f in ins])).astype(np.longdouble) * absy))
    bound = gamma(affine_iprodderiv_n(nq), u) * s1 + gamma(affine_physderiv_n(nq), u) * s2
    lhs, rhs = _dot(to_host(atf), to_host(x)), _dot(np.stack([to_host(f) for f in ins]), to_host(ax))
    print(f"transpose {nq} {dtype_name}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0


def test_batch_of_20011_hex8(sf, torch_mod):
    """20 011 elements at 3D nq = 8 (many workgroups, a ragged tail): 1 024 seeded elements and the ends against the
    long-double reference; a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 20011
    p = own_problem(FAM, sf, torch_mod, nq, nelmt, F64, 8)
    y = p.run(sf)
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(20240611)
    sample = np.unique(np.concatenate(([0, 1, nelmt - 2, nelmt - 1], rng.integers(0, nelmt, 1024))))
    p.check_elements(y, "20011 elements", torch_mod.tensor(sample, device="cuda"))
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y[0], again[0])


# ---- the C ABI: validation order and overlaps, case by case ------------------------------------------------------------
def _abi(sf, torch_mod, nq=(3, 3, 3), nelmt=50):
    """(call, tensors): call(**overrides) -> rc of sf_aff_iprodderiv_hex_f64_variant on device buffers; an override is
    a tensor, an int address or None, `variant`, `nq` and `nelmt` included."""
    nmt, nqt = sizes(nq)
    p = own_problem(FAM, sf, torch_mod, nq, nelmt, F64, 1)
    room = lambda v: torch_mod.cat([v, torch_mod.zeros(2, dtype=v.dtype, device=v.device)])[:v.numel()]   # noqa: E731
    t = {"basis0": p.consts["bs"][0], "basis1": p.consts["bs"][1], "basis2": p.consts["bs"][2],
         "deriv0": p.consts["ds"][0], "deriv1": p.consts["ds"][1], "deriv2": p.consts["ds"][2],
         "qw0": room(p.consts["qs"][0]), "qw1": room(p.consts["qs"][1]), "qw2": room(p.consts["qs"][2]),
         "dfe": room(p.data["dfe"]), "je": room(p.data["je"]), "in0": room(p.data["in0"]), "in1": room(p.data["in1"]),
         "in2": room(p.data["in2"]), "out": torch_mod.full((nelmt * nmt + 2,), 7.25, dtype=torch_mod.float64, device="cuda")}
    order = list(t)

    def ptr(v):
        if v is None:
            return None
        return ctypes.c_void_p(v if isinstance(v, int) else v.data_ptr())

    def call(variant=0, nq=nq, nelmt=nelmt, **over):
        vals = dict(t, **over)
        return sf.capi.lib().sf_aff_iprodderiv_hex_f64_variant(variant, *nq, nelmt, *[ptr(vals[k]) for k in order], None)

    return call, t


def test_validation_order(sf, torch_mod):
    """The order include/sumfact.h documents, each step against the next: range, empty batch, nulls, alignment, overlap,
    extents beyond the fallback, unsupported variant; je and every qw_d are looked at only when je is not null."""
    c = sf.capi
    call, t = _abi(sf, torch_mod)
    weights = ("qw0", "qw1", "qw2", "je")
    odd = lambda name: t[name].data_ptr() + 4                                   # noqa: E731  not 8-byte aligned
    assert call() == c.SF_OK
    assert call(nq=(3, 1, 3), nelmt=0, dfe=None) == c.SF_EINVAL                 # (1) before (2)
    assert call(variant=99, nelmt=0) == c.SF_EINVAL
    assert call(nelmt=0, dfe=None, out=None, basis0=None) == c.SF_OK            # (2) before (3)
    for name in t:                                                              # (3): required ...
        if name != "je":
            assert call(**{name: None}) == c.SF_EINVAL, name
    assert call(je=None) == c.SF_OK                                             # ... je may be null,
    assert call(je=None, qw0=None, qw1=None, qw2=None) == c.SF_OK               # and then no qw_d is looked at:
    assert call(je=None, qw0=odd("qw0"), qw1=odd("qw1"), qw2=odd("qw2")) == c.SF_OK
    assert call(dfe=None, in0=odd("in0")) == c.SF_EINVAL                        # (3) before (4)
    for name in t:                                                              # (4): scalar alignment of every pointer
        assert call(**{name: odd(name)}) == c.SF_EALIGN, name
    assert call(je=odd("je"), out=t["in0"]) == c.SF_EALIGN                      # (4) before (5)
    assert call(nq=(13, 3, 3), nelmt=1, out=t["in1"]) == c.SF_EINVAL            # (5) before (6)
    assert call(nq=(13, 3, 3), nelmt=1) == c.SF_ENOTBUILT                       # (6)
    assert call(variant=6) == c.SF_ENOTBUILT                                    # (7) mfma has no fused kernel
    assert call(variant=1, out=t["out"].data_ptr() + 8) == c.SF_EALIGN          # WAVE: out not 16-byte aligned
    over = {k: t[k].data_ptr() + 8 for k in weights + ("dfe", "in0", "in1", "in2")}
    assert call(variant=1, **over) == c.SF_OK                                   # everything else: scalar alignment
    torch_mod.cuda.synchronize()


def test_overlap_is_refused(sf, torch_mod):
    """out on an input, on dfe, on je: SF_EINVAL, nothing launched; out on an unused je (je == NULL is the call's own
    statement that it is unused) and out that ends where dfe begins are fine."""
    c = sf.capi
    nq, nelmt = (3, 3, 3), 50
    nmt, nqt = sizes(nq)
    n = nelmt * nmt                                                             # 400 scalars of out
    call, t = _abi(sf, torch_mod, nq, nelmt)
    big = sf.fill_random(5 * n, 5)
    keep = big.clone()
    dfe, je = big[n:n + nelmt * 9], big[3 * n:3 * n + nelmt]                    # 450 scalars, 50 scalars
    cases = {"out on in0": dict(out=t["in0"]), "out on in2": dict(out=t["in2"]), "out one scalar before in1 ends":
             dict(out=t["in1"].data_ptr() + 8 * (nelmt * nqt - 1)), "out on dfe": dict(out=dfe),
             "out over the head of dfe": dict(out=big[n - 8:]), "out on je": dict(out=je),
             "out over the last scalar of je": dict(out=big[3 * n + nelmt - 1:])}
    for what, over in cases.items():
        assert call(dfe=dfe, je=je, **over) == c.SF_EINVAL, what
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(big, keep) and bool((t["out"] == 7.25).all())
    assert call(dfe=dfe, je=None, out=big[3 * n:4 * n]) == c.SF_OK              # over the memory of a je the call does not take
    assert call(dfe=dfe, je=je, out=big[:n]) == c.SF_OK                         # ends exactly where dfe begins
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(big[n:3 * n], keep[n:3 * n]) and not torch_mod.equal(big[:n], keep[:n])
