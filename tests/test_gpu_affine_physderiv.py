"""GPU tests of the gradient on affine elements (include/sumfact.h sf_aff_physderiv_*) that are the family's own: bit
equality with sf_physderiv_* on planes filled with the constants, every dfe component on its own, scalar-aligned views of
dfe, the analytic gradient of a polynomial on affine elements, the backward pass of affine_physderiv_autograd, a 20 011
element batch, and the overlap and validation order of the C ABI case by case.  install() adds the family's cases of the
parametrised tests the fused families share (tests/fused_common.py); install_single() its cases of the tests of
tests/test_gpu_fused_common.py (tests/affine_deriv_families.py).

Reference and bound: tests/affine_deriv_ref.py.  Elementwise |gpu - ref| <= gamma_N absref against a long-double
reference, N = physderiv_n(nq), u = 2^-53 (fp64) or 2^-24 (fp32).  Data: seeded, distinct per element and per value,
uniform in [-1, 1).
"""
import ctypes
import math

import numpy as np
import pytest

from affine_deriv_families import AFFINE_IPRODDERIV, AFFINE_PHYSDERIV, install_single
from affine_deriv_ref import affine_iprodderiv_n, affine_physderiv_excess, affine_physderiv_n, ref_affine_physderiv
from fused_common import install
from fused_families import F32, F64, Problem, case_id, own_problem, sf, sizes, to_host, torch_mod  # noqa: F401
from iprod_ref import U64, gamma
from physderiv_ref import analytic_case

pytestmark = pytest.mark.gpu
FAM = AFFINE_PHYSDERIV
install(globals(), FAM)
install_single(globals(), FAM)

BIT_SHAPES = [(3, 3, 3), (6, 6, 6), (8, 8, 8), (5, 5), (16, 16), (6, 6, 12), (23, 5)]


def expand_df(p, dfe=None):
    """The planes df[e][c][k][j][i] = dfe[e][c] on the device, in the problem's precision."""
    dd, nqt = len(p.nq) ** 2, sizes(p.nq)[1]
    dfe = p.data["dfe"] if dfe is None else dfe
    return dfe.view(-1, dd, 1).expand(-1, dd, nqt).contiguous().reshape(-1)


def deformed(sf, p, df, n, variant="auto"):
    f = sf.physderiv_hex if len(p.nq) == 3 else sf.physderiv_quad
    return f(p.nq, *p.consts["bs"], *p.consts["ds"], df[:n * len(p.nq) ** 2 * sizes(p.nq)[1]],
             p.data["in"][:n * sizes(p.nq)[0]], variant=variant)


@pytest.mark.parametrize("dtype_name", [F64, F32])
@pytest.mark.parametrize("nq", BIT_SHAPES, ids=case_id)
def test_bits_of_the_deformed_call_on_expanded_planes(sf, torch_mod, nq, dtype_name):
    """On a route, sf_aff_physderiv_* is bit for bit sf_physderiv_* on planes filled with the constants: AUTO (the wave
    kernels on the table, the fallback off it) and, in fp64, the fallback by name, at 65 and 257 elements."""
    p = Problem(FAM, sf, torch_mod, nq, 257, dtype_name, 17)
    df = expand_df(p)
    for n in (65, 257):
        for variant in ("auto",) + (("generic",) if dtype_name == F64 else ()):
            got = p.run(sf, n=n, variant=variant)
            want = deformed(sf, p, df, n, variant)
            torch_mod.cuda.synchronize()
            for a in range(len(nq)):
                assert np.array_equal(to_host(got[a]), to_host(want[a])), (nq, dtype_name, n, variant, a)
            assert float(got[0].abs().max()) > 0
    p.check(got, "bits")


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (7, 7), (4, 9)], ids=case_id)
def test_each_dfe_component_alone(sf, torch_mod, nq):
    """One component of dfe non-zero, the others zero: pins the order c = a d + b (a transposed or permuted index would
    put the result into another output, or take another derivative)."""
    dim = len(nq)
    p = Problem(FAM, sf, torch_mod, nq, 131, F64, 41)
    c_host = {k: [to_host(t) for t in v] for k, v in p.consts.items()}
    for c in range(dim * dim):
        dfe = torch_mod.zeros_like(p.data["dfe"]).view(p.nelmt, dim * dim)
        dfe[:, c] = p.data["dfe"].view(p.nelmt, dim * dim)[:, c]
        dfe = dfe.reshape(-1)
        got = p.run(sf, data=dict(p.window(), dfe=dfe))
        torch_mod.cuda.synchronize()
        ref, absref = ref_affine_physderiv(nq, p.nelmt, c_host["bs"], c_host["ds"], to_host(dfe), to_host(p.data["in"]))
        q = affine_physderiv_excess(np.stack([to_host(g) for g in got]), ref, absref, nq, U64)
        print(f"component {c} {nq}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0
        for a in range(dim):
            assert (float(got[a].abs().max()) > 0) == (a == c // dim), (c, a)


@pytest.mark.parametrize("nq", [(8, 8, 8), (3, 3, 3), (8, 8), (11, 11), (6, 6, 12)], ids=case_id)
def test_scalar_aligned_dfe(sf, torch_mod, nq):
    """dfe at odd scalar offsets into a NaN-filled buffer: the same route (WAVE on the table), the same bits as the
    16-byte-aligned original, in both precisions."""
    for dtype_name in (F64, F32):
        p = Problem(FAM, sf, torch_mod, nq, 133, dtype_name, 4)
        base = p.run(sf)
        for off in (1, 3):
            buf = torch_mod.full((p.data["dfe"].numel() + 8,), float("nan"), dtype=p.dtype, device="cuda")
            view = buf[off:off + p.data["dfe"].numel()]
            view.copy_(p.data["dfe"])
            assert view.data_ptr() % 16 != 0
            got = p.run(sf, data=dict(p.window(), dfe=view))
            torch_mod.cuda.synchronize()
            assert all(torch_mod.equal(g, b) for g, b in zip(got, base)), (nq, dtype_name, off)
            if dtype_name == F64 and len(set(nq)) == 1:
                wave = p.run(sf, data=dict(p.window(), dfe=view), variant="wave")
                torch_mod.cuda.synchronize()
                assert all(torch_mod.equal(g, b) for g, b in zip(wave, base))
        p.check(base, "aligned original")


@pytest.mark.parametrize("dim,nq", [(3, 8), (3, 5), (2, 12)], ids=["3d-nq8", "3d-nq5", "2d-nq12"])
def test_analytic_gradient(sf, torch_mod, dim, nq):
    """Legendre modal basis at the Gauss-Lobatto points on affine elements x = A_e xi + c, dfe[e][a d + b] =
    (A_e^-1)[b][a]: within 1.5 gamma_N absref of the analytic gradient of the polynomial (1 for the kernel, 0.5 granted to
    the analytic reference's own rounding of df, as tests/test_gpu_physderiv.py does)."""
    nelmt, ext = 67, (nq,) * dim
    bases, derivs, df, x, exact = analytic_case(nq, dim, nelmt)
    dfe = np.ascontiguousarray(df.reshape(nelmt, dim * dim, -1)[:, :, 0]).reshape(-1)
    t = lambda a: torch_mod.tensor(a, device="cuda")      # noqa: E731
    f = sf.affine_physderiv_hex if dim == 3 else sf.affine_physderiv_quad
    _, absref = ref_affine_physderiv(ext, nelmt, bases, derivs, dfe, x)
    for variant in ("auto", "generic"):
        got = f(ext, *[t(b) for b in bases], *[t(d) for d in derivs], t(dfe), t(x), variant=variant)
        torch_mod.cuda.synchronize()
        q = affine_physderiv_excess(to_host(got), exact, absref, ext, U64, factor=1.5)
        print(f"analytic {ext} {variant}: max |gpu - analytic| / (1.5 gamma_N absref) = {q:.3g}")
        assert q <= 1.0


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (6, 6, 12)], ids=case_id)
def test_autograd_backward_is_the_transpose(sf, torch_mod, nq):
    """affine_physderiv_autograd: y = A x, loss = <f, y>; x.grad must be A^T f, i.e. <x.grad, x> = <f, A x> within
    gamma_N(transpose) <|A|^T |f|, |x|> + gamma_N(gradient) <|f|, |A| |x|>, and x.grad has the bits of
    affine_iprodderiv_*(je=None) on f."""
    dim, nelmt = len(nq), 67
    p = Problem(FAM, sf, torch_mod, nq, nelmt, F64, 23)
    bs, ds, dfe = p.consts["bs"], p.consts["ds"], p.data["dfe"]
    x = p.data["in"].clone().requires_grad_(True)
    y = sf.affine_physderiv_autograd(nq, bs, ds, dfe, x)
    f = sf.fill_random(y.numel(), 99).view(dim, -1)
    (f * y).sum().backward()
    torch_mod.cuda.synchronize()
    ipd = sf.affine_iprodderiv_hex if dim == 3 else sf.affine_iprodderiv_quad
    direct = ipd(nq, *bs, *ds, *(None,) * dim, dfe, None, f)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(x.grad, direct)
    assert all(torch_mod.equal(a, b) for a, b in zip(y.detach(), p.run(sf)))
    hb, hd = [to_host(b) for b in bs], [to_host(d) for d in ds]
    _, absy = ref_affine_physderiv(nq, nelmt, hb, hd, to_host(dfe), to_host(p.data["in"]))
    slack = float(np.sum(np.abs(to_host(f)).astype(np.longdouble) * absy))
    lhs = math.fsum(to_host(x.grad) * to_host(p.data["in"]))
    rhs = math.fsum((to_host(f) * to_host(y.detach())).reshape(-1))
    bound = (gamma(affine_iprodderiv_n(nq), U64) + gamma(affine_physderiv_n(nq), U64)) * slack
    print(f"autograd {nq}: |<A^T f, x> - <f, A x>| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0
    with pytest.raises(ValueError):
        sf.affine_physderiv_autograd(nq, bs, ds, dfe.clone().requires_grad_(True), x)


def test_batch_of_20011_hex8(sf, torch_mod):
    """20 011 elements at 3D nq = 8 (many workgroups, a ragged tail): 1 024 seeded elements and the ends against the
    long-double reference; a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 20011
    p = Problem(FAM, sf, torch_mod, nq, nelmt, F64, 8)
    y = p.run(sf)
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(20240611)
    sample = np.unique(np.concatenate(([0, 1, nelmt - 2, nelmt - 1], rng.integers(0, nelmt, 1024))))
    p.check_elements(y, "20011 elements", torch_mod.tensor(sample, device="cuda"))
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert all(torch_mod.equal(a, b) for a, b in zip(y, again))


# ---- the C ABI: validation order and overlaps, case by case ------------------------------------------------------------
def _abi(sf, torch_mod, nq=(3, 3, 3), nelmt=50):
    """(call, tensors): call(**overrides) -> rc of sf_aff_physderiv_hex_f64_variant on device buffers; an override is
    a tensor, an int address or None, `variant`, `nq` and `nelmt` included."""
    nmt, nqt = sizes(nq)
    p = Problem(FAM, sf, torch_mod, nq, nelmt, F64, 1)
    dfe = torch_mod.zeros(nelmt * 9 + 2, dtype=torch_mod.float64, device="cuda")     # room for a view one scalar further on
    dfe[:nelmt * 9] = p.data["dfe"]
    t = {"basis0": p.consts["bs"][0], "basis1": p.consts["bs"][1], "basis2": p.consts["bs"][2],
         "deriv0": p.consts["ds"][0], "deriv1": p.consts["ds"][1], "deriv2": p.consts["ds"][2], "dfe": dfe[:nelmt * 9],
         "in": p.data["in"]}
    t.update({f"out{a}": torch_mod.full((nelmt * nqt + 2,), 7.25, dtype=torch_mod.float64, device="cuda") for a in range(3)})
    order = ["basis0", "basis1", "basis2", "deriv0", "deriv1", "deriv2", "dfe", "in", "out0", "out1", "out2"]

    def ptr(v):
        if v is None:
            return None
        return ctypes.c_void_p(v if isinstance(v, int) else v.data_ptr())

    def call(variant=0, nq=nq, nelmt=nelmt, **over):
        vals = dict(t, **over)
        return sf.capi.lib().sf_aff_physderiv_hex_f64_variant(variant, *nq, nelmt, *[ptr(vals[k]) for k in order], None)

    return call, t


def test_validation_order(sf, torch_mod):
    """The order include/sumfact.h documents, each step against the next: range, empty batch, nulls, alignment, overlap,
    extents beyond the fallback, unsupported variant.  Nothing is launched by a refused call."""
    c = sf.capi
    call, t = _abi(sf, torch_mod)
    odd = t["dfe"].data_ptr() + 4                                               # not 8-byte aligned
    assert call() == c.SF_OK
    assert call(nq=(1, 3, 3), nelmt=0, dfe=None) == c.SF_EINVAL                 # (1) before (2)
    assert call(variant=99, nelmt=0) == c.SF_EINVAL
    assert call(variant=-1) == c.SF_EINVAL
    assert call(nelmt=0, dfe=None, out0=None, basis0=None) == c.SF_OK           # (2) before (3)
    for name in t:                                                              # (3): every pointer is required
        assert call(**{name: None}) == c.SF_EINVAL, name
    assert call(dfe=None, **{"in": odd}) == c.SF_EINVAL                         # (3) before (4)
    for name in t:                                                              # (4): scalar alignment of every pointer
        assert call(**{name: t[name].data_ptr() + 4}) == c.SF_EALIGN, name
    assert call(dfe=odd, out0=t["in"]) == c.SF_EALIGN                           # (4) before (5)
    assert call(nq=(13, 3, 3), nelmt=1, out1=t["out0"]) == c.SF_EINVAL          # (5) before (6)
    assert call(nq=(13, 3, 3), nelmt=1) == c.SF_ENOTBUILT                       # (6)
    assert call(nq=(13, 3, 3), nelmt=1, variant=6) == c.SF_ENOTBUILT            # (6) and (7): mfma, beyond the bounds
    assert call(variant=6) == c.SF_ENOTBUILT                                    # (7) mfma has no fused kernel
    assert call(variant=1, **{"in": t["in"].data_ptr() + 8}) == c.SF_EALIGN     # WAVE: in not 16-byte aligned
    assert call(variant=1, out2=t["out2"].data_ptr() + 8) == c.SF_EALIGN        # WAVE: one output not 16-byte aligned
    assert call(variant=1, dfe=t["dfe"].data_ptr() + 8) == c.SF_OK              # dfe needs scalar alignment only
    torch_mod.cuda.synchronize()


def test_overlap_is_refused(sf, torch_mod):
    """An output on `in`, on dfe, on its last scalar, or two outputs on the same memory: SF_EINVAL, nothing launched; an
    output that ends where dfe begins is fine."""
    c = sf.capi
    nq, nelmt = (3, 3, 3), 50
    nmt, nqt = sizes(nq)
    n = nelmt * nqt                                                             # 1350 scalars per output
    call, t = _abi(sf, torch_mod, nq, nelmt)
    big = sf.fill_random(4 * n, 5)
    keep = big.clone()
    dfe, x = big[n:n + nelmt * 9], big[2 * n:2 * n + nelmt * nmt]               # 450 and 400 scalars inside big
    cases = {"out0 on in": dict(out0=x), "out2 over the head of in": dict(out2=big[2 * n - n + 8:2 * n + 8]),
             "out1 on dfe": dict(out1=dfe), "out0 over the last scalar of dfe": dict(out0=big[n + nelmt * 9 - 1:]),
             "out1 == out0": dict(out1=t["out0"]), "out2 one scalar into out1": dict(out2=t["out1"].data_ptr() + 8)}
    for what, over in cases.items():
        assert call(dfe=dfe, **{"in": x}, **over) == c.SF_EINVAL, what
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(big, keep)
    assert all(bool((t[f"out{a}"] == 7.25).all()) for a in range(3))
    assert call(dfe=dfe, **{"in": x}, out0=big[:n]) == c.SF_OK                  # ends exactly where dfe begins
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(big[n:], keep[n:]) and not torch_mod.equal(big[:n], keep[:n])
