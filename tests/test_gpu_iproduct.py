"""GPU tests of IProductWRTBase (include/sumfact.h sf_iproduct_*), the transpose of BwdTrans, that are the family's own:
8-byte-aligned views, the full 1 048 576-element batch with adjointness to the GPU BwdTrans, and the autograd binding.
install() adds the family's cases of the parametrised tests the fused families share (tests/fused_common.py: every wave
order through AUTO, ragged counts, the fallback, explicit variants, guard bands); refusals, stream capture and two
streams in flight are tests/test_gpu_fused_common.py.

Reference and bounds: tests/iprod_ref.py.  Elementwise |gpu - ref| <= gamma_n * absref against a long-double reference,
gamma_n = n u / (1 - n u), n = nq0 + nq1 (+ nq2), u = 2^-53 (fp64) or 2^-24 (fp32); where long double would be too
slow, 2 gamma_n (1 + gamma_n) * absref64 against fp64 CPU sweeps, and the adjointness bound with the GPU BwdTrans."""
import math

import numpy as np
import pytest

from fused_common import install
from fused_families import BY_NAME, case_id, sf, to_host, torch_mod  # noqa: F401
from iprod_ref import (U64, adjoint_bound, elementwise_excess, iprod_f64, ref_iprod,
                       unit_roundoff)

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["iproduct"])


def _bases(sf, torch_mod, nq, dtype_name, seed):
    dtype = getattr(torch_mod, dtype_name)
    return [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]


def _iprod(sf, nq, bs, x, **kw):
    return (sf.iproduct_hex if len(nq) == 3 else sf.iproduct_quad)(tuple(nq), *bs, x, **kw)


def _check(nq, nelmt, bs, x, got, dtype_name, what):
    ref, absref = ref_iprod(nq, nelmt, [to_host(b) for b in bs], to_host(x))
    q = elementwise_excess(to_host(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"{what}: {nq} {dtype_name} nelmt={nelmt}: max |err| / (gamma_n absref) = {q:.3g}")
    assert q <= 1.0, (what, nq, dtype_name, nelmt, q)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=case_id)
def test_eight_byte_aligned_views_take_the_fallback(sf, torch_mod, nq):
    nelmt = 333
    nqt, nmt = int(np.prod(nq)), int(np.prod([q - 1 for q in nq]))
    for dtype_name, offsets in (("float64", ((1, 0), (0, 1), (1, 3))), ("float32", ((2, 0), (0, 2), (1, 3)))):
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 4)
        for off_in, off_out in offsets:
            xbuf = sf.fill_random(nelmt * nqt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nqt]
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            _iprod(sf, nq, bs, x, out=o)
            torch_mod.cuda.synchronize()
            _check(nq, nelmt, bs, x, o, dtype_name, f"view {off_in}/{off_out}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                with pytest.raises(sf.capi.SumfactError) as ei:
                    _iprod(sf, nq, bs, x, out=o, variant="wave")
                assert ei.value.rc == sf.capi.SF_EALIGN


def test_full_batch_hex8(sf, torch_mod):
    """1 048 576 elements at 3D nq = 8: elementwise against fp64 CPU sweeps (bound 2 gamma_n (1 + gamma_n) absref64),
    then adjointness with the GPU BwdTrans."""
    nq, nelmt = (8, 8, 8), 1 << 20
    nqt, nmt = 512, 343
    bs = _bases(sf, torch_mod, nq, "float64", 8)
    bh = [to_host(b) for b in bs]
    v = sf.fill_random(nelmt * nqt, 1234)
    w = sf.iproduct_hex(nq, *bs, v)
    torch_mod.cuda.synchronize()
    step, worst = 1 << 15, 0.0
    for lo in range(0, nelmt, step):
        vv = to_host(v[lo * nqt:(lo + step) * nqt])
        out64, abs64 = iprod_f64(nq, step, bh, vv)
        g = sum(nq) * U64 / (1 - sum(nq) * U64)
        worst = max(worst, elementwise_excess(to_host(w[lo * nmt:(lo + step) * nmt]), out64, abs64, nq, U64,
                                              factor=2 * (1 + g)))
    print(f"full batch: max |err| / (2 gamma_n (1 + gamma_n) absref64) = {worst:.3g}")
    assert worst <= 1.0
    del v
    # adjointness: sum_e <B x, y>_e against sum_e <x, I y>_e
    x = sf.fill_random(nelmt * nmt, 4321)
    y = sf.fill_random(nelmt * nqt, 8765)
    bx = sf.bwdtrans_hex(nq, *bs, x)
    iy = sf.iproduct_hex(nq, *bs, y)
    babs = sf.bwdtrans_hex(nq, *[b.abs() for b in bs], x.abs())
    torch_mod.cuda.synchronize()

    def dots(a, b):
        return (a.view(nelmt, -1) * b.view(nelmt, -1)).sum(dim=1).cpu().numpy()

    lhs = math.fsum(dots(bx, y))
    rhs = math.fsum(dots(x, iy))
    scale = math.fsum(dots(babs, y.abs()))
    bound = adjoint_bound(nq, U64) * scale
    print(f"adjointness: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("nq,nelmt", [((4, 4, 4), 3), ((5, 5), 4)], ids=lambda v: case_id(v))
def test_bwdtrans_autograd_gradcheck(sf, torch_mod, nq, nelmt):
    bs = _bases(sf, torch_mod, nq, "float64", 2)
    nmt = int(np.prod([q - 1 for q in nq]))
    x = sf.fill_random(nelmt * nmt, 17).requires_grad_(True)
    assert torch_mod.autograd.gradcheck(lambda t: sf.bwdtrans_autograd(nq, bs, t), (x,))
    # the backward pass is IProductWRTBase of the output gradient
    y = sf.bwdtrans_autograd(nq, bs, x)
    gy = sf.fill_random(y.numel(), 18)
    (gx,) = torch_mod.autograd.grad(y, x, gy)
    assert torch_mod.equal(gx, _iprod(sf, nq, bs, gy))
    with pytest.raises(ValueError):
        sf.bwdtrans_autograd(nq, [bs[0].clone().requires_grad_(True)] + bs[1:], x)

