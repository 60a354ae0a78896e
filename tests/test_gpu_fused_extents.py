"""GPU tests of the any-extent kernels of the six fused families (csrc/*_generic.hip, csrc/any_extent.h) at the edges
of their own arithmetic.  The families' files run nine to twelve fallback shapes, all well inside an LDS class, at no more
than 4099 elements.

test_grid_stride_loop: launch_any_extent() caps the grid at 2^22 workgroups and leaves the rest to the kernels' loop
`for (e = blockIdx.x; e < nelmt; e += gridDim.x)`.  variant "generic" on (3, 3) -- the cheapest shape every family
takes -- with 2^22 + 4099 elements: the 4099 elements from 2^22 on are the second trip of the loop.  The whole batch
against the fp64 numpy reference, the second trip also on its own.

test_class_boundaries_and_one_mode_directions: each kernel carves run-time-sized images out of a static lds[CAP] of a
small or a large class, chosen by a formula per family (tests/fused_families.py restates the three and writes the
arithmetic beside each shape; tests/test_fused_refs_cpu.py checks the tags).  The shapes sit on both sides of each switch
and at the extent bounds, and beside them shapes with an extent of 2 -- one mode, so every sweep along it is a single
product -- next to the largest extent the kernel takes.  1, 5 and 33 elements, every combination of optional coefficients,
both precisions, against the long-double reference (computed once at 33 elements; the smaller counts are prefixes).
AUTO reaches the any-extent kernel on a shape that is off the wave table; on a table shape ((8, 8, 8), (10, 10, 10)) fp64
asks for variant "generic", and float32, which has the AUTO route only, hands AUTO an output one scalar off 16-byte
alignment.

test_one_past_each_bound: SF_ENOTBUILT.
"""
import pytest

import fused_families as ff
from fused_families import FAMILIES, Problem, case_id, excess_over_slices, sf, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


def _nan_outs(torch_mod, fam, nq, nelmt, dtype_name, off=0):
    """NaN-filled outputs of nelmt elements; off = 1: one scalar past a 16-byte boundary."""
    n = nelmt * fam.out_per(nq)
    return [torch_mod.full((n + 4,), float("nan"), dtype=getattr(torch_mod, dtype_name), device="cuda")[off:off + n]
            for _ in range(fam.out_parts(nq))]


@pytest.mark.parametrize("fam", FAMILIES, ids=case_id)
def test_grid_stride_loop(sf, torch_mod, fam):
    nq, cap = (3, 3), 1 << 22
    nelmt = cap + 4099
    p = Problem(fam, sf, torch_mod, nq, nelmt, "float64", 3)
    outs = _nan_outs(torch_mod, fam, nq, nelmt, "float64")
    p.run(sf, out=outs, variant="generic")
    torch_mod.cuda.synchronize()
    assert all(bool(torch_mod.isfinite(t).all()) for t in outs), fam.name
    second = excess_over_slices(p, outs, None, 1 << 17, lo=cap)
    whole = excess_over_slices(p, outs, None, 1 << 17)
    print(f"grid stride {fam.name}: max |err| / (f64_factor gamma_N absref64) = {whole:.3g} over {nelmt} elements, "
          f"{second:.3g} over the {nelmt - cap} of the second trip")
    assert second <= 1.0 and whole <= 1.0, (fam.name, second, whole)


SHAPES = [(f, nq, side) for f in FAMILIES for nq, side in ff.boundary_shapes(f)] + \
         [(f, nq, "one-mode") for f in FAMILIES for nq in ff.one_mode_shapes(f)]


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("fam,nq,side", SHAPES, ids=[f"{f.name}-{case_id(nq)}-{s}" for f, nq, s in SHAPES])
def test_class_boundaries_and_one_mode_directions(sf, torch_mod, fam, nq, side, dtype_name):
    if side != "one-mode":
        assert (ff.lds_need(fam, nq) <= ff.SMALL_CAP) == (side == "small")
    table = ff.on_wave_table(fam, nq)
    variant = "generic" if table and dtype_name == "float64" else "auto"
    off = 1 if table and dtype_name == "float32" else 0      # AUTO leaves the wave table for an out that is not 16-byte aligned
    p = Problem(fam, sf, torch_mod, nq, 33, dtype_name, sum(nq))
    per, worst = fam.out_per(nq), 0.0
    for present in fam.modes:
        ref, absref = p.reference(present=present)
        for nelmt in (1, 5, 33):
            outs = _nan_outs(torch_mod, fam, nq, nelmt, dtype_name, off)
            assert all((t.data_ptr() % 16 != 0) == bool(off) for t in outs)
            p.run(sf, n=nelmt, present=present, out=outs, variant=variant)
            torch_mod.cuda.synchronize()
            what = (fam.name, nq, dtype_name, nelmt, present)
            assert all(bool(torch_mod.isfinite(t).all()) for t in outs), what
            q = p.excess(outs, ref[:, :nelmt * per], absref[:, :nelmt * per])
            worst = max(worst, q)
            assert q <= 1.0, (q,) + what
    print(f"extents {fam.name} {nq} {side} {dtype_name}: max |err| / (gamma_N absref) = {worst:.3g}")


@pytest.mark.parametrize("fam", FAMILIES, ids=case_id)
def test_one_past_each_bound(sf, torch_mod, fam):
    for nq in ff.past_the_bounds(fam):
        for dtype_name in ("float64", "float32"):
            p = Problem(fam, sf, torch_mod, nq, 2, dtype_name, 1)
            for variant in ("auto", "generic") if dtype_name == "float64" else ("auto",):
                with pytest.raises(sf.capi.SumfactError) as ei:
                    p.run(sf, variant=variant)
                assert ei.value.rc == sf.capi.SF_ENOTBUILT, (fam.name, nq, dtype_name, variant)
