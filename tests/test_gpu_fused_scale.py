"""GPU tests of the six fused families at batch sizes their own test files do not reach.

test_every_order_over_several_xcd_windows: workgroups are renumbered in windows of 8 * XG = 512 (logical_block<XG>,
csrc/sf_common.h); a grid that is no whole number of windows keeps a tail in identity order.  The families' files launch
3D nq 7 / 8 and 2D nq 9 / 12 that large and nothing else.  Here every wave order of every family, in both precisions,
runs one batch of 2^24 // nq^d + 1 elements, enlarged where the row needs it until the grid of launch_chunked
(csrc/wave_launch.h) holds at least three full windows, a partial one, and a ragged last chunk.  The grid follows from
the row's EC and WPB, which tests/fused_families.py mirrors from csrc/wave_table.h and the EC overrides of
csrc/helmholtz_launch.h (tests/test_fused_refs_cpu.py holds the mirror to the headers).  By those tables the starting
count gives 1552 workgroups or more on every row -- the fewest on iproduct / mass 2D nq 13 (64 elements per workgroup)
and 3D nq 11 (1576) in float32 -- and only the remainder conditions move it, by one element on sixteen rows.  The test
asserts the conditions on the count it runs and prints the grid.  The whole output is compared with the fp64 numpy
reference, elementwise, in slices.  The combinations of optional coefficients alternate over the orders.

test_streams_past_2_to_the_32_scalars: 3D nq 8 in float32 (the index arithmetic is in scalars, float32 halves the bytes),
the element count chosen so that the family's longest array just exceeds 2^32 scalars.  Windows of 300 elements against
the long-double reference at the head, across the elements where that array's scalar index passes 2^31 and 2^32, and at
the tail; the whole output bit-identical to the same data computed in two calls split at a multiple of 64 elements, each
of which keeps every array below 2^32 scalars; sf.fill_random itself against the oracle's generator across index 2^32
and at the tail.  26 to 46 GB of device memory per family, freed before the next.

Bounds: the family's own gamma_N (tests/*_ref.py), factor 1 against long double; against fp64 the factor of
Problem.f64_factor(), 2 (1 + gamma_N) for an fp64 result.
"""
import gc

import numpy as np
import pytest

from fused_families import (FAMILIES, WAVE_CASES, Problem, case_id, excess_over_slices, sf, sizes, to_host,  # noqa: F401
                            torch_mod, wave_ids, wave_row)

pytestmark = pytest.mark.gpu

WINDOW = 512                  # workgroups per renumbering window: 8 XCDs * XG = 64 (csrc/wave_table.h XG64)


def batch_for_windows(dim, nq, ec, wpb):
    """(nelmt, grid): from 2^24 // nq^d + 1 elements up, the first count whose grid (launch_chunked of
    csrc/wave_launch.h with KMAP = 1: chunks of EC elements, WPB chunks per workgroup) holds at least three full windows
    and a partial one, and whose last chunk is ragged (EC = 1: whose last workgroup is short of WPB elements)."""
    nelmt = (1 << 24) // nq ** dim + 1
    while True:
        grid = -(-(-(-nelmt // ec)) // wpb)
        if grid // WINDOW >= 3 and grid % WINDOW != 0 and (nelmt % ec != 0 if ec > 1 else nelmt % wpb != 0):
            return nelmt, grid
        nelmt += ec * wpb if grid // WINDOW < 3 else 1


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("fam,dim,nq", WAVE_CASES, ids=wave_ids())
def test_every_order_over_several_xcd_windows(sf, torch_mod, fam, dim, nq, dtype_name):
    ext = (nq,) * dim
    ec, wpb = wave_row(fam, dim, nq, dtype_name)
    nelmt, grid = batch_for_windows(dim, nq, ec, wpb)
    assert grid // WINDOW >= 3 and grid % WINDOW != 0 and (nelmt % ec != 0 if ec > 1 else nelmt % wpb != 0)
    present = fam.modes[(nq + (dtype_name == "float32")) % len(fam.modes)]
    p = Problem(fam, sf, torch_mod, ext, nelmt, dtype_name, nq)
    parts, per = fam.out_parts(ext), fam.out_per(ext)
    dtype = getattr(torch_mod, dtype_name)
    outs = [torch_mod.full((nelmt * per,), float("nan"), dtype=dtype, device="cuda") for _ in range(parts)]
    p.run(sf, present=present, out=outs)
    torch_mod.cuda.synchronize()
    assert all(bool(torch_mod.isfinite(t).all()) for t in outs), (fam.name, ext, dtype_name, nelmt)
    step = max(64, (1 << 20) // sizes(ext)[1])               # about 2^20 points per slice
    worst = excess_over_slices(p, outs, present, step)
    print(f"windows {fam.name} {ext} {dtype_name} nelmt={nelmt} grid={grid} present={present}: "
          f"max |err| / (f64_factor gamma_N absref64) = {worst:.3g}")
    assert worst <= 1.0, (fam.name, ext, dtype_name, nelmt, worst)
    again = [torch_mod.full((nelmt * per,), float("nan"), dtype=dtype, device="cuda") for _ in range(parts)]
    p.run(sf, present=present, out=again)
    torch_mod.cuda.synchronize()
    assert all(torch_mod.equal(a, b) for a, b in zip(outs, again))


def _all_finite(torch_mod, t, block=1 << 28):
    return all(bool(torch_mod.isfinite(t[a:a + block]).all()) for a in range(0, t.numel(), block))


@pytest.mark.parametrize("fam", FAMILIES, ids=case_id)
def test_streams_past_2_to_the_32_scalars(sf, torch_mod, oracle, fam):
    ext, dtype_name, win = (8, 8, 8), "float32", 300
    name, per_big = fam.largest_stream(ext)
    assert name != "out"                                      # the longest array is an input, filled by sf.fill_random
    nelmt = (1 << 32) // per_big + 1 + 333
    nelmt += 1 - nelmt % 2                                    # odd: a ragged last chunk (EC = 2) in a partial workgroup
    assert nelmt * per_big > 1 << 32
    parts, per = fam.out_parts(ext), fam.out_per(ext)
    split = nelmt // 2 // 64 * 64
    ops = fam.operands(ext)
    assert all(max(split, nelmt - split) * max(o.per, per) < 1 << 32 for o in ops)
    floats = sum(nelmt * o.per for o in ops) + parts * per * (nelmt + nelmt - split)
    need = 4 * floats + (2 << 30)
    free, _ = torch_mod.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"not enough device memory: {need >> 30} GiB")
    held = []                                                 # every large allocation, released whatever happens below
    try:
        p = Problem(fam, sf, torch_mod, ext, nelmt, dtype_name, 8)
        held += list(p.data.values())
        big = p.data[name]
        assert big.numel() > 1 << 32

        # the generator past 2^32 values: across the index 2^32 and at the tail
        for first in ((1 << 32) - 2048, big.numel() - 4096):
            want = oracle.fill_random(4096, p.seeds[name], first_idx=first).astype(np.float32)
            assert np.array_equal(to_host(big[first:first + 4096]), want), (fam.name, first)

        outs = [torch_mod.full((nelmt * per,), float("nan"), dtype=torch_mod.float32, device="cuda") for _ in range(parts)]
        held += outs
        p.run(sf, out=outs)
        torch_mod.cuda.synchronize()
        assert all(_all_finite(torch_mod, t) for t in outs), fam.name

        e31, e32 = (1 << 31) // per_big, (1 << 32) // per_big      # the elements that hold scalar 2^31 and 2^32 of `name`
        worst = 0.0
        for lo in (0, e31 - win // 2, e32 - win // 2, nelmt - win):
            assert 0 <= lo and lo + win <= nelmt
            ref, absref = p.reference(lo, win)
            q = p.excess([t[lo * per:(lo + win) * per] for t in outs], ref, absref)
            print(f"past 2^32 {fam.name} {name}: elements {lo} .. {lo + win}: max |err| / (gamma_N absref) = {q:.3g}")
            worst = max(worst, q)
        assert worst <= 1.0, (fam.name, worst)

        # the same data in two calls, each with every array below 2^32 scalars
        half = [torch_mod.empty(((nelmt - split) * per,), dtype=torch_mod.float32, device="cuda") for _ in range(parts)]
        held += half
        for lo, n in ((0, split), (split, nelmt - split)):
            views = [h[:n * per] for h in half]
            for v in views:
                v.fill_(float("nan"))
            p.run(sf, lo=lo, n=n, out=views)
            torch_mod.cuda.synchronize()
            assert all(torch_mod.equal(v, t[lo * per:(lo + n) * per]) for v, t in zip(views, outs)), (fam.name, lo, n)
        print(f"past 2^32 {fam.name}: nelmt={nelmt}, {name} holds {big.numel()} scalars, {need >> 30} GiB; "
              f"max |err| / (gamma_N absref) = {worst:.3g}")
    finally:
        # a failed assertion keeps this frame, and the frames of a failed call keep views: shrink the storages themselves,
        # or the families after this one would find the memory taken and skip
        for t in held:
            t.untyped_storage().resize_(0)
        gc.collect()
        torch_mod.cuda.empty_cache()
