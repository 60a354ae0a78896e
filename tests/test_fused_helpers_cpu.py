"""CPU checks of the helpers the common tests lean on: check_bound(), the assertion every result of the fused families
is held to, and Banded, the guard bands (tests/fused_families.py); parse(), which every kernel-resource test reads the
compiler's report through (tests/resources_ref.py).  No device and no compiler is needed: check_bound() takes host arrays,
Banded a device argument, parse() a line.
"""
import numpy as np
import pytest
import torch

import fused_families as ff
from fused_families import COMMON, F64, U64, Banded, check_bound, gamma
from resources_ref import parse

CASES = [(f, nq) for f in COMMON for nq in ((3, 4), (3, 4, 2))]


@pytest.mark.parametrize("fam,nq", CASES, ids=[f"{f.name}-{ff.case_id(nq)}" for f, nq in CASES])
def test_check_bound_passes_the_fp64_reference_and_fails_one_moved_entry(fam, nq):
    nelmt = 3
    for present in fam.modes:
        consts, data = ff.host_case(fam, nq, nelmt, present, seed=sum(nq) + len(present))
        shape = (fam.out_parts(nq), nelmt * fam.out_per(nq))
        ref, absref = (np.asarray(a).reshape(shape) for a in fam.ref(nq, nelmt, consts, data, ld=True))
        out64 = np.asarray(fam.ref(nq, nelmt, consts, data, ld=False)[0]).reshape(shape)
        assert ref.dtype == np.longdouble and out64.dtype == np.float64
        check_bound(fam, nq, F64, out64, ref, absref, f"fp64 reference present={present}")
        # one entry, the one with the largest bound, moved by twice its bound
        at = np.unravel_index(np.argmax(absref), shape)
        moved = out64.copy()
        moved[at] += float(2 * gamma(fam.n(nq), U64) * absref[at])
        assert moved[at] != out64[at]
        with pytest.raises(AssertionError):
            check_bound(fam, nq, F64, moved, ref, absref, "one entry moved")
        with pytest.raises(AssertionError):                       # a reference that is all zero checks nothing
            check_bound(fam, nq, F64, np.zeros(shape), np.zeros(shape, dtype=np.longdouble), absref, "zero reference")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("fill", [-3.5, float("nan")], ids=["sentinel", "nan"])
def test_banded_detects_one_changed_scalar_in_either_band(dtype, fill):
    for off, lines in ((0, 4), (5, 2)):
        b = Banded(torch, dtype, 37, off, fill, lines=lines, device="cpu")
        line = 128 // b.buf.element_size()
        assert b.view.numel() == 37 and b.lo == lines * line + off and b.buf.numel() == b.hi + lines * line
        b.view.fill_(1.0)                                         # the view itself is free to change
        assert b.bands_intact(torch)
        for at in (0, b.lo - 1, b.hi, b.buf.numel() - 1):        # both ends of both bands
            b.reset()
            b.buf[at] = 2.0
            assert not b.bands_intact(torch), at
        b.reset()
        assert b.bands_intact(torch)
    src = torch.arange(11, dtype=dtype)
    c = Banded.of(torch, src, fill)
    assert torch.equal(c.view, src) and c.bands_intact(torch) and c.view.data_ptr() % 16 == c.buf.data_ptr() % 16


def test_parse_reads_a_resource_line_and_refuses_scratch_spills_and_too_many_vgprs():
    line = "{:70s} vgpr {:3d} agpr {:3d} sgpr {:3d} scratch {:5d} spill v{}/s{} occ {}".format
    name = "hex_mass_wave_kernel<8, 8, 8, 1, 4, double>"
    r = parse(line(name, 124, 0, 58, 0, 0, 0, 4))
    assert r == (name, 124, 0, 58, 0, 0, 0, 4) and (r.vgpr, r.sgpr, r.occ) == (124, 58, 4)
    assert parse(line(name, 256, 0, 102, 0, 0, 0, 2)).vgpr == 256
    for bad in (line(name, 124, 0, 58, 8, 0, 0, 4),                # scratch
                line(name, 124, 0, 58, 0, 3, 0, 4),                # a VGPR spill
                line(name, 124, 0, 58, 0, 0, 1, 4),                # an SGPR spill
                line(name, 257, 0, 58, 0, 0, 0, 4),                # one VGPR too many
                line(name, -1, -1, -1, -1, -1, -1, -1),            # a report without figures
                name + " vgpr 124 sgpr 58",                        # not the tool's line
                "error: no such kernel"):
        with pytest.raises(AssertionError):
            parse(bad)
