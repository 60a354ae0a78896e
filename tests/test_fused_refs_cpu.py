"""CPU checks of what the GPU tests of the fused families lean on (tests/fused_families.py), at shapes the references
have not been run at before:

  * on the one-mode shapes of tests/test_gpu_fused_extents.py (an extent of 2 -- one mode -- beside the largest extent the
    any-extent kernels take) each family's fp64 numpy reference agrees with its long-double reference inside the
    family's bound, for every combination of optional coefficients; so does the reference of absolute values;
  * the LDS class that fused_families.py writes beside each boundary shape is the one its formula gives;
  * SMALL_CAP and the extent bounds are the constants of csrc/helmholtz_generic.h, mass_generic.hip and
    iproduct_generic.hip, and the class formulas those files state are the ones lds_need() restates;
  * the (EC, WPB) mirror that sizes the batches of tests/test_gpu_fused_offsets.py and test_gpu_fused_scale.py is what
    csrc/wave_table.h and csrc/helmholtz_launch.h say.
"""
import os
import re

import numpy as np
import pytest

import fused_families as ff
from fused_families import FAMILIES, U64, case_id

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-benchmarking_amd", "csrc")

ONE_MODE = [(f, nq) for f in FAMILIES for nq in ff.one_mode_shapes(f)]


@pytest.mark.parametrize("fam,nq", ONE_MODE, ids=[f"{f.name}-{case_id(nq)}" for f, nq in ONE_MODE])
def test_fp64_reference_agrees_with_long_double_on_one_mode_shapes(fam, nq):
    nelmt = 3
    for present in fam.modes:
        consts, data = ff.host_case(fam, nq, nelmt, present, seed=sum(nq) + len(present))
        ref, absref = fam.ref(nq, nelmt, consts, data, ld=True)
        out64, abs64 = fam.ref(nq, nelmt, consts, data, ld=False)
        assert np.asarray(ref).dtype == np.longdouble and np.asarray(out64).dtype == np.float64
        assert np.asarray(out64).shape == np.asarray(ref).shape
        assert np.asarray(ref).size == nelmt * fam.out_parts(nq) * fam.out_per(nq)
        assert float(np.max(np.abs(ref))) > 0
        q = fam.excess(out64, ref, absref, nq, U64)
        qa = fam.excess(abs64, absref, absref, nq, U64)
        print(f"{fam.name} {nq} present={present}: fp64 against long double {q:.3g}, of absolute values {qa:.3g}")
        assert q <= 1.0 and qa <= 1.0, (fam.name, nq, present, q, qa)


@pytest.mark.parametrize("fam", FAMILIES, ids=case_id)
def test_class_of_every_boundary_shape(fam):
    sides = set()
    for nq, side in ff.boundary_shapes(fam):
        need = ff.lds_need(fam, nq)
        assert (need <= ff.SMALL_CAP) == (side == "small"), (fam.name, nq, need, side)
        sides.add((len(nq), side))
    # 2D mass and 2D iproduct never leave the small class: 32 * 63 = 2016
    want = {(3, "small"), (3, "large")} | ({(2, "small"), (2, "large")} if fam.helm_rows else set())
    assert want <= sides
    if not fam.helm_rows:
        assert max(ff.lds_need(fam, (a, b)) for a in range(2, 33) for b in range(2, 33)) == 2016


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _const(text, name):
    return int(re.search(r"\b" + name + r"\s*=\s*(\d+)", text).group(1))


def test_lds_caps_and_extent_bounds_mirror_the_sources():
    """The tags "small" / "large" of the boundary shapes hang on these constants and formulas.  Like the test below, this
    one reads source text: a failure after a reformat or a rename in csrc means "update the mirror in fused_families.py
    (and the shapes, if a value moved)", not that a kernel is wrong."""
    helm, mass, iprod = _src("helmholtz_generic.h"), _src("mass_generic.hip"), _src("iproduct_generic.hip")
    assert {_const(helm, "kHelmSmallCap"), _const(mass, "kMassSmallCap"), _const(iprod, "kIprodSmallCap")} == {ff.SMALL_CAP}
    assert (_const(helm, "kHelmMax3D"), _const(helm, "kHelmMax2D")) == ff.MAX_EXTENT["helm"]
    assert (_const(mass, "kMassMax3D"), _const(mass, "kMassMax2D")) == ff.MAX_EXTENT["wide"]
    assert (_const(iprod, "kIprodMax3D"), _const(iprod, "kIprodMax2D")) == ff.MAX_EXTENT["wide"]
    # the formulas lds_need() restates, and that the launchers compare them with the small cap
    assert "return dim == 3 ? 4 * nq0 * nq1 * nq2 : 3 * nq0 * nq1;" in helm
    assert "sizeA = nq0 * nq1 * nq2;" in mass and "sizeB = nq0 * nq1 * (nq2 - 1);" in mass
    assert "sizeA = nq0 * nq1;" in mass and "sizeB = nq0 * (nq1 - 1);" in mass
    assert "sizeA + sizeB <= (unsigned)kMassSmallCap" in mass
    assert "need = nq[0] * nq[1] * nz + (nq[0] - 1) * nq[1] * nz;" in iprod and "need <= (unsigned)kIprodSmallCap" in iprod
    for name in ("helmholtz_generic.hip", "affine_generic.hip", "physderiv_generic.hip", "iprodderiv_generic.hip"):
        assert "helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap" in _src(name), name
    # the shapes of the GPU tests lie at these bounds, and one past them
    for fam in FAMILIES:
        m3, m2 = ff.MAX_EXTENT["helm" if fam.helm_rows else "wide"]
        shapes = [nq for nq, _ in ff.boundary_shapes(fam)] + ff.one_mode_shapes(fam)
        assert max(max(nq) for nq in shapes if len(nq) == 3) == m3 and max(max(nq) for nq in shapes if len(nq) == 2) == m2
        assert all(max(nq) == (m3 if len(nq) == 3 else m2) + 1 for nq in ff.past_the_bounds(fam))


def _rows(text, macro):
    return {int(n): (int(ec), int(wpb)) for n, ec, wpb in re.findall(macro + r"\((\d+),\s*(\d+),\s*(\d+),", text)}


def test_wave_rows_mirror_the_headers():
    """Reads source text, literal lines included: a failure after a reformat or a rename in csrc that changes no behaviour
    only means "update the mirror in fused_families.py".  It guards the batch sizes of the offsets and windows tests."""
    with open(os.path.join(CSRC, "wave_table.h")) as fh:
        table = fh.read()
    with open(os.path.join(CSRC, "helmholtz_launch.h")) as fh:
        helm = fh.read()
    hex64, quad64 = _rows(table, "SF_HEX_CFG"), _rows(table, "SF_QUAD_CFG")
    assert {n: hex64[n] for n in ff.HEX64} == ff.HEX64
    assert {n: quad64[n] for n in ff.QUAD64} == ff.QUAD64
    # fp32: twice the elements of the fp64 row at its waves per block, unless pinned
    assert "EC = 2 * HexCfg<NQ>::EC, WPB = HexCfg<NQ>::WPB" in table
    assert "EC = 2 * QuadCfg<NQ>::EC, WPB = QuadCfg<NQ>::WPB" in table
    pinned = re.findall(r"template <> struct HexCfgF32<(\d+)>[^{]*\{\s*static constexpr int EC = (\d+), WPB = (\d+)", table)
    assert {int(n): (int(e), int(w)) for n, e, w in pinned} == ff.HEX32_PINNED
    quad32 = {}
    for macro in ("SF_QUAD_F32_LOW", "SF_QUAD_F32_ODD", "SF_QUAD_F32"):       # each of them: WPB = 4
        assert re.search(r"#define " + macro + r"\(.*?EC = EC_, WPB = 4,", table, re.S)
        quad32.update({int(n): (int(ec), 4) for n, ec in re.findall(macro + r"\((\d+),\s*(\d+),", table)})
    assert {n: r for n, r in quad32.items() if n <= 16} == ff.QUAD32_PINNED
    # the EC overrides that helm_ec() restates, and the launchers that share them
    for line in ("if (nq == 6 && scalar_bytes == 8)", "const int cap = 128 / (nq * nq) > 0 ? 128 / (nq * nq) : 1;",
                 "const int cap = nq >= 9 ? 128 / nq : row_ec;", "return row_ec < cap ? row_ec : cap;"):
        assert line in helm, line
    for name in ("affine_launch.h", "physderiv_launch.h", "iprodderiv_launch.h"):
        with open(os.path.join(CSRC, name)) as fh:
            assert "launch_helm_wave<DIM, T>(nq, a, " in fh.read(), name
    assert ff.wave_row(ff.BY_NAME["iprodderiv"], 3, 6, "float32") == (3, 4)
    assert ff.wave_row(ff.BY_NAME["helmholtz"], 3, 6, "float64") == (1, 8)
    assert ff.wave_row(ff.BY_NAME["physderiv"], 2, 9, "float32") == (8, 4)
    assert ff.wave_row(ff.BY_NAME["mass"], 3, 9, "float32") == (4, 2)
