"""The (EC, WPB) of every BwdTrans kernel -- elements per chunk, waves (chunks) per workgroup -- for
tests/test_gpu_bwdtrans_bounds.py, which sizes its ragged batches and places its poisoned elements by them.  Imports nothing
of the product.

The wave rows are read from csrc/wave_table.h itself (the SF_HEX_CFG / SF_QUAD_CFG rows and the fp32 rules and pins beside
them).  The rows of the other launchers are a few conditional expressions in csrc/bwdtrans_hex.hip, bwdtrans_quad.hip and
bwdtrans_rt.hip; they are restated here, and tests/test_bwdtrans_cpu.py::test_kernel_rows_mirror_the_launchers holds each
restatement against the source line it mirrors.  A row that drifts changes which batch sizes are tested, never a verdict.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-benchmarking_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _macro_rows(text, macro):
    return {int(n): (int(a), int(b)) for n, a, b in re.findall(macro + r"\((\d+),\s*(\d+),\s*(\d+),", text)}


def wave_tables():
    """{"hex64", "quad64", "hex32", "quad32"}: nq -> (EC, WPB) of csrc/wave_table.h.  fp32: twice the fp64 row's elements at
    its waves per workgroup (HexCfgF32 / QuadCfgF32), unless the header pins the row."""
    text = source("wave_table.h")
    hex64, quad64 = _macro_rows(text, "SF_HEX_CFG"), _macro_rows(text, "SF_QUAD_CFG")
    hex32 = {n: (2 * ec, wpb) for n, (ec, wpb) in hex64.items()}
    quad32 = {n: (2 * ec, wpb) for n, (ec, wpb) in quad64.items()}
    for n, ec, wpb in re.findall(r"template <> struct HexCfgF32<(\d+)>[^{]*\{\s*static constexpr int EC = (\d+), WPB = (\d+)",
                                 text):
        hex32[int(n)] = (int(ec), int(wpb))
    hex32.update({int(n): (1, int(wpb)) for n, wpb in re.findall(r"SF_HEX_F32\((\d+),\s*(\d+),", text)})   # EC = 1
    for macro in ("SF_QUAD_F32_LOW", "SF_QUAD_F32_ODD", "SF_QUAD_F32"):                                     # WPB = 4
        quad32.update({int(n): (int(ec), 4) for n, ec in re.findall(macro + r"\((\d+),\s*(\d+),", text)})
    return {"hex64": hex64, "quad64": quad64, "hex32": hex32, "quad32": quad32}


_TABLES = wave_tables()


def wave_km(dim, nq):
    """Chunks per wave (KMAP) of the fp64 row; 0, the persistent mapping, counts as one in the launcher's threshold."""
    macro = "SF_HEX_CFG" if dim == 3 else "SF_QUAD_CFG"
    rows = re.findall(macro + r"\((\d+),\s*\d+,\s*\d+,\s*\w+,\s*\d+,\s*(\d+),", source("wave_table.h"))
    return max(1, {int(n): int(km) for n, km in rows}[nq])


def tuned_from(dim, nq, num_cu):
    """go<NQ>() of bwdtrans_hex.hip / bwdtrans_quad.hip: the element count from which the fp64 wave launcher runs the tuned
    row (two workgroups per CU); below it, the small-batch instantiation."""
    ec, wpb = _TABLES["hex64" if dim == 3 else "quad64"][nq]
    return 2 * ec * wpb * wave_km(dim, nq) * num_cu


def small_ec(dim, ec):
    """HexSmall / QuadSmall (bwdtrans_hex.hip, bwdtrans_quad.hip): the chunk of the one-wave workgroups that the fp64 wave
    launcher runs below two tuned workgroups per CU (tuned_from) -- the short batches of these tests."""
    if dim == 3 and ec == 1:
        return 1
    return max(2, (ec // 4 + 1) // 2 * 2)


def wave_rows(dim, nq, dtype_name):
    """The rows an isotropic wave launch of this order may take: the tuned row, and in fp64 the small-batch one.  nq = 2
    runs a stream kernel with 256-thread workgroups: the elements of one workgroup stand for the chunk."""
    f64 = dtype_name == "float64"
    if nq == 2:
        per_thread = {(3, True): 4, (2, True): 2, (3, False): 2, (2, False): 1}[(dim, f64)]   # threads per element
        return [(256 // per_thread, 1)]
    ec, wpb = _TABLES[("hex" if dim == 3 else "quad") + ("64" if f64 else "32")][nq]
    return [(ec, wpb)] + ([(small_ec(dim, ec), 1)] if f64 else [])


def triple_row(nq):
    """Cfg3 of bwdtrans_rt.hip: the compile-time anisotropic triples."""
    nqt = nq[0] * nq[1] * nq[2]
    return (min(8, max(1, 512 // nqt)), 4)


def rt_row(nq):
    """launch_hex_rt of bwdtrans_rt.hip: the run-time-extent wave kernel."""
    nq0, nq1, nq2 = nq
    nm0, nm1, nm2 = nq0 - 1, nq1 - 1, nq2 - 1
    s0, s1, s2 = nm0 | 1, nm1 | 1, nm2 | 1
    nqt = nq0 * nq1 * nq2

    def images(ec):
        in_img, w2, w1 = nm2 * nm1 * s0, nq1 * nq0 * s2, nq0 * nm2 * s1
        return ((ec * max(in_img, w2) + 1) & ~1) + ((ec * max(w1, nqt) + 1) & ~1)

    ec = min(16, max(1, 64 // (nq0 * nq1)))
    while ec > 1 and images(ec) > 2048:
        ec -= 1
    wpb = 4
    while wpb > 1 and 8 * wpb * images(ec) > 64 * 1024:
        wpb >>= 1
    return (ec, wpb)


def quad_mfma_row(nq, dtype_name="float64"):
    """go_mfma / go_f32 of bwdtrans_quad.hip: quad_mfma_kernel."""
    if dtype_name == "float32":
        return (4 if nq in (25, 28, 32) else 2, 4)
    return (4 if 13 <= nq <= 15 else 2, 2 if 25 <= nq <= 31 else 4)


def hex_mfma_row(nq, dtype_name="float64"):
    """go_mfma / go_f32 of bwdtrans_hex.hip: hex_mfma_kernel."""
    if dtype_name == "float32":
        return (1, 1)
    return (2, 2) if nq <= 10 else (1, 4 if nq == 11 else 1)


def quad_mfma4_row(nq):
    """go_mfma4 of bwdtrans_quad.hip: quad_mfma4_kernel; from nq = 25 a persistent grid fed from a batch counter."""
    return (4, 4) if 25 <= nq <= 27 else (2, 4)


def hex_mfma4_row(nq, direct):
    """go_mfma4 of bwdtrans_hex.hip: hex_mfma4_kernel, one element per chunk and one wave per workgroup on both output
    paths."""
    return (1, 1)


THREAD_ROW = (128, 1)     # launch_*_generic_t: hinted_block(128, ..) elements per workgroup, one per thread
BLOCK_ROW = (1, 1)        # block-lds, block-glb, generic: a workgroup per element

QUAD_F32_MFMA_FROM, HEX_F32_MFMA_FROM = 25, 13     # kQuadF32MfmaFrom; go_f32 of bwdtrans_hex.hip


def f32_auto_rows(dim, nq):
    """(kernel, rows) of what AUTO runs for T = float at an isotropic order on the tables."""
    if dim == 2 and nq >= QUAD_F32_MFMA_FROM:
        return "mfma", [quad_mfma_row(nq, "float32")]
    if dim == 3 and nq >= HEX_F32_MFMA_FROM:
        return "mfma", [hex_mfma_row(nq, "float32")]
    return "wave", wave_rows(dim, nq, "float32")


def ragged_counts(rows, limit=340):
    """1 element, one less and one more than a chunk, one workgroup of chunks plus one element, two workgroups plus three,
    for every row; `limit` keeps the long-double reference at a second or two (the largest count is 4 * 84 + 1 = 337 at
    the fp32 2D nq = 3 row)."""
    out = {1}
    for ec, wpb in rows:
        out |= {ec - 1, ec + 1, ec * wpb + 1, 2 * ec * wpb + 3}
    return sorted(n for n in out if 1 <= n <= limit)
