"""GPU tests of every BwdTrans kernel (include/sumfact.h sf_bwdtrans_*) against the long-double reference of
tests/bwd_ref.py, element by element:  |gpu - ref| <= gamma_N absref,  N = sum_d (nq_d - 1),  u = 2^-53 or 2^-24 -- the
bound the fused families are held to, derived in bwd_ref.py, where tests/test_gpu_parity.py judges a whole batch by
max |gpu - oracle| / max |oracle| <= 1e-12 (2e-5 in fp32).

(a) every kernel by name -- the wave kernels (isotropic, the compile-time triples, run-time extents), the four
    matrix-core kernels, the baseline variants, the generic kernels above the tables, the interleaved layout, and the fp32
    AUTO routes -- at every order it is built for, on ragged element counts placed by the kernel's own (EC, WPB): 1
    element, one less and one more than a chunk, one workgroup of chunks plus one, two plus three (tests/bwd_kernels.py).
    Batches that short run the small-batch instantiation of the fp64 wave launcher (one-wave workgroups, quarter chunks);
    the tuned rows of csrc/wave_table.h, which the benchmark runs, start at two workgroups per CU, so every fp64 wave order
    is also run at that size plus a ragged tail ("wave-tuned"), and so are the persistent 2D 4x4x4 grids at 131 101
    elements and the 2D 4x4x4 kernels with one tensor for both bases -- against fp64 sweeps in slices where long double
    would be too slow, bound f64_factor gamma_N absref64;
(b) `in` and every basis as views between NaN bands, `out` between guard words, at 16-byte-multiple offsets inside a
    128-byte line (odd scalar offsets for the kernels that take 8-byte-aligned buffers), with a partial last chunk: the
    matrix-core kernels feed their padding rows and columns clamped data times a zero basis, so a clamp that leaves the
    view is invisible on finite neighbours and a NaN here;
(c) element isolation: all coefficients of the first, the last and one interior element are NaN; every other element's
    output is bit-identical to the launch on the clean input, every output of a poisoned element is NaN.
(b) and (c) take the tuned wave rows and the one-basis 2D 4x4x4 kernels as cases of their own.

Each case prints max |err| / (gamma_N absref); `pytest -s` shows them, and the worst per kernel and precision at the end.
"""
import collections
import concurrent.futures

import numpy as np
import pytest

import bwd_kernels as bk
from bwd_ref import bwd_excess, bwd_f64, bwd_f64_factor, ref_bwdtrans, unit_roundoff
from test_gpu_parity import RT_SHAPES, TRIPLES

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)      # (kernel, dtype) -> worst excess of this run


@pytest.fixture(scope="module")
def sf():
    import __graft_entry__ as ge
    yield ge.load_package()
    for (kernel, dtype_name), q in sorted(WORST.items()):
        print(f"\nworst {kernel} {dtype_name}: max |err| / (its bound) = {q:.3g}", end="")
    print()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a GPU"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _sizes(nq):
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def _bases(sf, torch_mod, nq, dtype_name, seed):
    """Distinct bases per direction."""
    return [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=getattr(torch_mod, dtype_name)) for d, q in enumerate(nq)]


def _run(sf, nq, bs, x, variant, out=None):
    """One launch by name.  "mfma4-lds" / "mfma4-direct": the 3D 4x4x4 kernel with its output path named."""
    if variant in ("mfma4-lds", "mfma4-direct"):
        return sf.bwdtrans_hex_mfma4(nq[0], *bs, x, variant == "mfma4-direct", out=out)
    return (sf.bwdtrans_hex if len(nq) == 3 else sf.bwdtrans_quad)(tuple(nq), *bs, x, out=out, variant=variant)


def _note(kernel, dtype_name, q):
    WORST[(kernel, dtype_name)] = max(WORST[(kernel, dtype_name)], q)


STEP = 4096                                 # elements per slice of the fp64 reference of a long batch


class Batch:
    """Seeded data of one shape at its largest count, with the long-double reference computed once: the operands are
    element-major, so the first n elements are a problem of n elements.  shared: one tensor for both directions of a 2D
    shape (the 2D 4x4x4 launcher then runs its one-basis-copy instantiation).  long: a batch too long for long double --
    excess() then compares with fp64 sweeps in slices of STEP elements, bound f64_factor gamma_N absref64."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed, shared=False, long=False):
        self.nq, self.nelmt, self.dtype_name, self.long = tuple(nq), nelmt, dtype_name, long
        self.nmt, self.nqt = _sizes(nq)
        self.bs = _bases(sf, torch_mod, nq, dtype_name, seed)
        if shared:
            self.bs = [self.bs[0]] * len(nq)
        self.x = sf.fill_random(nelmt * self.nmt, 10 + seed, dtype=getattr(torch_mod, dtype_name))
        self.bh, self.xh = [_np(b) for b in self.bs], _np(self.x)
        if not long:
            self.ref, self.absref = ref_bwdtrans(nq, nelmt, self.bh, self.xh)

    @property
    def bound(self):
        return "f64_factor gamma_N absref64" if self.long else "gamma_N absref"

    def excess(self, got, n):
        u, gh = unit_roundoff(self.dtype_name), _np(got)
        if not self.long:
            return bwd_excess(gh, self.ref[:n * self.nqt], self.absref[:n * self.nqt], self.nq, u)
        factor = bwd_f64_factor(self.nq, u)

        def one(lo):
            m = min(STEP, n - lo)
            ref, absref = bwd_f64(self.nq, m, self.bh, self.xh[lo * self.nmt:(lo + m) * self.nmt])
            return bwd_excess(gh[lo * self.nqt:(lo + m) * self.nqt], ref, absref, self.nq, u, factor=factor)

        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            return max(pool.map(one, range(0, n, STEP)))

    def check(self, sf, torch_mod, variant, kernel, counts):
        for n in counts:
            got = _run(sf, self.nq, self.bs, self.x[:n * self.nmt], variant)
            torch_mod.cuda.synchronize()
            q = self.excess(got, n)
            _note(kernel, self.dtype_name, q)
            print(f"{kernel} {variant} {_ids(self.nq)} {self.dtype_name} nelmt={n}: max |err| / ({self.bound}) = {q:.3g}")
            assert q <= 1.0, (kernel, variant, self.nq, self.dtype_name, n, q)


def _elementwise(sf, torch_mod, nq, variants, rows, dtype_name="float64", kernel=None, seed=1, shared=False):
    counts = bk.ragged_counts(rows)
    batch = Batch(sf, torch_mod, nq, counts[-1], dtype_name, seed, shared=shared)
    for variant in variants:
        batch.check(sf, torch_mod, variant, kernel or variant, counts)


# ---- (a) every kernel by name, elementwise ------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", range(2, 12))
def test_hex_wave_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, (nq,) * 3, ["wave"], bk.wave_rows(3, nq, "float64"), seed=nq)


@pytest.mark.parametrize("nq", list(range(2, 25)) + [32])
def test_quad_wave_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, (nq, nq), ["wave"], bk.wave_rows(2, nq, "float64"), seed=nq)


def _tuned_count(sf, dim, nq):
    """The fp64 wave launcher runs the row of csrc/wave_table.h -- its EC, several waves per workgroup, XCD runs, the
    line-aligned lanes -- only from two workgroups per CU up (bk.tuned_from), and one-wave workgroups of quarter chunks
    below.  This count is that threshold, one workgroup more, and a partial last chunk (EC - 1 elements, or one)."""
    ec, wpb = bk.wave_rows(dim, nq, "float64")[0]
    return bk.tuned_from(dim, nq, sf.device_info()["num_cu"]) + ec * wpb * bk.wave_km(dim, nq) + max(1, ec - 1)


TUNED = [(3, n) for n in range(3, 12)] + [(2, n) for n in list(range(3, 25)) + [32]]     # nq = 2: stream kernels, one shape


@pytest.mark.parametrize("dim,nq", TUNED, ids=[f"{d}d-nq{n}" for d, n in TUNED])
def test_wave_tuned_rows_elementwise(sf, torch_mod, dim, nq):
    """The wave kernels as the benchmark runs them: the tuned instantiation of every fp64 order, at the first batch size
    that reaches it plus a ragged tail (2 065 elements at 3D nq 11, 86 225 at 2D nq 3)."""
    nelmt = _tuned_count(sf, dim, nq)
    batch = Batch(sf, torch_mod, (nq,) * dim, nelmt, "float64", nq, long=True)
    batch.check(sf, torch_mod, "wave", "wave-tuned", [nelmt])


@pytest.mark.parametrize("nq", TRIPLES, ids=_ids)
def test_hex_anisotropic_triples_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, nq, ["wave"], [bk.triple_row(nq)], kernel="wave-triple", seed=sum(nq))


@pytest.mark.parametrize("nq", RT_SHAPES, ids=_ids)
def test_hex_runtime_extents_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, nq, ["wave-rt"], [bk.rt_row(nq)], seed=sum(nq))


@pytest.mark.parametrize("nq", range(11, 33))
def test_quad_mfma_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, (nq, nq), ["mfma"], [bk.quad_mfma_row(nq)], seed=nq)


@pytest.mark.parametrize("nq", range(4, 17))
def test_hex_mfma_elementwise(sf, torch_mod, nq):
    _elementwise(sf, torch_mod, (nq,) * 3, ["mfma"], [bk.hex_mfma_row(nq)], seed=nq)


@pytest.mark.parametrize("nq", range(8, 33))
def test_quad_mfma4_elementwise(sf, torch_mod, nq):
    """Distinct bases, then one tensor for both directions: the launcher then runs the instantiation that keeps one copy
    of the basis in LDS (what the benchmark's isotropic calls run)."""
    _elementwise(sf, torch_mod, (nq, nq), ["mfma4"], [bk.quad_mfma4_row(nq)], seed=nq)
    _elementwise(sf, torch_mod, (nq, nq), ["mfma4"], [bk.quad_mfma4_row(nq)], kernel="mfma4-shared-basis", seed=nq,
                 shared=True)


@pytest.mark.parametrize("nq", range(12, 17))
def test_hex_mfma4_elementwise(sf, torch_mod, nq):
    """Both output paths by name, and the one SF_VARIANT_MFMA4 picks."""
    rows = [bk.hex_mfma4_row(nq, False), bk.hex_mfma4_row(nq, True)]
    _elementwise(sf, torch_mod, (nq,) * 3, ["mfma4-lds", "mfma4-direct", "mfma4"], rows, kernel="hex-mfma4", seed=nq)


@pytest.mark.parametrize("nq", [26, 28])
@pytest.mark.parametrize("shared", [False, True], ids=["distinct", "shared-basis"])
def test_quad_mfma4_persistent_grid_elementwise(sf, torch_mod, nq, shared):
    """The persistent 2D 4x4x4 kernels draw batches of chunks from a device-wide counter, two tickets up front per wave:
    131 101 elements are 16 388 batches of 4 two-element chunks at nq 28 and 4 097 batches of 8 four-element chunks at
    nq 26, against about 2 048 initial tickets, so waves redeem tickets issued inside their loop.  With distinct bases
    (the two-basis-copy instantiation) and with one tensor for both directions."""
    nelmt = 131101
    batch = Batch(sf, torch_mod, (nq, nq), nelmt, "float64", nq, shared=shared, long=True)
    batch.check(sf, torch_mod, "mfma4", "mfma4-persistent" + ("-shared-basis" if shared else ""), [nelmt])


BASELINE = ["thread", "block-lds", "block-glb", "generic"]
BASELINE_SHAPES = [(2, 2, 2), (4, 4, 4), (8, 8, 8), (3, 5, 4), (8, 2, 6), (10, 10, 10), (12, 12, 12),
                   (2, 2), (8, 8), (4, 9), (16, 3), (20, 20), (32, 32), (40, 40)]


@pytest.mark.parametrize("nq", BASELINE_SHAPES, ids=_ids)
def test_baseline_variants_elementwise(sf, torch_mod, nq):
    """thread (a workgroup of 128 elements), block-lds, block-glb and generic (a workgroup per element; 37 elements as
    well), one reference per shape."""
    counts = sorted(set(bk.ragged_counts([bk.THREAD_ROW, bk.BLOCK_ROW])) | {37})
    batch = Batch(sf, torch_mod, nq, counts[-1], "float64", sum(nq))
    for variant in BASELINE:
        batch.check(sf, torch_mod, variant, variant, counts)


@pytest.mark.parametrize("nq", [(17, 17, 17), (22, 22, 22), (33, 33), (100, 3)], ids=_ids)
def test_generic_above_the_tables_elementwise(sf, torch_mod, nq):
    """The any-extent kernels where nothing else is built: LDS-resident at (17,17,17), the library's scratch from
    (22,22,22) (one element's images exceed the LDS), 2D beyond nq 32 and with a one-pencil direction."""
    batch = Batch(sf, torch_mod, nq, 7, "float64", sum(nq))
    for variant in ("generic", "auto"):
        batch.check(sf, torch_mod, variant, "generic", (1, 2, 7))


def test_interleaved_layout_elementwise(sf, torch_mod):
    """The thread-per-element kernel on the wave-64 interleaved layout: 131 elements are two full groups and a ragged one."""
    nq, nelmt = (3, 5, 4), 131
    batch = Batch(sf, torch_mod, nq, nelmt, "float64", 5)
    x_il = sf.interleave64(batch.x, nelmt, batch.nmt)
    out_il = sf.bwdtrans_hex_interleaved(nq, *batch.bs, x_il, nelmt)
    got = sf.interleave64(out_il, nelmt, batch.nqt, inverse=True)
    torch_mod.cuda.synchronize()
    q = batch.excess(got, nelmt)
    _note("interleaved", "float64", q)
    print(f"interleaved {_ids(nq)} nelmt={nelmt}: max |err| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0


F32_AUTO = [(3, n) for n in range(2, 17)] + [(2, n) for n in range(2, 33)]


@pytest.mark.parametrize("dim,nq", F32_AUTO, ids=[f"{d}d-nq{n}" for d, n in F32_AUTO])
def test_fp32_auto_elementwise(sf, torch_mod, dim, nq):
    """T = float has the AUTO route only: the fp32 wave rows, and the v_mfma_f32_16x16x4_f32 kernels at 3D nq 13..16 and
    2D nq 25..32."""
    kernel, rows = bk.f32_auto_rows(dim, nq)
    _elementwise(sf, torch_mod, (nq,) * dim, ["auto"], rows, "float32", kernel=kernel, seed=nq)


# ---- (b), (c): the kernels that pack tiles, chunks or slabs ---------------------------------------------------------------
# kernel, shape, variant, (EC, WPB), scalar-aligned views (else 16-byte multiples), fp32 AUTO runs the same kernel, one tensor
# for both bases, the batch that reaches the tuned fp64 wave row (_tuned_count) instead of short ones
Packed = collections.namedtuple("Packed", "kernel nq variant row scalar f32 shared tuned", defaults=(False, False))


def _packed():
    cases = []
    for nq in (11, 13, 17, 30, 32):
        cases.append(Packed("mfma", (nq, nq), "mfma", bk.quad_mfma_row(nq), False, nq >= bk.QUAD_F32_MFMA_FROM))
    for nq in (8, 10, 22, 27, 31):
        cases.append(Packed("mfma4", (nq, nq), "mfma4", bk.quad_mfma4_row(nq), False, False))
        cases.append(Packed("mfma4-shared-basis", (nq, nq), "mfma4", bk.quad_mfma4_row(nq), False, False, shared=True))
    for nq in (4, 6, 13, 15):
        cases.append(Packed("mfma", (nq,) * 3, "mfma", bk.hex_mfma_row(nq), False, nq >= bk.HEX_F32_MFMA_FROM))
    for nq in (12, 13, 16):
        cases.append(Packed("hex-mfma4", (nq,) * 3, "mfma4-lds", bk.hex_mfma4_row(nq, False), False, False))
        cases.append(Packed("hex-mfma4", (nq,) * 3, "mfma4-direct", bk.hex_mfma4_row(nq, True), False, False))
    for dim, nq in ((3, 3), (3, 8), (2, 7), (2, 16)):
        row = bk.wave_rows(dim, nq, "float64")[0]
        cases.append(Packed("wave", (nq,) * dim, "wave", row, False, True))
        cases.append(Packed("wave-tuned", (nq,) * dim, "wave", row, False, False, tuned=True))
    cases.append(Packed("wave-rt", (3, 5, 4), "wave-rt", bk.rt_row((3, 5, 4)), True, False))
    cases.append(Packed("generic", (5, 9, 13), "generic", bk.BLOCK_ROW, True, True))
    return cases


def _f32_row(case):
    """The row of the kernel fp32 AUTO runs for a case with f32 set."""
    if case.kernel == "generic":
        return bk.BLOCK_ROW
    return bk.f32_auto_rows(len(case.nq), case.nq[0])[1][0]


PACKED = [(c, "float64") for c in _packed()] + [(c, "float32") for c in _packed() if c.f32]
PACKED_IDS = [f"{c.kernel}-{c.variant}-{_ids(c.nq)}-{d}" for c, d in PACKED]


def _row_of(case, dtype_name):
    return case.row if dtype_name == "float64" else _f32_row(case)


def _variant_of(sf, torch_mod, case, dtype_name):
    """T = float has the AUTO route only.  For (5,9,13) AUTO ends in the any-extent kernel because nothing before it takes
    the shape: the order tables and the triples are isotropic / fp64, the run-time-extent kernel is fp64 and stops at
    extent 8 -- and no specialisation of the shape may be ready, which is looked at here."""
    if dtype_name == "float64":
        return case.variant
    if case.kernel == "generic":
        assert sf.specialisation_state(case.nq, dtype=torch_mod.float32)[0] != 1, "AUTO would run the specialisation"
    return "auto"


def _round_up(n, m):
    return (n + m - 1) // m * m


def _between(torch_mod, data, off, band, fill):
    """`data` as a view at `off` scalars past a 128-byte line, inside an allocation that holds `fill` on both sides."""
    n = data.numel()
    buf = torch_mod.full((band + off + n + band,), fill, dtype=data.dtype, device=data.device)
    buf[band + off:band + off + n] = data
    return buf, buf[band + off:band + off + n]


def _sides(buf, view_numel, off, band):
    return buf[:band + off], buf[band + off + view_numel:]


@pytest.mark.parametrize("case,dtype_name", PACKED, ids=PACKED_IDS)
def test_nan_bands_and_guards(sf, torch_mod, case, dtype_name):
    """`in` and every basis between NaN bands, `out` between guard words, a partial last chunk.  A band is at least one
    chunk (one basis) long, so a gather clamped by a row, into the next element or past a ragged chunk's end lands in it.
    Why NaN: the matrix-core kernels multiply their padding by an exact zero, so a wrong clamp gives the right bits on
    finite neighbours (0 * finite = 0, s + 0 = s) and a NaN only here (0 * NaN = NaN)."""
    nq, (ec, wpb) = case.nq, _row_of(case, dtype_name)
    variant, dtype = _variant_of(sf, torch_mod, case, dtype_name), getattr(torch_mod, dtype_name)
    nmt, nqt = _sizes(nq)
    vec = 16 // (8 if dtype_name == "float64" else 4)             # scalars per 16 bytes
    line = 8 * vec                                                # scalars per 128-byte line
    # (elements, offset of in, offset of out, offsets of the bases), offsets in 16-byte units -- or, for the kernels that
    # take scalar-aligned buffers, in scalars and odd
    tail = ec - 1 if ec > 1 else 0
    layouts = [(ec * (wpb + 1) + tail, 1, 0, (3, 5, 7)), (2 * ec * wpb + 1, 3, 2, (1, 0, 6)), (ec + 1, 5, 7, (2, 4, 1)),
               (ec * wpb + 1 + tail, 0, 4, (7, 3, 0)), (3 * ec * wpb + 2 + tail, 6, 1, (5, 6, 2))]
    if case.tuned:
        layouts = [(_tuned_count(sf, len(nq), nq[0]), 3, 6, (5, 2, 7))]
    unit = 1 if case.scalar else vec
    batch = Batch(sf, torch_mod, nq, max(n for n, *_ in layouts), dtype_name, 3, shared=case.shared, long=case.tuned)
    for n, off_in, off_out, off_bs in layouts:
        if case.scalar:
            off_in, off_out, off_bs = 2 * off_in + 1, 2 * off_out + 1, [2 * o + 1 for o in off_bs]
        band_x = _round_up(max(64, ec * nmt), line)
        xbuf, x = _between(torch_mod, batch.x[:n * nmt], unit * off_in, band_x, float("nan"))
        if case.shared:                                           # one view, handed over for both directions
            off_bs = [off_bs[0]] * len(nq)
        based = [_between(torch_mod, b, unit * o, _round_up(max(64, b.numel()), line), float("nan"))
                 for b, o in zip(batch.bs, off_bs)]
        if case.shared:
            based = [based[0]] * len(nq)
        guard = _round_up(max(64, ec * nqt), line)
        obuf, out = _between(torch_mod, torch_mod.zeros(n * nqt, dtype=dtype, device="cuda"), unit * off_out, guard, -7.0)
        _run(sf, nq, [v for _, v in based], x, variant, out=out)
        torch_mod.cuda.synchronize()
        where = (case.kernel, variant, nq, dtype_name, n, off_in, off_out)
        assert bool(torch_mod.isfinite(out).all()), where
        q = batch.excess(out, n)
        _note(case.kernel + " between NaN bands", dtype_name, q)
        print(f"NaN bands {case.kernel} {variant} {_ids(nq)} {dtype_name} nelmt={n} in+{unit * off_in} out+{unit * off_out}: "
              f"max |err| / ({batch.bound}) = {q:.3g}")
        assert q <= 1.0, where + (q,)
        for buf, numel, off, band in ([(xbuf, n * nmt, unit * off_in, band_x)]
                                      + [(bb, b.numel(), unit * o, _round_up(max(64, b.numel()), line))
                                         for (bb, _), b, o in zip(based, batch.bs, off_bs)]):
            assert all(bool(torch_mod.isnan(s).all()) for s in _sides(buf, numel, off, band)), where
        assert torch_mod.equal(x, batch.x[:n * nmt]), where
        assert all(bool((s == -7.0).all()) for s in _sides(obuf, n * nqt, unit * off_out, guard)), where


@pytest.mark.parametrize("case,dtype_name", PACKED, ids=PACKED_IDS)
def test_a_poisoned_element_stays_in_its_element(sf, torch_mod, case, dtype_name):
    """2 EC WPB + 3 elements; the first, the last and one interior element hold NaN in every coefficient.  The interior one
    sits in the second chunk (the third where a chunk is one element), whose other elements are healthy, at every position
    of the chunk in turn.  The bases are dense and random, so every output of a poisoned element is NaN; every other
    element's output has the bits of the launch on the clean input.  No reference is needed.  A tuned wave case takes the
    batch that reaches the tuned row, and its interior element from a chunk in the middle of the batch."""
    nq, (ec, wpb) = case.nq, _row_of(case, dtype_name)
    variant, dtype = _variant_of(sf, torch_mod, case, dtype_name), getattr(torch_mod, dtype_name)
    nmt, nqt = _sizes(nq)
    nelmt = _tuned_count(sf, len(nq), nq[0]) if case.tuned else 2 * ec * wpb + 3
    first = (nelmt // 2) // ec * ec if case.tuned else max(2, ec)
    bs = _bases(sf, torch_mod, nq, dtype_name, 4)
    if case.shared:
        bs = [bs[0]] * len(nq)
    x = sf.fill_random(nelmt * nmt, 14, dtype=dtype)
    clean = _run(sf, nq, bs, x, variant).view(nelmt, nqt)
    torch_mod.cuda.synchronize()
    assert bool(torch_mod.isfinite(clean).all()) and float(clean.abs().max()) > 0
    for pos in range(ec):
        sick = [0, first + pos, nelmt - 1]
        assert 1 < sick[1] < sick[2] - 1
        xp = x.clone().view(nelmt, nmt)
        xp[sick] = float("nan")
        got = _run(sf, nq, bs, xp.view(-1), variant).view(nelmt, nqt)
        torch_mod.cuda.synchronize()
        well = torch_mod.ones(nelmt, dtype=torch_mod.bool, device="cuda")
        well[sick] = False
        where = (case.kernel, variant, nq, dtype_name, pos)
        assert torch_mod.equal(got[well], clean[well]), where + (
            (well & (got != clean).any(dim=1)).nonzero().view(-1).tolist()[:20],)
        assert bool(torch_mod.isnan(got[sick]).all()), where
