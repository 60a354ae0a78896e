"""GPU tests of the gather-scatter calls (include/sumfact.h sf_gs_setup, sf_global_to_local_*, sf_assemble_*, sf_gs_*):
structured meshes, random maps (empty rows, negative entries, a long row), the scan's tile boundaries, operands at scalar
offsets between NaN bands, the setup's determinism and its refusal of an entry out of range, run-to-run reproducibility,
stream capture, two streams, four host threads on one stream, and the assembled Helmholtz operator and its diagonal.

Reference: tests/gs_ref.py.  The summation order is specified (ascending local index, one rounding per addition) and
sign * x is exact, so every comparison is np.array_equal unless stated.  Data: sf.fill_random, seeded.

The end-to-end bound (derived, not measured): a global entry is the computed sum of the v contributions of its row, each
of which carries its family's own elementwise bound b_i = gamma_N absref_i (tests/helm_ref.py, tests/diag_ref.py):
    |got - ref| <= sum_i b_i + gamma_{v-1} sum_i (|ref_i| + b_i)
-- the first term the contributions' errors, assembled with |Q|^T, the second the v - 1 additions of the row on the
computed contributions (|computed_i| <= |ref_i| + b_i).  A zero bound needs a zero error.
"""
import ctypes
import threading

import numpy as np
import pytest

from diag_ref import diag_n, ref_diag
from gs_ref import (multiplicity, random_map, random_sign, ref_assemble, ref_global_to_local, ref_gs, shared,
                    structured_map)
from helm_ref import COMPONENTS, dense_operator, gamma, helm_n, unit_roundoff

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
SCAN_TILE = 2048            # csrc/gs.hip kScanTile: 256 lanes x 8 counts
MESHES = [((3, 2), 3), ((2, 2, 2), 3), ((17, 5), 7)]
RANDOM_NLOCAL = [1, 2, 3, 63, 64, 65, 255, 257, 1001, 100003]


@pytest.fixture(scope="module")
def sf():
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a GPU"
    return torch


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _values(sf, torch, n, seed, dtype_name):
    return sf.fill_random(n, seed, dtype=getattr(torch, dtype_name))


def check_all_three(sf, torch, l2g, nglobal, dtype_name, seed, signed, what):
    """global_to_local, assemble and gs of one map against the references, bit for bit."""
    nlocal = l2g.size
    gsmap = sf.gs_setup(_dev(torch, l2g), nglobal)
    sign = random_sign(nlocal, seed + 1, dtype_name) if signed else None
    sign_d = None if sign is None else _dev(torch, sign)
    loc = _values(sf, torch, nlocal, seed + 2, dtype_name)
    glo = _values(sf, torch, nglobal, seed + 3, dtype_name)
    loc_h, glo_h = _np(loc), _np(glo)
    got_l = sf.global_to_local(gsmap, glo, sign=sign_d)
    got_g = sf.assemble(gsmap, loc, sign=sign_d)
    work = loc.clone()
    assert sf.gs(gsmap, work, sign=sign_d) is work
    torch.cuda.synchronize()
    assert np.array_equal(_np(got_l), ref_global_to_local(l2g, glo_h, sign)), (what, "global_to_local")
    assert np.array_equal(_np(got_g), ref_assemble(l2g, nglobal, loc_h, sign)), (what, "assemble")
    assert np.array_equal(_np(work), ref_gs(l2g, nglobal, loc_h, sign)), (what, "gs")
    keep = ~shared(l2g, nglobal)                    # unmapped or alone on their row: the same bits as before
    assert np.array_equal(_np(work)[keep].view(np.uint8), loc_h[keep].view(np.uint8)), (what, "gs untouched")
    return gsmap


@pytest.mark.parametrize("signed", [False, True], ids=["plain", "signed"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("nel,nm", MESHES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"nm{v}")
def test_structured_meshes(sf, torch_mod, nel, nm, dtype_name, signed):
    l2g, nglobal = structured_map(nel, nm)
    assert multiplicity(l2g, nglobal).max() == 2 ** len(nel)
    check_all_three(sf, torch_mod, l2g, nglobal, dtype_name, 10 * nm + len(nel), signed, (nel, nm))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("nlocal", RANDOM_NLOCAL)
def test_random_maps(sf, torch_mod, nlocal, dtype_name):
    """nglobal about a third of nlocal, a fifth of the rows empty, 5 % negative entries, signs; at 100 003 one row of
    1024 entries and more."""
    nglobal = max(1, nlocal // 3)
    long_row = 1024 if nlocal >= 4096 else 0
    l2g = random_map(nlocal, nglobal, nlocal, empty_share=0.2, negative_share=0.05, long_row=long_row)
    if long_row:
        assert multiplicity(l2g, nglobal).max() >= 1024
    if nlocal >= 63:
        m = multiplicity(l2g, nglobal)
        assert (m == 0).any() and (m > 1).any() and (l2g < 0).any()
    check_all_three(sf, torch_mod, l2g, nglobal, dtype_name, nlocal, True, nlocal)
    check_all_three(sf, torch_mod, l2g, nglobal, dtype_name, nlocal + 7, False, nlocal)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_all_negative_map_and_one_global(sf, torch_mod, dtype_name):
    check_all_three(sf, torch_mod, np.full(1001, -1, dtype=np.int32), 77, dtype_name, 5, True, "all negative")
    l2g = random_map(1001, 1, 9, negative_share=0.05)
    assert (l2g == 0).sum() > 900
    check_all_three(sf, torch_mod, l2g, 1, dtype_name, 6, True, "nglobal 1")


@pytest.mark.parametrize("nglobal", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE ** 2 + 1],
                         ids=["B-1", "B", "B+1", "B^2+1"])
def test_scan_tile_boundaries(sf, torch_mod, nglobal):
    """One tile that is not full, exactly one, one and a word, and one more than a full step of the scan over the tile
    sums (B^2 + 1 = 4 194 305 >= 2^22 global degrees of freedom): every row begin comes out of the scan."""
    assert 2 ** 22 <= SCAN_TILE ** 2 + 1 < 2 ** 23
    nlocal = nglobal + nglobal // 4
    l2g = random_map(nlocal, nglobal, nglobal % 1000, empty_share=0.1, negative_share=0.02)
    l2g[-1], l2g[0] = nglobal - 1, nglobal - 1      # the last row is in use
    torch = torch_mod
    gsmap = sf.gs_setup(_dev(torch, l2g), nglobal)
    loc = _values(sf, torch, nlocal, 3, "float64")
    got = sf.assemble(gsmap, loc)
    work = loc.clone()
    sf.gs(gsmap, work)
    torch.cuda.synchronize()
    want = ref_assemble(l2g, nglobal, _np(loc))
    assert np.array_equal(_np(got), want)
    assert np.array_equal(_np(work), np.where(shared(l2g, nglobal), ref_global_to_local(l2g, want), _np(loc)))


def _banded(torch, a, off, pad=8):
    """(allocation, view): the values of `a` starting `off` scalars into an allocation whose other entries are NaN (the
    smallest int32 for an index array)."""
    t = _dev(torch, a)
    guard = float("nan") if t.is_floating_point() else -2 ** 31
    buf = torch.full((t.numel() + pad,), guard, dtype=t.dtype, device="cuda")
    buf[off:off + t.numel()] = t
    return buf, buf[off:off + t.numel()]


def _bands_intact(buf, off, n):
    rest = np.concatenate([_np(buf[:off]), _np(buf[off + n:])])
    return bool(np.all(np.isnan(rest))) if rest.dtype.kind == "f" else bool(np.all(rest == -2 ** 31))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("map_off,val_off", [(1, 1), (3, 3), (1, 3), (3, 1), (0, 1), (2, 0)],
                         ids=lambda v: f"+{v}")
def test_operands_at_scalar_offsets_between_nan_bands(sf, torch_mod, map_off, val_off, dtype_name):
    """Every operand a view that starts `map_off` (the int32 arrays) or `val_off` (the values, the sign) scalars into its
    allocation, with equal and with unequal 16-byte phases.  The allocations are NaN outside the views, and stay so."""
    torch = torch_mod
    nlocal, nglobal = 1001, 333
    l2g = random_map(nlocal, nglobal, 12, empty_share=0.2, negative_share=0.05)
    sign = random_sign(nlocal, 13, dtype_name)
    l2g_b, l2g_v = _banded(torch, l2g, map_off)
    rows_b, rows_v = _banded(torch, np.zeros(nglobal, dtype=np.int32), map_off)
    perm_b, perm_v = _banded(torch, np.zeros(nlocal, dtype=np.int32), map_off)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = sf.capi.lib().sf_gs_setup(nlocal, nglobal, ptr(l2g_v), ptr(rows_v), ptr(perm_v),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    gsmap = sf.GsMap(l2g_v, rows_v, perm_v, nlocal, nglobal)
    assert _bands_intact(rows_b, map_off, nglobal) and _bands_intact(perm_b, map_off, nlocal)
    assert _bands_intact(l2g_b, map_off, nlocal)
    loc_h, glo_h = _np(_values(sf, torch, nlocal, 14, dtype_name)), _np(_values(sf, torch, nglobal, 15, dtype_name))
    sign_b, sign_v = _banded(torch, sign, val_off)
    loc_b, loc_v = _banded(torch, loc_h, val_off)
    glo_b, glo_v = _banded(torch, glo_h, val_off)
    outl_b, outl_v = _banded(torch, np.zeros_like(loc_h), val_off)
    outg_b, outg_v = _banded(torch, np.zeros_like(glo_h), val_off)
    for s_v, s_h in ((sign_v, sign), (None, None)):
        sf.global_to_local(gsmap, glo_v, sign=s_v, out=outl_v)
        sf.assemble(gsmap, loc_v, sign=s_v, out=outg_v)
        work_b, work_v = _banded(torch, loc_h, val_off)
        sf.gs(gsmap, work_v, sign=s_v)
        torch.cuda.synchronize()
        assert np.array_equal(_np(outl_v), ref_global_to_local(l2g, glo_h, s_h))
        assert np.array_equal(_np(outg_v), ref_assemble(l2g, nglobal, loc_h, s_h))
        assert np.array_equal(_np(work_v), ref_gs(l2g, nglobal, loc_h, s_h))
        for buf, n in ((outl_b, nlocal), (outg_b, nglobal), (work_b, nlocal), (loc_b, nlocal), (glo_b, nglobal),
                       (sign_b, nlocal)):
            assert _bands_intact(buf, val_off, n)
        keep = ~shared(l2g, nglobal)
        assert np.array_equal(_np(work_v)[keep].view(np.uint8), loc_h[keep].view(np.uint8))


def test_setup_is_deterministic_and_refuses_an_entry_out_of_range(sf, torch_mod):
    torch = torch_mod
    nlocal, nglobal = 100003, 33334
    l2g = random_map(nlocal, nglobal, 21, empty_share=0.2, negative_share=0.05, long_row=1024)
    a, b = sf.gs_setup(_dev(torch, l2g), nglobal), sf.gs_setup(_dev(torch, l2g), nglobal)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.perm, b.perm)
    bad = l2g.copy()
    bad[nlocal // 2] = nglobal
    with pytest.raises(sf.capi.SumfactError) as e:
        sf.gs_setup(_dev(torch, bad), nglobal)
    assert e.value.rc == sf.capi.SF_EINVAL
    bad[nlocal // 2] = 2 ** 31 - 1
    with pytest.raises(sf.capi.SumfactError) as e:
        sf.gs_setup(_dev(torch, bad), nglobal)
    assert e.value.rc == sf.capi.SF_EINVAL
    # the refusals left the library usable
    check_all_three(sf, torch, l2g, nglobal, "float64", 22, True, "after refusal")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_assemble_five_runs_identical(sf, torch_mod, dtype_name):
    torch = torch_mod
    l2g, nglobal = structured_map((17, 5), 7)
    gsmap = sf.gs_setup(_dev(torch, l2g), nglobal)
    loc = _values(sf, torch, l2g.size, 31, dtype_name)
    outs = [sf.assemble(gsmap, loc) for _ in range(5)]
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert np.array_equal(_np(outs[0]), ref_assemble(l2g, nglobal, _np(loc)))


def test_stream_capture_replayed_on_changed_inputs(sf, torch_mod):
    """The three apply calls captured as one linear chain (global_to_local -> gs -> assemble), replayed twice, each time
    on new inputs in the captured buffers."""
    torch = torch_mod
    l2g, nglobal = structured_map((2, 2, 2), 3)
    nlocal = l2g.size
    gsmap = sf.gs_setup(_dev(torch, l2g), nglobal)
    sign = random_sign(nlocal, 41, np.float64)
    sign_d = _dev(torch, sign)
    glo = torch.zeros(nglobal, dtype=torch.float64, device="cuda")
    loc = torch.zeros(nlocal, dtype=torch.float64, device="cuda")
    out = torch.zeros(nglobal, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            sf.global_to_local(gsmap, glo, sign=sign_d, out=loc, stream=side)
            sf.gs(gsmap, loc, sign=sign_d, stream=side)
            sf.assemble(gsmap, loc, sign=sign_d, out=out, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (51, 52):
        x = sf.fill_random(nglobal, seed)
        glo.copy_(x)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        l = ref_gs(l2g, nglobal, ref_global_to_local(l2g, _np(x), sign), sign)
        assert np.array_equal(_np(loc), l)
        assert np.array_equal(_np(out), ref_assemble(l2g, nglobal, l, sign))
        assert float(out.abs().max()) > 0


def test_two_streams_in_flight(sf, torch_mod):
    torch = torch_mod
    jobs = [structured_map((17, 5), 7), (random_map(100003, 33334, 61, 0.2, 0.05), 33334)]
    maps = [sf.gs_setup(_dev(torch, l2g), ng) for l2g, ng in jobs]
    locs = [sf.fill_random(l2g.size, 62 + k) for k, (l2g, _) in enumerate(jobs)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for m, x, st in zip(maps, locs, streams):
        with torch.cuda.stream(st):
            g = sf.assemble(m, x, stream=st)
            outs.append((g, sf.global_to_local(m, g, stream=st)))
    torch.cuda.synchronize()
    for (l2g, ng), x, (g, l) in zip(jobs, locs, outs):
        want = ref_assemble(l2g, ng, _np(x))
        assert np.array_equal(_np(g), want) and np.array_equal(_np(l), ref_global_to_local(l2g, want))


def test_four_host_threads_on_one_stream(sf, torch_mod):
    """Four threads call the raw C entry points on ONE stream, arguments marshalled beforehand (the calls release the GIL,
    so the threads are inside the library together), each thread its own map and one output per launch: every output
    equals the reference, bit for bit."""
    torch = torch_mod
    jobs = [structured_map((17, 5), 7), structured_map((2, 2, 2), 3), (random_map(100003, 33334, 71, 0.2, 0.05), 33334),
            (random_map(1001, 333, 72, 0.2, 0.05), 333)]
    launches, timeout = 12, 120
    st = torch.cuda.Stream()
    lib = sf.capi.lib()
    handle = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    maps = [sf.gs_setup(_dev(torch, l2g), ng) for l2g, ng in jobs]
    locs = [sf.fill_random(l2g.size, 73 + k) for k, (l2g, _) in enumerate(jobs)]
    outs, calls = [], []
    for m, x in zip(maps, locs):
        stride = (m.nglobal + 31) // 32 * 32
        o = torch.full((launches, stride), float("nan"), dtype=torch.float64, device="cuda")
        outs.append(o[:, :m.nglobal])
        calls.append([(lib.sf_assemble_f64, (m.nglobal, ptr(m.rows), ptr(m.perm), None, ptr(x), ptr(o[k]), handle))
                      for k in range(launches)])
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(jobs))
    errors = [None] * len(jobs)

    def body(i):
        try:
            barrier.wait(timeout=timeout)
            for fn, args in calls[i]:
                rc = fn(*args)
                assert rc == 0, rc
        except BaseException as e:      # noqa: B036 -- handed to the main thread below
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not [i for i, t in enumerate(threads) if t.is_alive()]
    for e in errors:
        if e is not None:
            raise e
    torch.cuda.synchronize()
    for (l2g, ng), x, o in zip(jobs, locs, outs):
        want = ref_assemble(l2g, ng, _np(x))
        for k in range(launches):
            assert np.array_equal(_np(o[k]), want), k


# ---- end to end: the assembled Helmholtz operator and its diagonal ------------------------------------------------------
LAM = 0.75


class Assembled:
    """Seeded operator data of a small structured mesh on the device, and Q^T blockdiag(H_e) Q, dense, in long double."""

    def __init__(self, sf, torch, nel, nq_iso, dtype_name, signed):
        dim, dtype = len(nel), getattr(torch, dtype_name)
        self.nq, self.nm, self.dtype_name = (nq_iso,) * dim, nq_iso - 1, dtype_name
        self.l2g, self.nglobal = structured_map(nel, self.nm)
        self.nelmt, self.nmt, nqt = int(np.prod(nel)), self.nm ** dim, nq_iso ** dim
        self.nlocal, ncomp = self.l2g.size, len(COMPONENTS[dim])
        self.bs = [sf.fill_random(self.nm * nq_iso, 900 + d, dtype=dtype) for d in range(dim)]
        self.ds = [sf.fill_random(nq_iso * nq_iso, 910 + d, dtype=dtype) for d in range(dim)]
        self.g = sf.fill_random(self.nelmt * ncomp * nqt, 920, dtype=dtype)
        self.w = sf.fill_random(self.nelmt * nqt, 921, dtype=dtype)
        self.sign = random_sign(self.nlocal, 922, dtype_name) if signed else None
        self.sign_d = None if self.sign is None else _dev(torch, self.sign)
        self.gsmap = sf.gs_setup(_dev(torch, self.l2g), self.nglobal)
        ld = np.longdouble
        bh, dh = [_np(b) for b in self.bs], [_np(d) for d in self.ds]
        gh, wh = _np(self.g).reshape(self.nelmt, -1), _np(self.w).reshape(self.nelmt, -1)
        self.host = (bh, dh, gh, wh)
        n = self.nlocal
        self.H, self.absH = np.zeros((n, n), dtype=ld), np.zeros((n, n), dtype=ld)
        for e in range(self.nelmt):
            s = slice(e * self.nmt, (e + 1) * self.nmt)
            self.H[s, s] = dense_operator(self.nq, bh, dh, gh[e], wh[e], LAM)
            self.absH[s, s] = dense_operator(self.nq, [np.abs(b) for b in bh], [np.abs(d) for d in dh], np.abs(gh[e]),
                                             np.abs(wh[e]), LAM)
        self.Q = np.zeros((n, self.nglobal), dtype=ld)
        self.Q[np.arange(n), self.l2g] = 1 if self.sign is None else self.sign
        self.A = self.Q.T @ self.H @ self.Q
        self.rows = multiplicity(self.l2g, self.nglobal)

    def bound(self, ref_local, b_local):
        """|Q|^T b + gamma_{v-1} |Q|^T (|ref| + b), elementwise over the global entries."""
        u, aq = unit_roundoff(self.dtype_name), np.abs(self.Q)
        gv = np.array([gamma(max(int(v) - 1, 0), u) for v in self.rows], dtype=np.longdouble)
        return aq.T @ b_local + gv * (aq.T @ (np.abs(ref_local) + b_local))


def _excess(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    if np.any(np.isnan(err)) or np.any((bound == 0) & (err > 0)):
        return float("inf")
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, 0.0)))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("nel", [(3, 2), (2, 2, 2)], ids=["2d-3x2", "3d-2x2x2"])
def test_assembled_helmholtz_operator_column_by_column(sf, torch_mod, nel, dtype_name):
    """assemble(helmholtz(global_to_local(e_g))) for every global unit vector against the dense Q^T blockdiag(H_e) Q."""
    torch = torch_mod
    p = Assembled(sf, torch, nel, 4, dtype_name, signed=True)
    helm = sf.helmholtz_hex if len(nel) == 3 else sf.helmholtz_quad
    u = unit_roundoff(dtype_name)
    eye = torch.eye(p.nglobal, dtype=getattr(torch, dtype_name), device="cuda")
    worst = 0.0
    for c in range(p.nglobal):
        x = sf.global_to_local(p.gsmap, eye[c], sign=p.sign_d)
        y = helm(p.nq, *p.bs, *p.ds, p.g, p.w, LAM, x)
        col = sf.assemble(p.gsmap, y, sign=p.sign_d)
        torch.cuda.synchronize()
        assert np.array_equal(_np(x).astype(np.longdouble), p.Q[:, c])
        ref_local = p.H @ p.Q[:, c]
        b_local = gamma(helm_n(p.nq), u) * (p.absH @ np.abs(p.Q[:, c]))
        worst = max(worst, _excess(_np(col), p.A[:, c], p.bound(ref_local, b_local)))
    print(f"assembled operator {nel} {dtype_name}: max |err| / bound = {worst:.3g}")
    assert float(np.max(np.abs(p.A))) > 0
    assert worst <= 1.0


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("nel", [(3, 2), (2, 2, 2)], ids=["2d-3x2", "3d-2x2x2"])
def test_assembled_diagonal(sf, torch_mod, nel, dtype_name):
    """assemble(diag_helmholtz(...)), sign None, against the diagonal of the dense assembled matrix."""
    torch = torch_mod
    p = Assembled(sf, torch, nel, 4, dtype_name, signed=False)
    f = sf.diag_helmholtz_hex if len(nel) == 3 else sf.diag_helmholtz_quad
    d_local = f(p.nq, *p.bs, *p.ds, p.g, p.w, LAM)
    got = sf.assemble(p.gsmap, d_local)
    torch.cuda.synchronize()
    bh, dh, gh, wh = p.host
    ref_local, absref_local = ref_diag(p.nq, p.nelmt, bh, dh, gh.reshape(-1), wh.reshape(-1), LAM)
    b_local = gamma(diag_n(p.nq), unit_roundoff(dtype_name)) * absref_local
    q = _excess(_np(got), np.diag(p.A), p.bound(ref_local, b_local))
    print(f"assembled diagonal {nel} {dtype_name}: max |err| / bound = {q:.3g}")
    assert float(np.max(np.abs(np.diag(p.A)))) > 0
    assert q <= 1.0
