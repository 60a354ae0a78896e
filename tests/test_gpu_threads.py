"""GPU tests of the promise of include/sumfact.h that every entry point may be called concurrently from several host
threads, also on ONE stream: (1) the persistent 2D kernels (nq 25..32, a batch counter per stream) launched by four
threads on one stream; (2) every operator family interleaved by four threads, on one shared stream and on one stream per
thread; (3) a process's first calls made by eight threads at once (a fresh child process); (4) the batch-counter ring
exhausted, so that the fixed-share kernel runs eagerly.

Rules of every test: all tensors exist before a thread starts and the threads only launch, released together by a
barrier; every launch writes to an output of its own that holds NaN beforehand, so an unwritten result cannot pass for a
stale correct one; the expected result is the same call made serially beforehand on the same stream, compared with
torch.equal (no kernel uses atomics on its output: reruns are bit-identical); that serial result is first checked against
the project's reference within the reference's own bound (BwdTrans: the oracle, 1e-12 in fp64 and 2e-5 in fp32; the fused
operators: the long-double references of tests/*_ref.py, excess <= 1).  A thread's exception is raised again in the
main thread, a thread that outlives join(timeout=120) fails the test, and a thread stops launching at the first
non-zero return code.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from affine_ref import affine_excess, ref_affine
from helm_ref import helm_excess, ref_helmholtz
from iprod_ref import U32, U64, elementwise_excess, ref_iprod
from iprodderiv_ref import iprodderiv_excess, ref_iprodderiv
from mass_ref import mass_excess, ref_mass
from physderiv_ref import physderiv_excess, ref_physderiv

pytestmark = pytest.mark.gpu

TOL, TOL32 = 1e-12, 2e-5
JOIN_TIMEOUT = 120
LAM = 0.75


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


def _np64(t):
    return _np(t).astype(np.float64)


def run_threads(workers):
    """Start one thread per callable behind a barrier; join each with a timeout; raise a thread's exception here."""
    barrier = threading.Barrier(len(workers))
    errors = [None] * len(workers)

    def body(i):
        try:
            barrier.wait(timeout=JOIN_TIMEOUT)
            workers[i]()
        except BaseException as e:      # noqa: B036 -- handed to the main thread below
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(workers))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=JOIN_TIMEOUT)
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"threads {alive} still run after {JOIN_TIMEOUT} s"
    for e in errors:
        if e is not None:
            raise e


# ---- 1. the persistent 2D kernels: several threads, one stream -------------------------------------------------------
def hammer_persistent_quad(sf, torch, oracle, nq, variant, stream, nthreads, launches, nelmt=101):
    """`nthreads` threads make `launches` calls each of 2D BwdTrans nq x nq on `stream` (None: the null stream) through
    the raw C entry point, arguments marshalled beforehand: the calls release the GIL, so the threads are inside the
    library at the same time.  Thread t has its own input.  Returns (outputs that differ from their thread's serial
    result, outputs that hold a NaN, outputs in all)."""
    fn = sf.capi.lib().sf_bwdtrans_quad_f64_variant
    nm, n = nq - 1, nelmt * nq * nq
    bs = [sf.fill_random(nm * nq, 300 + d + nq) for d in range(2)]          # a basis of its own per direction
    xs = [sf.fill_random(nelmt * nm * nm, 1000 + 17 * t + nq) for t in range(nthreads)]
    torch.cuda.synchronize()
    want = [sf.bwdtrans_quad((nq, nq), *bs, x, variant=variant, stream=stream) for x in xs]
    torch.cuda.synchronize()
    for x, w in zip(xs, want):
        ref = oracle.bwdtrans_quad((nq, nq), nelmt, _np(bs[0]), _np(bs[1]), _np(x))
        err = oracle.rel_err(_np(w), ref)
        assert err <= TOL, (nq, variant, err)
    # one output per launch; rows start 256-byte aligned, as fresh allocations would (an odd row length would otherwise
    # put every second output on an 8-byte boundary, which AUTO serves with another kernel)
    stride = (n + 31) // 32 * 32
    outs = [torch.full((launches, stride), float("nan"), dtype=torch.float64, device="cuda") for _ in range(nthreads)]
    handle = ctypes.c_void_p(None if stream is None else stream.cuda_stream)
    v = sf.VARIANTS[variant]
    calls = [[(v, nq, nq, nelmt, ctypes.c_void_p(bs[0].data_ptr()), ctypes.c_void_p(bs[1].data_ptr()),
               ctypes.c_void_p(xs[t].data_ptr()), None, ctypes.c_void_p(outs[t][k].data_ptr()), handle)
              for k in range(launches)] for t in range(nthreads)]
    torch.cuda.synchronize()

    def worker(t):
        def work():
            for args in calls[t]:
                sf.capi.check(fn(*args), "sf_bwdtrans_quad_f64_variant")    # raises, and so stops, at a non-zero code
        return work

    run_threads([worker(t) for t in range(nthreads)])
    torch.cuda.synchronize()
    wrong = nans = 0
    for t in range(nthreads):
        got = outs[t][:, :n]
        wrong += int((got != want[t][None, :]).any(dim=1).sum())
        nans += int(torch.isnan(got).any(dim=1).sum())
        if wrong == 0:
            assert torch.equal(got, want[t][None, :].expand(launches, n))
    return wrong, nans, nthreads * launches


PERSISTENT = [(25, "auto"), (28, "auto"), (31, "auto"), (32, "mfma4")]     # all four draw batches from a counter


@pytest.mark.parametrize("which", ["shared", "null"])
@pytest.mark.parametrize("nq,variant", PERSISTENT, ids=[f"nq{n}-{v}" for n, v in PERSISTENT])
def test_persistent_quad_kernels_several_threads_one_stream(sf, torch_mod, oracle, nq, variant, which):
    """Four host threads, 100 launches each of 101 elements (several batches per launch at both batch sizes) on ONE
    stream -- a torch.cuda.Stream() they share, or the null stream, which is what every new Python thread gets from
    torch.cuda.current_stream().  The launches of a stream share that stream's batch counter: a launch whose counter
    reset and kernel are not one unit on the stream finds the counter drained by another thread's kernel and writes
    nothing (the sentinel NaN stays), silently."""
    stream = torch_mod.cuda.Stream() if which == "shared" else None
    wrong, nans, total = hammer_persistent_quad(sf, torch_mod, oracle, nq, variant, stream, nthreads=4, launches=100)
    print(f"nq {nq} {variant} {which} stream: {wrong} of {total} outputs wrong, {nans} hold a NaN")
    assert wrong == 0 and nans == 0, f"{wrong} of {total} outputs differ from the serial result ({nans} hold a NaN)"


# ---- 2. every operator family, interleaved ------------------------------------------------------------------------
class Job:
    """One call with its own data: call(out, stream) -> the result (`out`, or a float), new_out() -> a NaN-filled output
    (None for a scalar result), check(result): the result against the reference of its family."""

    def __init__(self, name, call, new_out, check):
        self.name, self.call, self.new_out, self.check = name, call, new_out, check


def _sizes(nq):
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def _same(torch, a, b):
    return a == b if isinstance(b, float) else torch.equal(a, b)


def build_jobs(sf, torch, oracle):
    jobs = []
    nan = float("nan")

    def rnd(n, seed, dtype):
        return sf.fill_random(n, seed, dtype=dtype)

    def flat(n, dtype):
        return lambda: torch.full((n,), nan, dtype=dtype, device="cuda")

    def operands(nq, nelmt, seed, dtype):
        nmt, nqt = _sizes(nq)
        bs = [rnd((q - 1) * q, seed + 1 + d, dtype) for d, q in enumerate(nq)]
        ds = [rnd(q * q, seed + 11 + d, dtype) for d, q in enumerate(nq)]
        return nmt, nqt, bs, ds

    def bwd(nq, variant, nelmt=37, f32=False):
        seed, dtype = 100 * len(jobs), torch.float32 if f32 else torch.float64
        nmt, nqt, bs, _ = operands(nq, nelmt, seed, dtype)
        x = rnd(nelmt * nmt, seed, dtype)
        fn, ofn = (sf.bwdtrans_hex, oracle.bwdtrans_hex) if len(nq) == 3 else (sf.bwdtrans_quad, oracle.bwdtrans_quad)

        def check(got):
            err = oracle.rel_err(_np64(got), ofn(tuple(nq), nelmt, *[_np64(b) for b in bs], _np64(x)))
            assert err <= (TOL32 if f32 else TOL), (nq, variant, err)

        jobs.append(Job(f"bwdtrans {nq} {variant}{' f32' if f32 else ''}",
                        lambda out, st: fn(nq, *bs, x, out=out, variant=variant, stream=st), flat(nelmt * nqt, dtype),
                        check))

    def fused(name, nq, make, nelmt=37, f32=False):
        """make(nelmt, nmt, nqt, bs, ds, rnd1) -> (call(out, st), numel or shape of out, reference() -> (ref, absref), the
        excess function of the family)"""
        seed, dtype = 100 * len(jobs), torch.float32 if f32 else torch.float64
        nmt, nqt, bs, ds = operands(nq, nelmt, seed, dtype)
        count = [0]

        def rnd1(n):
            count[0] += 1
            return rnd(n, seed + 20 + count[0], dtype)

        call, shape, reference, excess = make(nelmt, nmt, nqt, bs, ds, rnd1)
        u = U32 if f32 else U64

        def check(got):
            ref, absref = reference()
            assert float(np.max(np.abs(ref))) > 0
            q = excess(_np(got), ref, absref, nq, u)
            assert q <= 1.0, (name, nq, q)

        shape = (shape,) if isinstance(shape, int) else shape
        jobs.append(Job(f"{name} {nq}{' f32' if f32 else ''}", call,
                        lambda: torch.full(shape, nan, dtype=dtype, device="cuda"), check))

    def hq(nq, hexfn, quadfn):
        return hexfn if len(nq) == 3 else quadfn

    def iproduct(nq):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            x = rnd1(nelmt * nqt)
            f = hq(nq, sf.iproduct_hex, sf.iproduct_quad)
            return (lambda out, st: f(nq, *bs, x, out=out, stream=st), nelmt * nmt,
                    lambda: ref_iprod(nq, nelmt, [_np(b) for b in bs], _np(x)), elementwise_excess)
        fused("iproduct", nq, make)

    def mass(nq):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            w, x = rnd1(nelmt * nqt), rnd1(nelmt * nmt)
            f = hq(nq, sf.mass_hex, sf.mass_quad)
            return (lambda out, st: f(nq, *bs, w, x, out=out, stream=st), nelmt * nmt,
                    lambda: ref_mass(nq, nelmt, [_np(b) for b in bs], _np(w), _np(x)), mass_excess)
        fused("mass", nq, make)

    def helmholtz(nq, f32=False):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            ncomp = len(nq) * (len(nq) + 1) // 2
            g, w, x = rnd1(nelmt * ncomp * nqt), rnd1(nelmt * nqt), rnd1(nelmt * nmt)
            f = hq(nq, sf.helmholtz_hex, sf.helmholtz_quad)
            return (lambda out, st: f(nq, *bs, *ds, g, w, LAM, x, out=out, stream=st), nelmt * nmt,
                    lambda: ref_helmholtz(nq, nelmt, [_np(b) for b in bs], [_np(d) for d in ds], _np(g), _np(w), LAM,
                                          _np(x)), helm_excess)
        fused("helmholtz", nq, make, f32=f32)

    def affine(nq):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            ncomp = len(nq) * (len(nq) + 1) // 2
            qs = [rnd1(q) for q in nq]
            ge, je, x = rnd1(nelmt * ncomp), rnd1(nelmt), rnd1(nelmt * nmt)
            f = hq(nq, sf.affine_helmholtz_hex, sf.affine_helmholtz_quad)
            return (lambda out, st: f(nq, *bs, *ds, *qs, ge, je, LAM, x, out=out, stream=st), nelmt * nmt,
                    lambda: ref_affine(nq, nelmt, [_np(b) for b in bs], [_np(d) for d in ds], [_np(q) for q in qs],
                                       _np(ge), _np(je), LAM, _np(x)), affine_excess)
        fused("affine_helmholtz", nq, make)

    def physderiv(nq):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            d = len(nq)
            df, x = rnd1(nelmt * d * d * nqt), rnd1(nelmt * nmt)
            f = hq(nq, sf.physderiv_hex, sf.physderiv_quad)
            return (lambda out, st: f(nq, *bs, *ds, df, x, out=out, stream=st), (d, nelmt * nqt),
                    lambda: ref_physderiv(nq, nelmt, [_np(b) for b in bs], [_np(m) for m in ds], _np(df), _np(x)),
                    physderiv_excess)
        fused("physderiv", nq, make)

    def iprodderiv(nq):
        def make(nelmt, nmt, nqt, bs, ds, rnd1):
            d = len(nq)
            df, w = rnd1(nelmt * d * d * nqt), rnd1(nelmt * nqt)
            fin = rnd1(d * nelmt * nqt).view(d, nelmt * nqt)
            f = hq(nq, sf.iprodderiv_hex, sf.iprodderiv_quad)
            return (lambda out, st: f(nq, *bs, *ds, df, w, fin, out=out, stream=st), nelmt * nmt,
                    lambda: ref_iprodderiv(nq, nelmt, [_np(b) for b in bs], [_np(m) for m in ds], _np(df), _np(w),
                                           [_np(r) for r in fin]), iprodderiv_excess)
        fused("iprodderiv", nq, make)

    bwd((8, 8, 8), "wave")
    bwd((3, 5, 4), "wave-rt")                   # run-time extents
    bwd((12, 12, 12), "mfma4")
    bwd((13, 13, 13), "mfma")
    bwd((22, 22, 22), "auto", nelmt=3)          # the any-extent kernel on the library's scratch (scratch_mutex)
    bwd((16, 16), "wave")
    bwd((21, 21), "mfma4")
    bwd((28, 28), "auto")                       # persistent, batch counter
    bwd((32, 32), "mfma")
    bwd((40, 40), "auto")                       # generic
    iproduct((8, 8, 8))
    iproduct((12, 12))
    mass((8, 8, 8))
    helmholtz((8, 8, 8))
    helmholtz((6, 6, 12))                       # the fallback shape
    affine((8, 8, 8))
    physderiv((8, 8, 8))
    iprodderiv((12, 12))
    bwd((8, 8, 8), "auto", f32=True)
    helmholtz((9, 9), f32=True)

    big = sf.fill_random(100003, 4242)

    def check_sumsq(got):
        want = oracle.sumsq(_np(big))
        assert abs(got - want) <= 1e-12 * want

    jobs.append(Job("sumsq", lambda out, st: sf.sumsq(big, stream=st), lambda: None, check_sumsq))   # blocking, a float

    a, xv = sf.fill_random(37 * 101, 4243), sf.fill_random(101, 4244)

    def check_matvec(got):
        assert oracle.rel_err(_np(got), oracle.matvec(37, 101, _np(a), _np(xv))) <= TOL

    jobs.append(Job("matvec", lambda out, st: sf.matvec(37, 101, a, xv, y=out, stream=st), flat(37, torch.float64),
                    check_matvec))
    return jobs


@pytest.fixture(scope="module")
def jobs(sf, torch_mod, oracle):
    """The job list and each job's serial result on the null stream, checked once against the reference of its family."""
    torch = torch_mod
    js = build_jobs(sf, torch, oracle)
    torch.cuda.synchronize()
    serial = [j.call(j.new_out(), None) for j in js]
    torch.cuda.synchronize()
    for j, r in zip(js, serial):
        j.check(r)
    return js, serial


ROUNDS = 3


@pytest.mark.parametrize("streams", ["one shared stream", "one stream per thread"])
def test_every_operator_family_interleaved(sf, torch_mod, jobs, streams):
    """Four threads walk the job list (every BwdTrans route, every fused operator, two fp32 jobs, the blocking reduction,
    the matrix-vector product), each from another rotation, three rounds: on one stream the scratch of the any-extent
    kernel and of the reduction, the reduction's result copy and the batch counter of 2D nq 28 are shared by all four."""
    torch = torch_mod
    js, serial = jobs
    nthreads = 4
    if streams == "one shared stream":
        sts = [torch.cuda.Stream()] * nthreads
    else:
        sts = [torch.cuda.Stream() for _ in range(nthreads)]
    torch.cuda.synchronize()
    for st in {id(s): s for s in sts}.values():     # the same calls made serially on the stream of the threads
        fresh = [j.new_out() for j in js]
        torch.cuda.synchronize()                    # the NaN fills run on the null stream, which `st` does not wait for
        again = [j.call(o, st) for j, o in zip(js, fresh)]
        st.synchronize()
        for j, r, s in zip(js, again, serial):
            assert _same(torch, r, s), (j.name, "serial call on another stream")
    order = [[(i + t * len(js) // nthreads) % len(js) for i in range(len(js))] * ROUNDS for t in range(nthreads)]
    outs = [[js[i].new_out() for i in order[t]] for t in range(nthreads)]
    results = [[float("nan")] * len(order[t]) for t in range(nthreads)]
    torch.cuda.synchronize()

    def worker(t):
        def work():
            for k, i in enumerate(order[t]):
                results[t][k] = js[i].call(outs[t][k], sts[t])     # a non-zero code raises SumfactError: the thread stops
        return work

    run_threads([worker(t) for t in range(nthreads)])
    torch.cuda.synchronize()
    bad = [(t, k, js[i].name) for t in range(nthreads) for k, i in enumerate(order[t])
           if not _same(torch, results[t][k], serial[i])]
    assert not bad, f"{len(bad)} of {nthreads * len(order[0])} results differ from the serial ones: {bad[:8]}"


# ---- 3. a process's first calls, made by eight threads at once ---------------------------------------------------------
FIRST_CALLS_THREADED = r"""
import sys
import threading
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
sf = ge.load_package()
sf.capi.lib()                                   # dlopen only: no call into the library yet
torch.manual_seed(7)
nan = float("nan")


def rnd(*shape):                                # torch only: the library's first kernel launch is made by the threads
    return torch.rand(*shape, dtype=torch.float64, device="cuda") * 2 - 1


def sizes(nq):
    nmt, nqt = 1, 1
    for q in nq:
        nmt, nqt = nmt * (q - 1), nqt * q
    return nmt, nqt


def operands(nq):
    return [rnd((q - 1) * q) for q in nq], [rnd(q * q) for q in nq]


def bwd(nq, nelmt):
    (nmt, nqt), (bs, _) = sizes(nq), operands(nq)
    x = rnd(nelmt * nmt)
    f = sf.bwdtrans_hex if len(nq) == 3 else sf.bwdtrans_quad
    return nelmt * nqt, lambda out: f(nq, *bs, x, out=out)


def helmholtz(nq, nelmt):
    (nmt, nqt), (bs, ds) = sizes(nq), operands(nq)
    g, w, x = rnd(nelmt * 6 * nqt), rnd(nelmt * nqt), rnd(nelmt * nmt)
    return nelmt * nmt, lambda out: sf.helmholtz_hex(nq, *bs, *ds, g, w, 0.75, x, out=out)


def iprodderiv(nq, nelmt):
    (nmt, nqt), (bs, ds) = sizes(nq), operands(nq)
    df, w, fin = rnd(nelmt * 4 * nqt), rnd(nelmt * nqt), rnd(2, nelmt * nqt)
    return nelmt * nmt, lambda out: sf.iprodderiv_quad(nq, *bs, *ds, df, w, fin, out=out)


def mass(nq, nelmt):
    (nmt, nqt), (bs, _) = sizes(nq), operands(nq)
    w, x = rnd(nelmt * nqt), rnd(nelmt * nmt)
    return nelmt * nmt, lambda out: sf.mass_hex(nq, *bs, w, x, out=out)


big = rnd(100003)
jobs = [bwd((8, 8, 8), 37), bwd((8, 8, 8), 37),             # two threads, the same instantiation
        bwd((28, 28), 101), bwd((22, 22, 22), 3), helmholtz((8, 8, 8), 37), iprodderiv((12, 12), 37),
        mass((8, 8, 8), 37), (None, lambda out: sf.sumsq(big))]


def new_out(n):
    return None if n is None else torch.full((n,), nan, dtype=torch.float64, device="cuda")


outs = [new_out(n) for n, _ in jobs]
again = [new_out(n) for n, _ in jobs]
torch.cuda.synchronize()
barrier = threading.Barrier(len(jobs))
got, errors = [nan] * len(jobs), [None] * len(jobs)


def body(i):
    try:
        barrier.wait(timeout=120)
        got[i] = jobs[i][1](outs[i])            # one call on the null stream: this thread's current stream
    except BaseException as e:
        errors[i] = e


threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
for t in threads:
    t.start()
for t in threads:
    t.join(timeout=120)
assert not any(t.is_alive() for t in threads), "a thread still runs"
for e in errors:
    if e is not None:
        raise e
torch.cuda.synchronize()
for i, (n, call) in enumerate(jobs):
    want = call(again[i])
    torch.cuda.synchronize()
    if n is None:
        assert got[i] == want and want == want and want > 0, (i, got[i], want)
    else:
        assert torch.equal(got[i], want), (i, int((got[i] != want).sum()))
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0, i
print("first calls threaded")
"""


def test_first_calls_of_a_process_made_by_eight_threads():
    """A fresh child process whose first calls into the library -- first kernel launch, first occupancy query, first
    device_info(), first counter and scratch allocation -- are made by eight threads at once on the null stream, two of
    them the same instantiation; each result equals the same call repeated serially afterwards."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", FIRST_CALLS_THREADED, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first calls threaded" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- 4. the counter ring, exhausted ------------------------------------------------------------------------------------
COUNTER_SLOTS = 8192       # kCounterSlots of csrc/aux_kernels.hip: a change of that constant has to be made here too


class PerThreadStream:
    cuda_stream = 2         # hipStreamPerThread


def test_counter_ring_exhausted(sf, torch_mod, oracle):
    """Counter slots are not recycled and a launch on hipStreamPerThread keeps one for good: after kCounterSlots such
    launches a stream without a slot gets none and runs the fixed-share kernel -- eagerly, which nothing else reaches
    (the capture test reaches it inside a capture only).  Its result equals the batched one bit for bit, a stream that has
    a slot keeps using it, and two threads on the slotless stream stay right."""
    torch = torch_mod
    lib = sf.capi.lib()
    nq, nelmt = 28, 37
    nm = nq - 1
    torch.cuda.synchronize()
    assert lib.sf_shutdown() == 0                   # an empty ring: no pooled stream handle owns a slot from earlier tests
    try:
        bs = [sf.fill_random(nm * nq, 61 + d) for d in range(2)]
        x = sf.fill_random(nelmt * nm * nm, 63)
        small = torch.full((5 * nq * nq,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s0 = torch.cuda.Stream()
        want = sf.bwdtrans_quad((nq, nq), *bs, x, stream=s0)       # s0 takes a slot and keeps it
        want5 = sf.bwdtrans_quad((nq, nq), *bs, x[:5 * nm * nm], stream=s0)
        s0.synchronize()
        ref = oracle.bwdtrans_quad((nq, nq), nelmt, _np(bs[0]), _np(bs[1]), _np(x))
        assert oracle.rel_err(_np(want), ref) <= TOL
        for _ in range(COUNTER_SLOTS + 64):                         # one slot per launch, never given back
            sf.bwdtrans_quad((nq, nq), *bs, x[:5 * nm * nm], out=small, stream=PerThreadStream)
        torch.cuda.synchronize()
        assert torch.equal(small, want5)
        fresh = torch.cuda.Stream()
        assert fresh.cuda_stream != s0.cuda_stream
        out = torch.full_like(want, float("nan"))
        sf.bwdtrans_quad((nq, nq), *bs, x, out=out, stream=fresh)   # no slot to be had: the fixed-share kernel
        fresh.synchronize()
        assert torch.equal(out, want), int((out != want).sum())
        out = torch.full_like(want, float("nan"))
        sf.bwdtrans_quad((nq, nq), *bs, x, out=out, stream=s0)      # s0 still draws batches from its counter
        s0.synchronize()
        assert torch.equal(out, want), int((out != want).sum())
        wrong, nans, total = hammer_persistent_quad(sf, torch, oracle, nq, "auto", fresh, nthreads=2, launches=50)
        assert wrong == 0 and nans == 0, f"{wrong} of {total} outputs differ from the serial result ({nans} hold a NaN)"
    finally:
        torch.cuda.synchronize()
        assert lib.sf_shutdown() == 0               # no later test inherits a full ring
