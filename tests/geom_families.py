"""The geometric-factor family (sf_geom_*, sf_geom_affine_*) for tests/test_gpu_geom.py, in the pattern of
tests/fused_families.py and tests/affine_deriv_families.py: the literals of the cases, GeomProblem (the data of one case on
the device, its runs, its reference and its checks) and install_single() with the bodies of the tests every fused
family carries (refusals, stream capture, the first call of a process inside a capture, two streams in flight).

The Family adapter itself does not fit: this family has d inputs and up to four outputs of different lengths, each with
a bound of its own that is a running error bound (tests/geom_ref.py GeomRef), not gamma_N absref.  What fits is kept:
prepare() gives the coordinates -- deformed elements of geom_ref.deformed(), never raw random fills, whose Jacobians
would be singular somewhere -- the seeds, the guard bands (fused_families.Banded) and the bodies of install_single.

Operands.  bases / derivs / qws: the Legendre modal basis at the Gauss-Lobatto points, its differentiation matrix and
weights (geom_ref.gll_operands), rounded to the working precision; the reference is computed on the rounded values the
device holds.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from fused_families import F32, F64, NO_KERNEL, _refused, case_id, to_host
from geom_ref import AFFINE_OUTPUTS, OUTPUTS, deformed, gll_operands, ref_geom, sizes, unit_roundoff

WAVE_3D = (((2, 2, 2), 33), ((3, 3, 3), 1001), ((5, 5, 5), 67), ((6, 6, 6), 129), ((8, 8, 8), 65))
WAVE_2D = (((5, 5), 4099), ((16, 16), 127))
FALLBACK = (((6, 6, 12), 13), ((9, 9, 9), 15), ((23, 5), 14))
SUBSETS = (((3, 3, 3), 1001), ((5, 5), 4099))
REFUSED = _refused((((9, 9, 9),), 5, NO_KERNEL), (((6, 6, 12), (17, 17), (4, 9)), 5, ("wave",)),
                   (((8, 8),), 5, ("mfma", "thread")), (((13, 4, 4),), 2, ("auto",)), (((4, 4, 13),), 3, ("generic",)),
                   (((33, 5), (5, 33)), 3, ("auto",))) + (((13, 4, 4), 3, F32, "auto"),)
GRAPH = (((8, 8, 8), 2003), ((9, 9), 5003), ((6, 6, 12), 301), ((3, 3, 3), 1001))
FIRST_CALL = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
STREAMS, STREAM_SAMPLE = (((7, 7, 7), 3011), ((12, 12), 10003)), 64


def condition_limit(nq, dtype_name):
    """The limit on e(det) / |det| that the reference asserts: 2^-10 (geom_ref.py), with TWO exceptions, both float32.
    At (8, 8, 8) and (16, 16) the prescribed inputs cannot meet it in float32: e(J) = gamma_N(2^-24) absJ with the GLL
    differentiation matrix (entries up to 60 at 16 points) gives e(det) / |det| = 1.03e-3 and 2.55e-3 on these elements
    against 2^-10 = 0.98e-3; the figures that led to 2^-10 were taken in fp64.  The condition exists so that the
    second-order terms stay inside the factor 2 of the assertion: they are at most the sum of the relative errors of the
    factors of a value (fewer than ten of them, each at most a few times e(det) / |det|) times the first-order bound, so
    2^-8 = 3.9e-3 leaves them below a tenth of it.  The assertion on the outputs, |got - ref| <= 2 e, is the same
    everywhere."""
    return 2.0 ** -8 if (tuple(nq), dtype_name) in (((8, 8, 8), F32), ((16, 16), F32)) else 2.0 ** -10


def per_element(nq):
    """Scalars per element of every output."""
    d, nqt = len(nq), sizes(nq)[1]
    return {"df": d * d * nqt, "w": nqt, "g": d * (d + 1) // 2 * nqt, "detj": nqt, "dfe": d * d, "ge": d * (d + 1) // 2,
            "je": 1}


class GeomProblem:
    """One case on the device.  prepare() is the hook of the family: it fills .xs, the (d, n) coordinates."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed, affine=False):
        self.sf, self.torch, self.nq, self.nelmt, self.dtype_name = sf, torch_mod, tuple(nq), nelmt, dtype_name
        self.dtype, self.seed, self.affine = getattr(torch_mod, dtype_name), seed, affine
        self.d, self.per = len(nq), per_element(self.nq)
        dev = lambda a: torch_mod.tensor(np.asarray(a), dtype=self.dtype, device="cuda")      # noqa: E731
        self.bs, self.ds, self.qs = ([dev(v) for v in vs] for vs in gll_operands(self.nq))
        self.prepare()
        self._refs = {}

    def prepare(self):
        xs, self.A = deformed(self.nq, self.nelmt, 1000 + self.seed, affine=self.affine)
        n = xs[0].size
        pad = -n % 64                                               # rows 256-byte aligned, as physderiv_* returns them
        buf = self.torch.zeros((self.d, n + pad), dtype=self.dtype, device="cuda")
        for a in range(self.d):
            buf[a, :n] = self.torch.tensor(xs[a], dtype=self.dtype, device="cuda")
        self.xs = buf[:, :n]

    def prefix(self, n):
        """The problem of the first n elements: views of the same arrays."""
        import copy
        q = copy.copy(self)
        q.nelmt, q.xs, q._refs = n, self.xs[:, :n * sizes(self.nq)[0]], {}
        return q

    def run(self, outputs=OUTPUTS, out=None, variant="auto", xs=None, stream=None):
        """geom_hex / geom_quad: the dict of the outputs asked for."""
        fn = self.sf.geom_hex if self.d == 3 else self.sf.geom_quad
        return fn(self.nq, *self.bs, *self.ds, *self.qs, self.xs if xs is None else xs, outputs=outputs, out=out,
                  variant=variant, stream=stream)

    def run_affine(self, xs=None, stream=None):
        fn = self.sf.geom_affine_hex if self.d == 3 else self.sf.geom_affine_quad
        return dict(zip(AFFINE_OUTPUTS, fn(self.nq, *self.bs, *self.ds, self.xs if xs is None else xs, stream=stream)))

    def host_operands(self):
        return [[to_host(t).astype(np.float64) for t in v] for v in (self.bs, self.ds, self.qs)]

    def reference(self, elements=None, affine=False, xs=None):
        """GeomRef on what the device holds (of the elements `elements` only); the condition is asserted inside."""
        key = (None if elements is None else tuple(int(e) for e in elements), affine, xs is None)
        if key not in self._refs or xs is not None:
            B, D, Q = self.host_operands()
            src = self.xs if xs is None else xs
            rows = [to_host(src[a]).astype(np.float64).reshape(self.nelmt, -1) for a in range(self.d)]
            n = self.nelmt
            if elements is not None:
                rows, n = [r[np.asarray(elements)] for r in rows], len(elements)
            ref = ref_geom(self.nq, n, B, D, Q, [r.reshape(-1) for r in rows], unit_roundoff(self.dtype_name), affine=affine,
                           limit=condition_limit(self.nq, self.dtype_name))
            if xs is not None:
                return ref
            self._refs[key] = ref
        return self._refs[key]

    def check(self, got, what, elements=None, affine=False, ref=None):
        """Every output in `got` within 2 e of the long-double reference, elementwise; prints each figure first."""
        ref = self.reference(elements, affine) if ref is None else ref
        for name, t in got.items():
            host = to_host(t).reshape(self.nelmt, -1)
            if elements is not None:
                host = host[np.asarray(elements)]
            q = ref.excess(name, host)
            print(f"{what}: geom {self.nq} {self.dtype_name} nelmt={self.nelmt} {name}: max |err| / (2 e) = {q:.3g}")
            assert q <= 1.0, (what, self.nq, self.dtype_name, name, q)
            assert float(np.max(np.abs(ref.val[name]))) > 0, (what, name)


def bits(torch_mod, t):
    """The tensor as integers: equal bits, NaN included."""
    return t.view(torch_mod.int64 if t.dtype == torch_mod.float64 else torch_mod.int32)


def same_bits(torch_mod, a, b):
    return a.keys() == b.keys() and all(torch_mod.equal(bits(torch_mod, a[k]), bits(torch_mod, b[k])) for k in a)


def install_single(ns):
    """The family's cases of the tests of tests/test_gpu_fused_common.py, with the bodies they have there."""

    def test_refusals(sf, torch_mod):
        """Extents outside the fallback's bounds, "wave" off the table, variants without a fused kernel: SF_ENOTBUILT."""
        for nq, nelmt, dtype_name, variant in REFUSED:
            p = GeomProblem(sf, torch_mod, nq, nelmt, dtype_name, 2)
            with pytest.raises(sf.capi.SumfactError) as ei:
                p.run(variant=variant)
            assert ei.value.rc == sf.capi.SF_ENOTBUILT, (nq, dtype_name, variant)
            if variant == "auto":                                   # the affine form has the fallback's bounds
                with pytest.raises(sf.capi.SumfactError) as ei:
                    p.run_affine()
                assert ei.value.rc == sf.capi.SF_ENOTBUILT, (nq, dtype_name)

    @pytest.mark.parametrize("nq,nelmt", GRAPH, ids=[case_id(s) + "-" + str(n) for s, n in GRAPH])
    def test_captured_graph_replay_matches_eager(sf, torch_mod, nq, nelmt):
        p = GeomProblem(sf, torch_mod, nq, nelmt, F64, 11)
        for outputs in (OUTPUTS, ("df",), ("g", "w")):
            eager = p.run(outputs)
            outs = {k: torch_mod.zeros_like(t) for k, t in eager.items()}
            torch_mod.cuda.synchronize()
            side = torch_mod.cuda.Stream()
            side.wait_stream(torch_mod.cuda.current_stream())
            g = torch_mod.cuda.CUDAGraph()
            with torch_mod.cuda.stream(side):
                with torch_mod.cuda.graph(g, stream=side):
                    p.run(outputs, out=outs, stream=side)
            torch_mod.cuda.current_stream().wait_stream(side)
            g.replay()
            torch_mod.cuda.synchronize()
            assert same_bits(torch_mod, outs, eager)
            assert all(float(o.abs().max()) > 0 for o in outs.values())
        sample = [0, 1, nelmt // 2, nelmt - 1]
        p.check(outs, "graph", elements=sample)

    def test_first_call_inside_a_capture():
        """Capture-safe from the first call: a fresh child process whose first call of each route of the family (3D wave,
        3D fallback, 2D wave, 2D fallback, then the affine kernel) is inside a stream capture; the replay equals an eager
        call made afterwards."""
        script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geom_first_call.py")
        r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

    def test_two_streams_in_flight(sf, torch_mod):
        """Two problems enqueued on two streams before either is waited for; a seeded sample of elements and the ends
        against long double."""
        streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
        probs = [GeomProblem(sf, torch_mod, nq, nelmt, F64, nelmt % 97) for nq, nelmt in STREAMS]
        torch_mod.cuda.synchronize()
        outs = []
        for p, st in zip(probs, streams):
            with torch_mod.cuda.stream(st):
                outs.append(p.run(stream=st))
        torch_mod.cuda.synchronize()
        rng = np.random.default_rng(7)
        for p, o in zip(probs, outs):
            ends = [0, 1, p.nelmt - 2, p.nelmt - 1]
            sample = np.unique(np.concatenate((ends, rng.integers(0, p.nelmt, STREAM_SAMPLE))))
            p.check(o, "stream job", elements=sample)

    ns.update(test_refusals=test_refusals, test_captured_graph_replay_matches_eager=test_captured_graph_replay_matches_eager,
              test_first_call_inside_a_capture=test_first_call_inside_a_capture,
              test_two_streams_in_flight=test_two_streams_in_flight)
