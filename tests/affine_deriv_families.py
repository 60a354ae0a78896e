"""Adapters of sf_aff_physderiv_* and sf_aff_iprodderiv_* to the common GPU tests of the fused families
(tests/fused_families.py Family, tests/fused_common.py install()), and install_single(): this pair's cases of the tests
that tests/test_gpu_fused_common.py writes once over fused_families.COMMON (refusals, stream capture, the first call of
a process inside a capture, two streams in flight) -- COMMON is a fixed list there, so the two families carry those cases
in their own files, with the same bodies.

References and bounds: tests/affine_deriv_ref.py (long double; N = physderiv_n for the gradient, iprodderiv_n + d for the
weak divergence).  Like Affine, the per-element constants are too short for an element count to change what is exercised:
one Problem per shape, runs on prefixes (Affine.plan).  The ragged shapes are where the lane -> element map of the
per-element constants can go wrong: many elements per wave in two passes (3D nq 2, 3), two elements (nq 5), one element
and uniform constants (nq 6, 7, 8), the 2D chunk sizes, and the shrunk fp32 rows.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from affine_deriv_ref import (affine_iprodderiv_excess, affine_iprodderiv_n, affine_physderiv_excess, affine_physderiv_n,
                              ref_affine_iprodderiv, ref_affine_physderiv)
from fused_families import (F32, F64, NO_KERNEL, RAGGED, SCALAR, VEC, Affine, Family, Operand, _refused, case_id, own_problem,
                            sizes)
from multifield_common import capture_replay, same_bits

_GUARD = {(2, 2, 2): 33, (3, 3, 3): 1001, (5, 5, 5): 67, (6, 6, 6): 129, (8, 8, 8): 65, (5, 5): 4099, (16, 16): 127,
          (6, 6, 12): 13, (9, 9, 9): 15, (23, 5): 14}
_REFUSED = (_refused((((9, 9, 9),), 5, NO_KERNEL), (((6, 6, 12), (17, 17), (4, 9)), 5, ("wave",)),
                     (((8, 8),), 5, ("mfma", "thread")), (((13, 4, 4),), 2, ("auto",)), (((4, 4, 13),), 3, ("generic",)),
                     (((33, 5), (5, 33)), 3, ("auto",))) + (((13, 4, 4), 3, F32, "auto"),))


class _AffineDeriv(Family):
    consts = ("bs", "ds")
    ragged, ragged_shapes, fallback = RAGGED, Affine.ragged_shapes, Affine.fallback
    ragged_seed, fallback_seed = staticmethod(lambda n: 3), staticmethod(lambda n: 70)
    explicit_count, refused, guard = 333, _REFUSED, _GUARD
    graph = (((8, 8, 8), 2003), ((9, 9), 5003), ((6, 6, 12), 301), ((3, 3, 3), 1001))
    first_call = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
    streams, stream_sample, stream_ld = (((7, 7, 7), 3011), ((12, 12), 10003)), 256, True
    plan = Affine.plan


class AffinePhysDeriv(_AffineDeriv):
    name = stem = "affine_physderiv"
    guard_test = "test_guard_words_around_every_output_and_nan_around_in_and_dfe"

    def operands(self, nq):
        return [Operand("in", sizes(nq)[0], VEC, False, 10), Operand("dfe", len(nq) ** 2, SCALAR, False, 8000)]

    def out_parts(self, nq):
        return len(nq)

    def out_per(self, nq):
        return sizes(nq)[1]

    def call(self, sf, nq, c, d, out, variant, **kw):
        got = self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["dfe"], d["in"], out=out, variant=variant, **kw)
        return [got[a] for a in range(len(nq))]

    def ref(self, nq, n, c, d, ld=True):
        return ref_affine_physderiv(nq, n, c["bs"], c["ds"], d["dfe"], d["in"], np.longdouble if ld else np.float64)

    excess = staticmethod(affine_physderiv_excess)
    n = staticmethod(affine_physderiv_n)


class AffineIProdDeriv(_AffineDeriv):
    name = stem = "affine_iprodderiv"
    consts, modes, guarded_consts = ("bs", "ds", "qs"), (("je",), ()), ("qs",)
    guard_test = "test_guard_words_around_out_and_nan_around_every_input_dfe_je_and_qw"

    def prepare(self, p, sf):
        """The d inputs as the rows of one (d, n) array of one seed, as sf_aff_physderiv_* returns them."""
        n = p.nelmt * sizes(p.nq)[1]
        rows = sf.fill_random(len(p.nq) * n, 10 + p.seed, dtype=p.dtype).view(len(p.nq), n)
        p.data.update({f"in{a}": rows[a] for a in range(len(p.nq))})

    def operands(self, nq):
        nqt = sizes(nq)[1]
        return ([Operand(f"in{a}", nqt, SCALAR, False, 10 + 2000 * a) for a in range(len(nq))]
                + [Operand("dfe", len(nq) ** 2, SCALAR, False, 8000), Operand("je", 1, SCALAR, True, 7000)])

    def call(self, sf, nq, c, d, out, variant, **kw):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], *c["qs"], d["dfe"], d["je"], ins, out=out and out[0],
                                 variant=variant, **kw)]

    def ref(self, nq, n, c, d, ld=True):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return ref_affine_iprodderiv(nq, n, c["bs"], c["ds"], c["qs"], d["dfe"], d["je"], ins,
                                     np.longdouble if ld else np.float64)

    excess = staticmethod(affine_iprodderiv_excess)
    n = staticmethod(affine_iprodderiv_n)


AFFINE_PHYSDERIV, AFFINE_IPRODDERIV = AffinePhysDeriv(), AffineIProdDeriv()
BY_NAME = {f.name: f for f in (AFFINE_PHYSDERIV, AFFINE_IPRODDERIV)}


def install_single(ns, fam):
    """The family's cases of the tests of tests/test_gpu_fused_common.py, with the bodies they have there."""

    def test_refusals(sf, torch_mod):
        """Extents outside the fallback's bounds, "wave" off the table, variants without a fused kernel: SF_ENOTBUILT."""
        for nq, nelmt, dtype_name, variant in fam.refused:
            p = own_problem(fam, sf, torch_mod, nq, nelmt, dtype_name, 2)
            with pytest.raises(sf.capi.SumfactError) as ei:
                p.run(sf, variant=variant)
            assert ei.value.rc == sf.capi.SF_ENOTBUILT, (nq, dtype_name, variant)

    @pytest.mark.parametrize("nq,nelmt", fam.graph, ids=[case_id(s) + "-" + str(n) for s, n in fam.graph])
    def test_captured_graph_replay_matches_eager(sf, torch_mod, nq, nelmt):
        p = own_problem(fam, sf, torch_mod, nq, nelmt, F64, 11)
        for present in fam.modes:
            eager = p.run(sf, present=present)
            outs = [torch_mod.zeros_like(t) for t in eager]
            capture_replay(torch_mod, lambda side: p.run(sf, present=present, out=outs, stream=side))
            assert same_bits(torch_mod, outs, eager)
            assert all(float(o.abs().max()) > 0 for o in outs)
            p.check(outs, "graph", present=present)

    def test_first_call_inside_a_capture():
        """Capture-safe from the first call: a fresh child process whose first call of each route of the family (3D wave,
        3D fallback, 2D wave, 2D fallback) is inside a stream capture; the replay equals an eager call made afterwards."""
        script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "affine_deriv_first_call.py")
        r = subprocess.run([sys.executable, script, fam.name], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

    def test_two_streams_in_flight(sf, torch_mod):
        """Two problems enqueued on two streams before either is waited for; a seeded sample of elements and the ends
        against long double."""
        streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
        probs = [own_problem(fam, sf, torch_mod, nq, nelmt, F64, nelmt % 97) for nq, nelmt in fam.streams]
        torch_mod.cuda.synchronize()
        outs = []
        for p, st in zip(probs, streams):
            with torch_mod.cuda.stream(st):
                outs.append(p.run(sf, stream=st))
        torch_mod.cuda.synchronize()
        rng = np.random.default_rng(7)
        for p, o in zip(probs, outs):
            ends = [0, 1, p.nelmt - 2, p.nelmt - 1]
            sample = np.unique(np.concatenate((ends, rng.integers(0, p.nelmt, fam.stream_sample))))
            p.check_elements(o, "stream job", torch_mod.tensor(sample, device="cuda"), ld=fam.stream_ld)

    ns.update(test_refusals=test_refusals, test_captured_graph_replay_matches_eager=test_captured_graph_replay_matches_eager,
              test_first_call_inside_a_capture=test_first_call_inside_a_capture,
              test_two_streams_in_flight=test_two_streams_in_flight)
