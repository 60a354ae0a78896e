"""GPU tests that the fused families (sf_iproduct_*, sf_mass_*, sf_helmholtz_*, sf_affine_helmholtz_*, sf_physderiv_*,
sf_iprodderiv_*, sf_diag_helmholtz_*) have in common and that have one case per family or a few, written once over the
adapters of tests/fused_families.py: refusals, stream capture (also as a process's first call) and two streams in
flight.  An ID is the family's name in front of the ID the case had in the family's own file.  The common tests with
many cases per family are written once in tests/fused_common.py and keep their IDs in tests/test_gpu_<family>.py; what
a family's own mathematics asks is written there.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from fused_families import COMMON, F64, own_problem, sf, torch_mod  # noqa: F401
from multifield_common import _params, capture_replay, same_bits

pytestmark = pytest.mark.gpu


@_params("fam", ((f,) for f in COMMON if f.refused))
def test_refusals(sf, torch_mod, fam):
    """Extents outside the fallback's bounds, "wave" off the table, variants without a fused kernel: SF_ENOTBUILT."""
    for nq, nelmt, dtype_name, variant in fam.refused:
        p = own_problem(fam, sf, torch_mod, nq, nelmt, dtype_name, 2)
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, variant=variant)
        assert ei.value.rc == sf.capi.SF_ENOTBUILT, (nq, dtype_name, variant)


@_params("fam,nq,nelmt", ((f, s, n) for f in COMMON for s, n in f.graph))
def test_captured_graph_replay_matches_eager(sf, torch_mod, fam, nq, nelmt):
    p = own_problem(fam, sf, torch_mod, nq, nelmt, F64, 11)
    for present in fam.modes:
        eager = p.run(sf, present=present)
        outs = [torch_mod.zeros_like(t) for t in eager]
        capture_replay(torch_mod, lambda side: p.run(sf, present=present, out=outs, stream=side))
        assert same_bits(torch_mod, outs, eager)
        assert all(float(o.abs().max()) > 0 for o in outs)
        if fam.graph_bound:
            p.check(outs, "graph", present=present)


@_params("fam", ((f,) for f in COMMON))
def test_first_call_inside_a_capture(fam):
    """Capture-safe from the first call: a fresh child process whose first call of each route of the family (3D wave,
    3D fallback, 2D wave, 2D fallback) is inside a stream capture; the replay equals an eager call made afterwards."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "first_call_captured.py")
    r = subprocess.run([sys.executable, script, fam.name], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@_params("fam", ((f,) for f in COMMON))
def test_two_streams_in_flight(sf, torch_mod, fam):
    """Two problems enqueued on two streams before either is waited for; each against the reference the family's own
    file used: every element against the fp64 sweeps, or against long double, or a seeded sample against long double."""
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
        sample = None
        if fam.stream_sample:
            ends = [0, 1, p.nelmt - 2, p.nelmt - 1]
            sample = np.unique(np.concatenate((ends, rng.integers(0, p.nelmt, fam.stream_sample))))
            sample = torch_mod.tensor(sample, device="cuda")
        p.check_elements(o, "stream job", sample, ld=fam.stream_ld)
