"""GPU tests that the multi-field families (sf_geom_*, sf_advect_*, sf_aff_advect_*, sf_vecgrad_*) have in common, written
once over the MultiField adapters of tests/multifield_common.py, in the manner of tests/test_gpu_fused_common.py: the
SF_ENOTBUILT refusals, stream capture (also as a process's first call) and two streams in flight.  An ID is the family's
name in front of the ID the case had in the family's own file.  What a family's own mathematics or its own C signature
asks is written in tests/test_gpu_<family>.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from fused_families import F64, sf, torch_mod  # noqa: F401
from multifield_common import _params, capture_replay, families, leaves, same_bits

pytestmark = pytest.mark.gpu
FAMILIES = families()


@_params("fam", ((f,) for f in FAMILIES))
def test_not_built_refusals(sf, torch_mod, fam):
    """Extents outside the fallback's bounds, "wave" off the table, variants without a kernel of the family:
    SF_ENOTBUILT from every form of the call."""
    for nq, nelmt, dtype_name, variant in fam.refused:
        p = fam.problem(sf, torch_mod, nq, nelmt, dtype_name, 2)
        for call in fam.refused_calls(p, variant):
            with pytest.raises(sf.capi.SumfactError) as ei:
                call()
            assert ei.value.rc == sf.capi.SF_ENOTBUILT, (nq, dtype_name, variant)


@_params("fam,nq,nelmt", ((f, s, n) for f in FAMILIES for s, n in f.graph))
def test_captured_graph_replay_matches_eager(sf, torch_mod, fam, nq, nelmt):
    p = fam.problem(sf, torch_mod, nq, nelmt, F64, 11)
    for mode in fam.graph_modes:
        eager = p.run(**mode)
        out = fam.zeros(p, **mode)
        capture_replay(torch_mod, lambda side: p.run(out=out, stream=side, **mode))
        assert same_bits(torch_mod, out, eager)
        assert all(float(t.abs().max()) > 0 for t in leaves(out))
    p.check(out, "graph", elements=[0, 1, nelmt // 2, nelmt - 1], **fam.graph_check)


@_params("fam", ((f,) for f in FAMILIES))
def test_first_call_inside_a_capture(fam):
    """Capture-safe from the first call: a fresh child process whose first call of each route of the family (3D wave, 3D
    fallback, 2D wave, 2D fallback; for sf_geom_* then the affine kernel) is inside a stream capture; the replay equals an
    eager call made afterwards.  sf_aff_advect_* also in a second child that makes them eagerly."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multifield_first_call.py")
    for mode in ("captured", "eager") if fam.first_eager else ("captured",):
        r = subprocess.run([sys.executable, script, fam.name, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"first calls {mode}" in r.stdout, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@_params("fam", ((f,) for f in FAMILIES))
def test_two_streams_in_flight(sf, torch_mod, fam):
    """Two problems enqueued on two streams before either is waited for; a seeded sample of elements and the ends against
    long double."""
    streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
    probs = [fam.problem(sf, torch_mod, nq, nelmt, F64, fam.stream_seed(k, nelmt)) for k, (nq, nelmt) in enumerate(fam.streams)]
    torch_mod.cuda.synchronize()
    outs = []
    for p, st in zip(probs, streams):
        with torch_mod.cuda.stream(st):
            outs.append(p.run(stream=st))
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(7)
    for p, o in zip(probs, outs):
        ends = [0, 1, p.nelmt - 2, p.nelmt - 1]
        sample = np.unique(np.concatenate((ends, rng.integers(0, p.nelmt, fam.stream_sample))))
        p.check(o, "stream job", elements=sample)
    if fam.streams_differ:
        assert not same_bits(torch_mod, outs[0], outs[1])
