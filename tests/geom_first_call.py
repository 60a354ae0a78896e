"""Child process of test_first_call_inside_a_capture of tests/test_gpu_geom.py: `python geom_first_call.py`.  The process's
first call of each route of the family (geom_families.FIRST_CALL: 3D wave, 3D fallback, 2D wave, 2D fallback) and then
of the affine kernel is made inside a stream capture; the replay must equal an eager call made afterwards."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from geom_families import FIRST_CALL, GeomProblem, same_bits  # noqa: E402

sf = ge.load_package()


def captured(call, like):
    outs = {k: torch.zeros_like(t) for k, t in like.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(outs, side)                                  # the process's first call of this route
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return outs


problems = []
for nq, nelmt in FIRST_CALL:
    p = GeomProblem(sf, torch, nq, nelmt, "float64", 40)      # nothing of the family has run
    per = {k: nelmt * p.per[k] for k in ("df", "w", "g", "detj")}
    like = {k: torch.empty(n, dtype=torch.float64, device="cuda") for k, n in per.items()}
    outs = captured(lambda o, s: p.run(out=o, stream=s), like)
    eager = p.run()
    torch.cuda.synchronize()
    assert same_bits(torch, outs, eager), nq
    assert all(float(o.abs().max()) > 0 for o in outs.values()), nq
    problems.append(p)

# the affine kernel allocates its own outputs: capture it through the C call's wrapper on a private memory pool
p = problems[0]
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
graph = torch.cuda.CUDAGraph()
with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
        got = p.run_affine(stream=side)
torch.cuda.current_stream().wait_stream(side)
graph.replay()
torch.cuda.synchronize()
eager = p.run_affine()
torch.cuda.synchronize()
assert same_bits(torch, got, eager) and float(got["je"].min()) > 0
print("first calls captured")
