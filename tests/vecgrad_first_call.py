"""Child process of test_first_call_inside_a_capture of tests/test_gpu_vecgrad.py: `python vecgrad_first_call.py`.  The
process's first call of each route of the family (vecgrad_families.FIRST_CALL: 3D wave, 3D fallback, 2D wave, 2D
fallback) is made inside a stream capture; the replay must equal an eager call made afterwards."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from vecgrad_families import FIRST_CALL, VecgradProblem, per_element, rows, same_outputs  # noqa: E402

sf = ge.load_package()


def captured(p):
    per, ncurl = per_element(p.nq)
    n = p.nelmt
    out = {"grad": torch.zeros(n * per["grad"], dtype=p.dtype, device="cuda"),
           "div": torch.zeros(n * per["div"], dtype=p.dtype, device="cuda"),
           "curl": rows(torch, ncurl, n * per["curl"], p.dtype, fill=0.0) if ncurl > 1
           else torch.zeros(n * per["curl"], dtype=p.dtype, device="cuda")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            p.run(out=out, stream=side)                       # the process's first call of this route
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return out


for nq, nelmt in FIRST_CALL:
    p = VecgradProblem(sf, torch, nq, nelmt, "float64", 40)   # no operator of the family has run on this route
    out = captured(p)
    eager = p.run()
    torch.cuda.synchronize()
    assert same_outputs(torch, out, eager), nq
    assert all(float(t.abs().max()) > 0 for t in out.values()), nq
print("first calls captured")
