"""Child process of test_first_call_inside_a_capture of tests/test_gpu_advect.py: `python advect_first_call.py`.  The
process's first call of each route of the family (advect_families.FIRST_CALL: 3D wave, 3D fallback, 2D wave, 2D fallback),
with d fields and then with one, is made inside a stream capture; the replay must equal an eager call made afterwards."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from advect_families import FIRST_CALL, AdvectProblem, rows, same_bits  # noqa: E402

sf = ge.load_package()


def captured(call, parts, n):
    out = rows(torch, parts, n, torch.float64, fill=0.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(out, side)                                   # the process's first call of this route
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return out


for nq, nelmt in FIRST_CALL:
    p = AdvectProblem(sf, torch, nq, nelmt, "float64", 40)    # no operator of the family has run on this route
    for field in (None, 0):
        parts = p.d if field is None else 1
        out = captured(lambda o, s: p.run(field=field, out=o, stream=s), parts, nelmt * p.nmt)
        eager = p.run(field=field)
        torch.cuda.synchronize()
        assert same_bits(torch, out, eager), (nq, field)
        assert float(out.abs().max()) > 0, (nq, field)
print("first calls captured")
