"""Child process of test_first_call_inside_a_capture_and_eager of tests/test_gpu_affine_advect.py:
`python affine_advect_first_call.py captured|eager`.  The process's first call of the library's operators is the affine
advection call: "captured" makes the first call of each route of the family (affine_advect_families.FIRST_CALL: 3D wave,
3D fallback, 2D wave, 2D fallback), with d fields and then with one, inside a stream capture, and the replay must equal
an eager call made afterwards; "eager" makes them eagerly.  Either way the result must equal the deformed call on the
expanded planes, which runs after it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from affine_advect_families import FIRST_CALL, AffineAdvectProblem, rows, same_bits  # noqa: E402

sf = ge.load_package()
mode = sys.argv[1]
assert mode in ("captured", "eager")


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
    p = AffineAdvectProblem(sf, torch, nq, nelmt, "float64", 40)    # fills and torch only: no operator has run
    for field in (None, 0):
        parts = p.d if field is None else 1
        if mode == "captured":
            out = captured(lambda o, s: p.run(field=field, out=o, stream=s), parts, nelmt * p.nmt)
        else:
            out = p.run(field=field)
        eager = p.run(field=field)
        torch.cuda.synchronize()
        assert same_bits(torch, out, eager), (nq, field)
        assert same_bits(torch, out, p.deformed(field=field)), (nq, field)
        assert float(out.abs().max()) > 0, (nq, field)
print(f"first calls {mode}")
