"""Child process of test_first_call_inside_a_capture (tests/test_gpu_fused_common.py): `python first_call_captured.py
FAMILY`.  The process's first call of each route of the family (Family.first_call: 3D wave, 3D fallback, 2D wave, 2D
fallback) is made inside a stream capture; the replay must equal an eager call made afterwards.  A Problem as it stands:
nothing but sf.fill_random has run before the capture, so sf_diag_helmholtz_* builds its tables inside it as well."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from fused_families import BY_NAME, Problem  # noqa: E402
from multifield_common import capture_replay  # noqa: E402

fam = BY_NAME[sys.argv[1]]
sf = ge.load_package()
for nq, nelmt in fam.first_call:
    p = Problem(fam, sf, torch, nq, nelmt, "float64", 40)
    outs = [torch.zeros(nelmt * fam.out_per(nq), dtype=torch.float64, device="cuda") for _ in range(fam.out_parts(nq))]
    capture_replay(torch, lambda side: p.run(sf, out=outs, stream=side))      # the process's first call of this route
    eager = p.run(sf)
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(outs, eager)), nq
    assert all(float(o.abs().max()) > 0 for o in outs), nq
print("first calls captured")
