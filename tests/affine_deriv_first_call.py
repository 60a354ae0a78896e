"""Child process of test_first_call_inside_a_capture of tests/test_gpu_affine_physderiv.py and
tests/test_gpu_affine_iprodderiv.py: `python affine_deriv_first_call.py FAMILY`, tests/first_call_captured.py for the two
families of tests/affine_deriv_families.py.  The process's first call of each route of the family (Family.first_call: 3D
wave, 3D fallback, 2D wave, 2D fallback) is made inside a stream capture; the replay must equal an eager call made
afterwards."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from affine_deriv_families import BY_NAME  # noqa: E402
from fused_families import own_problem  # noqa: E402
from multifield_common import capture_replay  # noqa: E402

fam = BY_NAME[sys.argv[1]]
sf = ge.load_package()
for nq, nelmt in fam.first_call:
    p = own_problem(fam, sf, torch, nq, nelmt, "float64", 40)              # nothing but sf.fill_random has run
    outs = [torch.zeros(nelmt * fam.out_per(nq), dtype=torch.float64, device="cuda") for _ in range(fam.out_parts(nq))]
    capture_replay(torch, lambda side: p.run(sf, out=outs, stream=side))      # the process's first call of this route
    eager = p.run(sf)
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(outs, eager)), nq
    assert all(float(o.abs().max()) > 0 for o in outs), nq
print("first calls captured")
