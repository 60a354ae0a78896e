"""Child process of test_first_call_inside_a_capture of tests/test_gpu_tensor.py: `python tensor_first_call.py`.  The
process's first call into the library is an AUTO sf_tensor_* call inside a stream capture -- a 3D shape of the compiled
table, then the first call of the any-extent kernel (a 2D shape off the table), each captured before it has ever run
eagerly; the replay must equal an eager call made afterwards."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from multifield_common import capture_replay  # noqa: E402

sf = ge.load_package()

for ni, no, trans, nelmt in (((4, 4, 4), (6, 6, 6), 0, 1001), ((9, 5), (3, 7), 1, 333)):
    rng = np.random.default_rng(len(ni))
    mats = [torch.from_numpy(rng.uniform(-1, 1, a * b)).cuda() for a, b in zip(ni, no)]
    x = torch.from_numpy(rng.uniform(-1, 1, nelmt * int(np.prod(ni)))).cuda()
    out = torch.zeros(nelmt * int(np.prod(no)), dtype=torch.float64, device="cuda")
    fn = sf.tensor_hex if len(ni) == 3 else sf.tensor_quad
    # the process's first call of this route
    capture_replay(torch, lambda side: fn(ni, no, *mats, x, trans=trans, out=out, stream=side))
    eager = fn(ni, no, *mats, x, trans=trans)
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and float(out.abs().max()) > 0, (ni, no)
print("first calls captured")
