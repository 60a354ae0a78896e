"""Child process of test_first_call_inside_a_capture (tests/test_gpu_multifield_common.py): `python
multifield_first_call.py FAMILY [captured|eager]`.  "captured": the process's first call of each route of the family
(MultiField.first_call: 3D wave, 3D fallback, 2D wave, 2D fallback), in each of MultiField.first_modes, is made inside a
stream capture, and the replay must equal an eager call made afterwards; then what MultiField.first_tail adds.  "eager",
for the families that have it: the first calls are made eagerly.  A problem as it stands: fills and torch only have run
before the first call."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from multifield_common import capture_replay, families, leaves, same_bits  # noqa: E402

fam = {f.name: f for f in families()}[sys.argv[1]]
how = sys.argv[2] if len(sys.argv) > 2 else "captured"
assert how in (("captured", "eager") if fam.first_eager else ("captured",))
sf = ge.load_package()
problems = []
for nq, nelmt in fam.first_call:
    p = fam.problem(sf, torch, nq, nelmt, "float64", 40)      # no operator of the family has run on this route
    for mode in fam.first_modes:
        if how == "captured":
            out = fam.zeros(p, **mode)
            capture_replay(torch, lambda side: p.run(out=out, stream=side, **mode))   # the process's first call of this route
        else:
            out = p.run(**mode)
        eager = p.run(**mode)
        torch.cuda.synchronize()
        assert same_bits(torch, out, eager), (nq, mode)
        assert fam.first_also is None or fam.first_also(p, out, **mode), (nq, mode)
        assert all(float(t.abs().max()) > 0 for t in leaves(out)), (nq, mode)
    problems.append(p)
if fam.first_tail:
    fam.first_tail(torch, problems)
print(f"first calls {how}")
