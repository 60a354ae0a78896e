#!/usr/bin/env python3
"""Time the weak advection term on affine elements (sf_aff_advect_*, nf = d) and, in the same process on the same buffers,
the deformed call (sf_advect_*) on the planes expanded on the device from the same dfe / je / qw, with the protocol of
bench.py's extras(): grouped_ms -- 40 groups of 8 back-to-back launches, graph-replayed, mean and min per launch.  Default
batch: 262 144 elements in 3D, 1 048 576 in 2D, fp64; --repeats times everything that often (a fresh measurement each
time).

The roofline fraction of the affine call uses ITS algorithmic bytes against 8 TB/s: sizeof(T) * nelmt * (d nq^d + 2 d nm^d
+ d*d + 1).  `ratio` is t_deformed / t_affine, `ok` whether t_affine <= t_deformed.  --check compares the bits of the two
calls (the affine form is bit for bit the deformed one on expanded planes) and fails the run when they differ.

    python3 gpu-benchmarking_amd/tools/affine_advect_bench.py [--check] [--repeats 2] [--json FILE] [--hex 4,6,8]
                                                              [--quad 8,12,16] [--f32] [--variant auto]
"""
import sys

import opbench
from opbench import scalars


def case(s, c, rep, table):
    """The affine and the deformed call at one (dtype, dim, nq); returns whether their outputs compared equal."""
    torch, dim, nelmt, npt, nq = s.torch, c.dim, c.nelmt, c.npt, c.nq
    qw = c.fill(nq, 6)
    bs, ds, qs, kw = c.bs, c.ds, (qw,) * dim, c.kw
    x = c.fill(dim * nelmt * c.nmt, 1).view(dim, -1)
    cv = c.fill(dim * nelmt * npt, 7).view(dim, -1)
    dfe = c.fill(nelmt * dim * dim, 5)
    je = c.fill(nelmt, 2)
    df, w = opbench.expand_affine(torch, dim, nelmt, npt, qw, dfe, je)        # the planes of the deformed call
    aadv, adv = c.op("affine_advect"), c.op("advect")
    oa, od = (torch.empty((dim, nelmt * c.nmt), dtype=c.dtype, device=s.dev) for _ in range(2))
    row = s.versus_deformed(c, lambda: aadv(c.ext, *bs, *ds, *qs, dfe, je, cv, x, out=oa, **kw),
                            lambda: adv(c.ext, *bs, *ds, df, w, cv, x, out=od, **kw),
                            scalars("affine_advect", dim, nq), scalars("advect", dim, nq, nf=dim), oa, od)
    table.setdefault(f"advect_{c.key}", {})[str(nq)] = row
    print(f"repeat {rep} advect {c.label}: {row}", flush=True)
    return row.get("bits_equal", True)


def options(argv=None):
    ap = opbench.parser(__doc__, repeats=(1, "measure everything this often"),
                        check="compare the bits of the affine call with the deformed call",
                        variant="fp64 route of every call: auto, wave or generic")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, nf = d, {args.reps} groups of 8 back-to-back "
                       "launches (bench.py grouped_ms); frac = affine algorithmic bytes / time / 8 TB/s; ratio = deformed / "
                       "affine",
           "device": s.device_name, "repeats": []}
    bits_ok = True
    for rep in range(args.repeats):
        table = {}
        for c in s.sweep():
            bits_ok = case(s, c, rep, table) and bits_ok
        res["repeats"].append(table)
    s.emit(res, all_ok=all(r["ok"] for t in res["repeats"] for k in t.values() for r in k.values()),
           **({"bits_equal": bits_ok} if args.check else {}))
    return 0 if bits_ok else 1


if __name__ == "__main__":
    sys.exit(main())
