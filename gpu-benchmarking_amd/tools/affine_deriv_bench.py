#!/usr/bin/env python3
"""Time the gradient and the weak divergence on affine elements (sf_aff_physderiv_*, sf_aff_iprodderiv_*) and, in
the same process, their deformed calls (sf_physderiv_*, sf_iprodderiv_*) on the planes expanded on the device from the same
dfe / je / qw, with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8 back-to-back launches,
graph-replayed, mean and min per launch.  Default batch: 262 144 elements in 3D, 1 048 576 in 2D, fp64; --repeats times
everything that often (a fresh measurement each time).

The roofline fraction of an affine call uses ITS algorithmic bytes against 8 TB/s: sizeof(T) * nelmt * (nm^d + d nq^d +
d*d) for the gradient, (d nq^d + nm^d + d*d + 1) for the weak divergence (--no-je: one scalar less, and the deformed call
runs without w).  `ratio` is t_deformed / t_affine, `ok` whether t_affine <= t_deformed.  --check compares the bits of the
two calls (the affine forms are bit for bit the deformed ones on expanded planes) and fails the run when they differ.

    python3 gpu-benchmarking_amd/tools/affine_deriv_bench.py [--check] [--repeats 2] [--json FILE] [--hex 4,6,8]
                                                             [--quad 8,12,16] [--f32] [--no-je] [--variant auto]
"""
import sys

import opbench
from opbench import scalars


def case(s, c, rep, table):
    """Both operators at one (dtype, dim, nq); returns whether every pair of outputs compared equal."""
    torch, args, dim, nelmt, npt, nq = s.torch, s.args, c.dim, c.nelmt, c.npt, c.nq
    qw = c.fill(nq, 6)
    bs, ds, qs, kw = c.bs, c.ds, (qw,) * dim, c.kw
    x = c.fill(nelmt * c.nmt, 1)
    f = c.fill(dim * nelmt * npt, 7).view(dim, -1)
    dfe = c.fill(nelmt * dim * dim, 5)
    je = None if args.no_je else c.fill(nelmt, 2)
    has_je = je is not None
    df, w = opbench.expand_affine(torch, dim, nelmt, npt, qw, dfe, je)        # the planes of the deformed calls
    apd, pd, aipd, ipd = c.op("affine_physderiv"), c.op("physderiv"), c.op("affine_iprodderiv"), c.op("iprodderiv")
    og, og2 = (torch.empty((dim, nelmt * npt), dtype=c.dtype, device=s.dev) for _ in range(2))
    om, om2 = (torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev) for _ in range(2))
    calls = {
        "gradient": (lambda: apd(c.ext, *bs, *ds, dfe, x, out=og, **kw),
                     lambda: pd(c.ext, *bs, *ds, df, x, out=og2, **kw),
                     scalars("affine_physderiv", dim, nq), scalars("physderiv", dim, nq), og, og2),
        "weak_divergence": (lambda: aipd(c.ext, *bs, *ds, *qs, dfe, je, f, out=om, **kw),
                            lambda: ipd(c.ext, *bs, *ds, df, w, f, out=om2, **kw),
                            scalars("affine_iprodderiv", dim, nq, je=has_je), scalars("iprodderiv", dim, nq, w=has_je),
                            om, om2)}
    bits_ok = True
    for op, call in calls.items():
        row = s.versus_deformed(c, *call)
        bits_ok = bits_ok and row.get("bits_equal", True)
        table.setdefault(f"{op}_{c.key}", {})[str(nq)] = row
        print(f"repeat {rep} {op} {c.label}: {row}", flush=True)
    return bits_ok


def options(argv=None):
    ap = opbench.parser(__doc__, repeats=(1, "measure everything this often"),
                        check="compare the bits of each affine call with its deformed call",
                        variant="fp64 route of every call: auto, wave or generic")
    ap.add_argument("--no-je", action="store_true", help="the weak divergence without weight (je = None, w = None)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = affine algorithmic bytes / time / 8 TB/s; ratio = deformed / affine",
           "device": s.device_name, "je": not args.no_je, "repeats": []}
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
