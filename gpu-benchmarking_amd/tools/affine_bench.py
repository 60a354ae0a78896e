#!/usr/bin/env python3
"""Time the fused Helmholtz operator on affine elements (sf_affine_helmholtz_*) and, in the same process, sf_helmholtz_*
on the planes g / w expanded from the same ge / je / qw, with the protocol of bench.py's extras(): grouped_ms -- 40 groups
of 8 back-to-back launches, graph-replayed, mean and min per launch.  Default batch: 262 144 elements in 3D, 1 048 576 in
2D, fp64.

The roofline fraction of the affine call uses ITS algorithmic bytes, sizeof(T) * nelmt * (2 nm^d + d(d+1)/2 + 1), against
8 TB/s (--laplacian: lambda = 0, je = None, one scalar less; the deformed call then runs without w); `ratio` is
t_deformed / t_affine, `ok` whether t_affine <= t_deformed.  --mass also times sf_mass_* on the expanded w for context.

    python3 gpu-benchmarking_amd/tools/affine_bench.py [--mass] [--laplacian] [--json FILE] [--hex 4,6,8] [--quad 8,12,16]
                                                       [--f32] [--no-deformed]
"""
import sys

import opbench
from opbench import frac, fracs, gdof_s, ms, roofline, scalars


def case(s, c, lam):
    torch, args, dim, nelmt, npt = s.torch, s.args, c.dim, c.nelmt, c.npt
    ncomp = dim * (dim + 1) // 2
    qw = c.fill(c.nq, 6)
    qs = (qw,) * dim
    x = c.fill(nelmt * c.nmt, 1)
    ge = c.fill(nelmt * ncomp, 5)
    je = None if args.laplacian else c.fill(nelmt, 2)
    o = torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    aff, helm, mass = c.op("affine_helmholtz"), c.op("helmholtz"), c.op("mass")
    a_sc = scalars("affine_helmholtz", dim, c.nq, je=not args.laplacian)
    d_sc = scalars("affine_helmholtz_deformed", dim, c.nq, je=not args.laplacian)
    abytes, dbytes = c.size * nelmt * a_sc, c.size * nelmt * d_sc
    a_mean, a_min = s.timed(lambda: aff(c.ext, *c.bs, *c.ds, *qs, ge, je, lam, x, out=o, **c.kw))
    row = {"ms": ms(a_mean), "ms_min": ms(a_min), "gdof_s": gdof_s(nelmt * c.nmt, a_mean), "scalars_per_element": a_sc,
           **roofline(abytes, a_mean, a_min)}
    w = None
    if args.mass or not (args.no_deformed or args.laplacian):   # lambda = 0 without --mass: nobody reads a point array w
        w = opbench.expand_affine(torch, dim, nelmt, npt, qw, je=c.fill(nelmt, 2) if je is None else je)[1]
    if not args.no_deformed:
        g = torch.empty(nelmt * ncomp * npt, dtype=c.dtype, device=s.dev)
        torch.mul(ge.view(nelmt, ncomp, 1), opbench.point_weights(torch, dim, qw).view(1, 1, -1),
                  out=g.view(nelmt, ncomp, npt))
        wd = None if args.laplacian else w
        o2 = torch.empty_like(o)
        d_mean, d_min = s.timed(lambda: helm(c.ext, *c.bs, *c.ds, g, wd, lam, x, out=o2, **c.kw))
        row.update({"ms_deformed": ms(d_mean), "ms_deformed_min": ms(d_min), "deformed_scalars_per_element": d_sc,
                    "deformed_frac_mean": frac(dbytes, d_mean), "ratio": round(d_mean / a_mean, 3),
                    "ratio_min": round(d_min / a_min, 3), "ok": bool(a_mean <= d_mean),
                    "rel_diff": float((o - o2).abs().max() / o.abs().max())})
        del g, o2
    if args.mass:
        m_mean, m_min = s.timed(lambda: mass(c.ext, *c.bs, w, x, out=o))
        row.update({"ms_mass": ms(m_mean), **fracs("mass", c.nbytes("mass"), m_mean, m_min)})
    print(f"affine {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, variant="fp64 route of both calls: auto, wave or generic")
    ap.add_argument("--laplacian", action="store_true", help="lambda = 0, je = None")
    ap.add_argument("--mass", action="store_true", help="also time sf_mass_* on the expanded w")
    ap.add_argument("--no-deformed", action="store_true", help="the affine call only (no expanded planes are allocated)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    lam = 0.0 if args.laplacian else 0.75
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = affine algorithmic bytes / time / 8 TB/s; ratio = deformed / affine",
           "device": s.device_name, "lambda": lam, "affine": {}}
    s.collect(res["affine"], lambda c: case(s, c, lam))
    s.emit(res, all_ok=all(r.get("ok", True) for t in res["affine"].values() for r in t.values()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
