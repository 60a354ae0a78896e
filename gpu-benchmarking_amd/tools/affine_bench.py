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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())


def _orders(s):
    return [int(x) for x in s.split(",") if x]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--laplacian", action="store_true", help="lambda = 0, je = None")
    ap.add_argument("--mass", action="store_true", help="also time sf_mass_* on the expanded w")
    ap.add_argument("--no-deformed", action="store_true", help="the affine call only (no expanded planes are allocated)")
    ap.add_argument("--variant", default="auto", help="fp64 route of both calls: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge_
    sf = ge_.load_package()
    dev = torch.device("cuda:0")
    lam = 0.0 if args.laplacian else 0.75
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = affine algorithmic bytes / time / 8 TB/s; ratio = deformed / affine",
           "device": sf.device_info()["name"], "lambda": lam, "affine": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            ncomp = dim * (dim + 1) // 2
            for nq in orders:
                nm, ext, npt = nq - 1, (nq,) * dim, nq ** dim
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                d = sf.fill_random(nq * nq, 4, dtype=dtype, device=dev)
                qw = sf.fill_random(nq, 6, dtype=dtype, device=dev)
                bs, ds, qs = (b,) * dim, (d,) * dim, (qw,) * dim
                x = sf.fill_random(nelmt * nm ** dim, 1, dtype=dtype, device=dev)
                ge = sf.fill_random(nelmt * ncomp, 5, dtype=dtype, device=dev)
                je = None if args.laplacian else sf.fill_random(nelmt, 2, dtype=dtype, device=dev)
                o = torch.empty(nelmt * nm ** dim, dtype=dtype, device=dev)
                aff, helm, mass = ((sf.affine_helmholtz_hex, sf.helmholtz_hex, sf.mass_hex) if dim == 3 else
                                   (sf.affine_helmholtz_quad, sf.helmholtz_quad, sf.mass_quad))
                consts = ncomp + (0 if args.laplacian else 1)
                abytes = size * nelmt * (2 * nm ** dim + consts)
                dbytes = size * nelmt * (2 * nm ** dim + consts * npt)

                def frac(nb, ms):
                    return round(nb / ms * 1e-6 / HBM_PEAK_GBS, 4)

                a_mean, a_min, g0 = grouped_ms(torch, lambda: aff(ext, *bs, *ds, *qs, ge, je, lam, x, out=o, **kw),
                                               args.reps)
                replayed = replayed and g0
                row = {"ms": round(a_mean, 5), "ms_min": round(a_min, 5),
                       "gdof_s": round(nelmt * nm ** dim / a_mean * 1e-6, 2), "scalars_per_element": 2 * nm ** dim + consts,
                       "gb_s": round(abytes / a_mean * 1e-6, 1), "frac_mean": frac(abytes, a_mean),
                       "frac_min": frac(abytes, a_min)}
                if not args.no_deformed or args.mass:
                    q = qw
                    for _ in range(dim - 1):
                        q = torch.outer(qw, q.reshape(-1)).reshape(-1)
                    w = None
                    if args.mass or not args.laplacian:     # lambda = 0 without --mass: nobody reads a point array w
                        w = (sf.fill_random(nelmt, 2, dtype=dtype, device=dev) if je is None else je).view(nelmt, 1)
                        w = (w * q.view(1, -1)).reshape(-1)
                if not args.no_deformed:
                    g = torch.empty(nelmt * ncomp * npt, dtype=dtype, device=dev)
                    torch.mul(ge.view(nelmt, ncomp, 1), q.view(1, 1, -1), out=g.view(nelmt, ncomp, npt))
                    wd = None if args.laplacian else w
                    o2 = torch.empty_like(o)
                    d_mean, d_min, g1 = grouped_ms(torch, lambda: helm(ext, *bs, *ds, g, wd, lam, x, out=o2, **kw),
                                                   args.reps)
                    replayed = replayed and g1
                    row.update({"ms_deformed": round(d_mean, 5), "ms_deformed_min": round(d_min, 5),
                                "deformed_scalars_per_element": 2 * nm ** dim + consts * npt,
                                "deformed_frac_mean": frac(dbytes, d_mean), "ratio": round(d_mean / a_mean, 3),
                                "ratio_min": round(d_min / a_min, 3), "ok": bool(a_mean <= d_mean),
                                "rel_diff": float((o - o2).abs().max() / o.abs().max())})
                    del g, o2
                if args.mass:
                    m_mean, m_min, g2 = grouped_ms(torch, lambda: mass(ext, *bs, w, x, out=o), args.reps)
                    replayed = replayed and g2
                    mb = size * nelmt * (2 * nm ** dim + npt)
                    row.update({"ms_mass": round(m_mean, 5), "mass_frac_mean": frac(mb, m_mean),
                                "mass_frac_min": frac(mb, m_min)})
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["affine"].setdefault(key, {})[str(nq)] = row
                print(f"affine {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del x, ge, je, o
                w = q = None
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    res["all_ok"] = all(r.get("ok", True) for t in res["affine"].values() for r in t.values())
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
