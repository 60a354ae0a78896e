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
    ap.add_argument("--repeats", type=int, default=1, help="measure everything this often")
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--check", action="store_true", help="compare the bits of the affine call with the deformed call")
    ap.add_argument("--variant", default="auto", help="fp64 route of every call: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge_
    sf = ge_.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, nf = d, {args.reps} groups of 8 back-to-back "
                       "launches (bench.py grouped_ms); frac = affine algorithmic bytes / time / 8 TB/s; ratio = deformed / "
                       "affine",
           "device": sf.device_info()["name"], "repeats": []}
    replayed, bits_ok = True, True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for rep in range(args.repeats):
        table = {}
        for tname, dtype in dtypes:
            size = torch.finfo(dtype).bits // 8
            kw = {"variant": args.variant} if dtype == torch.float64 else {}
            for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
                dd = dim * dim
                for nq in orders:
                    nm, ext, npt = nq - 1, (nq,) * dim, nq ** dim
                    nmt = nm ** dim
                    b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                    d = sf.fill_random(nq * nq, 4, dtype=dtype, device=dev)
                    qw = sf.fill_random(nq, 6, dtype=dtype, device=dev)
                    bs, ds, qs = (b,) * dim, (d,) * dim, (qw,) * dim
                    x = sf.fill_random(dim * nelmt * nmt, 1, dtype=dtype, device=dev).view(dim, -1)
                    c = sf.fill_random(dim * nelmt * npt, 7, dtype=dtype, device=dev).view(dim, -1)
                    dfe = sf.fill_random(nelmt * dd, 5, dtype=dtype, device=dev)
                    je = sf.fill_random(nelmt, 2, dtype=dtype, device=dev)
                    # the planes of the deformed call, expanded on the device in the working precision
                    df = dfe.view(nelmt, dd, 1).expand(nelmt, dd, npt).contiguous().reshape(-1)
                    q = qw
                    for _ in range(dim - 1):
                        q = torch.outer(qw, q.reshape(-1)).reshape(-1)          # qw_d * (the product so far)
                    w = (je.view(nelmt, 1) * q.view(1, -1)).reshape(-1).contiguous()
                    aadv, adv = ((sf.affine_advect_hex, sf.advect_hex) if dim == 3 else
                                 (sf.affine_advect_quad, sf.advect_quad))
                    oa, od = (torch.empty((dim, nelmt * nmt), dtype=dtype, device=dev) for _ in range(2))
                    a_sc = dim * npt + 2 * dim * nmt + dd + 1
                    d_sc = (dd + dim + 1) * npt + 2 * dim * nmt
                    a_mean, a_min, g0 = grouped_ms(torch, lambda: aadv(ext, *bs, *ds, *qs, dfe, je, c, x, out=oa, **kw),
                                                   args.reps)
                    d_mean, d_min, g1 = grouped_ms(torch, lambda: adv(ext, *bs, *ds, df, w, c, x, out=od, **kw), args.reps)
                    replayed = replayed and g0 and g1
                    abytes, dbytes = size * nelmt * a_sc, size * nelmt * d_sc
                    row = {"ms": round(a_mean, 5), "ms_min": round(a_min, 5), "scalars_per_element": a_sc,
                           "gb_s": round(abytes / a_mean * 1e-6, 1),
                           "frac_mean": round(abytes / a_mean * 1e-6 / HBM_PEAK_GBS, 4),
                           "frac_min": round(abytes / a_min * 1e-6 / HBM_PEAK_GBS, 4),
                           "ms_deformed": round(d_mean, 5), "ms_deformed_min": round(d_min, 5),
                           "deformed_scalars_per_element": d_sc,
                           "deformed_frac_mean": round(dbytes / d_mean * 1e-6 / HBM_PEAK_GBS, 4),
                           "ratio": round(d_mean / a_mean, 3), "ratio_min": round(d_min / a_min, 3),
                           "ok": bool(a_mean <= d_mean)}
                    if args.check:
                        torch.cuda.synchronize()
                        row["bits_equal"] = bool(torch.equal(oa, od)) and float(oa.abs().max()) > 0
                        bits_ok = bits_ok and row["bits_equal"]
                    table.setdefault(f"advect_{'hex' if dim == 3 else 'quad'}_{tname}", {})[str(nq)] = row
                    print(f"repeat {rep} advect {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                    del x, c, dfe, je, df, w, oa, od
                    torch.cuda.empty_cache()
        res["repeats"].append(table)
    res["hip_graph_replay"] = replayed
    res["all_ok"] = all(r["ok"] for t in res["repeats"] for k in t.values() for r in k.values())
    if args.check:
        res["bits_equal"] = bits_ok
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    return 0 if bits_ok else 1


if __name__ == "__main__":
    sys.exit(main())
