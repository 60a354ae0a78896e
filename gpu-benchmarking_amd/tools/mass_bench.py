#!/usr/bin/env python3
"""Time the fused mass operator (sf_mass_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8
back-to-back launches, graph-replayed, mean and min per launch -- at 1 048 576 elements.

DOF are counted as nelmt * nm^d; the roofline fraction uses the fused algorithmic bytes sizeof(T) * nelmt * (2 nm^d + nq^d)
against 8 TB/s.  --chain also times, in the same process on the same buffers, the three-launch composition it replaces
(bwdtrans_*, an in-place torch.mul by w, iproduct_*) and prints the speed-up; ms_bwd_plus_iprod is the part of the chain
that is this library's own two kernels (tools/iprod_bench.py --bwdtrans times the same two on their own).

    python3 gpu-benchmarking_amd/tools/mass_bench.py [--chain] [--json FILE] [--hex 2,...,11] [--quad 2,...,16] [--no-f32]
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
    ap.add_argument("--nelmt", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hex", type=_orders, default=list(range(2, 12)))
    ap.add_argument("--quad", type=_orders, default=list(range(2, 17)))
    ap.add_argument("--no-f32", action="store_true", help="fp64 only")
    ap.add_argument("--chain", action="store_true", help="also time bwdtrans, torch.mul, iproduct on the same buffers")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    nelmt = args.nelmt
    res = {"protocol": f"{nelmt} elements, {args.reps} groups of 8 back-to-back launches (bench.py grouped_ms); "
                       "frac = algorithmic bytes sizeof(T)*nelmt*(2 nm^d + nq^d) / mean time / 8 TB/s",
           "device": sf.device_info()["name"], "mass": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([] if args.no_f32 else [("f32", torch.float32)])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders in ((3, args.hex), (2, args.quad)):
            for nq in orders:
                nm, ext = nq - 1, (nq,) * dim
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                bs = (b,) * dim
                x = sf.fill_random(nelmt * nm ** dim, 1, dtype=dtype, device=dev)
                w = 0.25 + sf.fill_random(nelmt * nq ** dim, 2, dtype=dtype, device=dev).abs()
                o = torch.empty(nelmt * nm ** dim, dtype=dtype, device=dev)
                mass, bwd, ipr = ((sf.mass_hex, sf.bwdtrans_hex, sf.iproduct_hex) if dim == 3 else
                                  (sf.mass_quad, sf.bwdtrans_quad, sf.iproduct_quad))
                nbytes = size * nelmt * (2 * nm ** dim + nq ** dim)
                mean_ms, min_ms, graphed = grouped_ms(torch, lambda: mass(ext, *bs, w, x, out=o, **kw), args.reps)
                replayed = replayed and graphed
                row = {"ms": round(mean_ms, 5), "ms_min": round(min_ms, 5),
                       "gdof_s": round(nelmt * nm ** dim / mean_ms * 1e-6, 2),
                       "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                       "frac_mean": round(nbytes / mean_ms * 1e-6 / HBM_PEAK_GBS, 4),
                       "frac_min": round(nbytes / min_ms * 1e-6 / HBM_PEAK_GBS, 4)}
                if args.chain:
                    pts = torch.empty(nelmt * nq ** dim, dtype=dtype, device=dev)

                    def chain():
                        bwd(ext, *bs, x, out=pts)
                        torch.mul(pts, w, out=pts)
                        ipr(ext, *bs, pts, out=o)

                    c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                    b_mean, _, g2 = grouped_ms(torch, lambda: bwd(ext, *bs, x, out=pts), args.reps)
                    i_mean, _, g3 = grouped_ms(torch, lambda: ipr(ext, *bs, pts, out=o), args.reps)
                    replayed = replayed and g1 and g2 and g3
                    row.update({"ms_chain": round(c_mean, 5), "speedup_vs_chain": round(c_mean / mean_ms, 3),
                                "ms_bwd": round(b_mean, 5), "ms_iprod": round(i_mean, 5),
                                "ms_bwd_plus_iprod": round(b_mean + i_mean, 5),
                                "ratio_to_bwd_plus_iprod": round(mean_ms / (b_mean + i_mean), 4)})
                    del pts
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["mass"].setdefault(key, {})[str(nq)] = row
                print(f"mass {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del x, w, o
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
