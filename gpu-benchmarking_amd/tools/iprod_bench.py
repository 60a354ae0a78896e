#!/usr/bin/env python3
"""Time IProductWRTBase (sf_iproduct_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8
back-to-back launches, graph-replayed, mean and min per launch -- at 1 048 576 elements.

DOF are counted as bench.py counts them, nelmt * nm^d, and the roofline fraction uses the same algorithmic bytes,
sizeof(T) * nelmt * (nm^d + nq^d) against 8 TB/s, so the fp64 rows compare directly with extra.hex_sweep and extra.quad
of `bench.py --full`.  --bwdtrans also times AUTO BwdTrans of every order in the same process (same data sizes).

    python3 gpu-benchmarking_amd/tools/iprod_bench.py [--json FILE] [--hex 2,...,11] [--quad 2,...,16] [--no-f32]
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
    ap.add_argument("--bwdtrans", action="store_true", help="also time AUTO BwdTrans of every order")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    nelmt = args.nelmt
    res = {"protocol": f"{nelmt} elements, {args.reps} groups of 8 back-to-back launches (bench.py grouped_ms); "
                       "frac = algorithmic bytes sizeof(T)*nelmt*(nm^d + nq^d) / mean time / 8 TB/s",
           "device": sf.device_info()["name"], "iproduct": {}, "bwdtrans": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([] if args.no_f32 else [("f32", torch.float32)])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        for dim, orders in ((3, args.hex), (2, args.quad)):
            for nq in orders:
                nm = nq - 1
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                bs = (b,) * dim
                nbytes = size * nelmt * (nm ** dim + nq ** dim)
                ops = [("iproduct", nq ** dim, nm ** dim,
                        (lambda x, o: sf.iproduct_hex((nq,) * 3, *bs, x, out=o)) if dim == 3 else
                        (lambda x, o: sf.iproduct_quad((nq,) * 2, *bs, x, out=o)))]
                if args.bwdtrans:
                    ops.append(("bwdtrans", nm ** dim, nq ** dim,
                                (lambda x, o: sf.bwdtrans_hex((nq,) * 3, *bs, x, out=o)) if dim == 3 else
                                (lambda x, o: sf.bwdtrans_quad((nq,) * 2, *bs, x, out=o))))
                for what, nin, nout, call in ops:
                    x = sf.fill_random(nelmt * nin, 1, dtype=dtype, device=dev)
                    o = torch.empty(nelmt * nout, dtype=dtype, device=dev)
                    mean_ms, min_ms, graphed = grouped_ms(torch, lambda: call(x, o), args.reps)
                    replayed = replayed and graphed
                    gbs_mean, gbs_min = nbytes / mean_ms * 1e-6, nbytes / min_ms * 1e-6
                    key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                    res[what].setdefault(key, {})[str(nq)] = {
                        "gdof_s": round(nelmt * nm ** dim / mean_ms * 1e-6, 2),
                        "gdof_s_min": round(nelmt * nm ** dim / min_ms * 1e-6, 2),
                        "gb_s": round(gbs_mean, 1), "frac_mean": round(gbs_mean / HBM_PEAK_GBS, 4),
                        "frac_min": round(gbs_min / HBM_PEAK_GBS, 4)}
                    print(f"{what:8s} {dim}D {tname} nq {nq:2d}: {res[what][key][str(nq)]}", flush=True)
                    del x, o
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
