#!/usr/bin/env python3
"""Time IProductWRTBase (sf_iproduct_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8
back-to-back launches, graph-replayed, mean and min per launch -- at 1 048 576 elements.

DOF are counted as bench.py counts them, nelmt * nm^d, and the roofline fraction uses the same algorithmic bytes,
sizeof(T) * nelmt * (nm^d + nq^d) against 8 TB/s, so the fp64 rows compare directly with extra.hex_sweep and extra.quad
of `bench.py --full`.  --bwdtrans also times AUTO BwdTrans of every order in the same process (same data sizes).

    python3 gpu-benchmarking_amd/tools/iprod_bench.py [--json FILE] [--hex 2,...,11] [--quad 2,...,16] [--no-f32]
"""
import sys

import opbench
from opbench import gdof_s, roofline


def case(s, c, res):
    ops = [("iproduct", c.npt, c.nmt)] + ([("bwdtrans", c.nmt, c.npt)] if s.args.bwdtrans else [])
    for what, nin, nout in ops:
        call = c.op(what)
        x = c.fill(c.nelmt * nin, 1)
        o = s.torch.empty(c.nelmt * nout, dtype=c.dtype, device=s.dev)
        mean_ms, min_ms = s.timed(lambda: call(c.ext, *c.bs, x, out=o))
        row = {"gdof_s": gdof_s(c.nelmt * c.nmt, mean_ms), "gdof_s_min": gdof_s(c.nelmt * c.nmt, min_ms),
               **roofline(c.nbytes(what), mean_ms, min_ms)}
        res[what].setdefault(c.key, {})[str(c.nq)] = row
        print(f"{what:8s} {c.label}: {row}", flush=True)
        del x, o


def options(argv=None):
    ap = opbench.parser(__doc__, nelmt="single", hex=(opbench.orders, list(range(2, 12))),
                        quad=(opbench.orders, list(range(2, 17))), f32="--no-f32", variant=None)
    ap.add_argument("--bwdtrans", action="store_true", help="also time AUTO BwdTrans of every order")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt} elements, {args.reps} groups of 8 back-to-back launches (bench.py grouped_ms); "
                       "frac = algorithmic bytes sizeof(T)*nelmt*(nm^d + nq^d) / mean time / 8 TB/s",
           "device": s.device_name, "iproduct": {}, "bwdtrans": {}}
    for c in s.sweep():
        case(s, c, res)
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
