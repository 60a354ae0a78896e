#!/usr/bin/env python3
"""Time the fused mass operator (sf_mass_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8
back-to-back launches, graph-replayed, mean and min per launch -- at 1 048 576 elements.

DOF are counted as nelmt * nm^d; the roofline fraction uses the fused algorithmic bytes sizeof(T) * nelmt * (2 nm^d + nq^d)
against 8 TB/s.  --chain also times, in the same process on the same buffers, the three-launch composition it replaces
(bwdtrans_*, an in-place torch.mul by w, iproduct_*) and prints the speed-up; ms_bwd_plus_iprod is the part of the chain
that is this library's own two kernels (tools/iprod_bench.py --bwdtrans times the same two on their own).

    python3 gpu-benchmarking_amd/tools/mass_bench.py [--chain] [--json FILE] [--hex 2,...,11] [--quad 2,...,16] [--no-f32]
"""
import sys

import opbench
from opbench import gdof_s, ms, roofline


def case(s, c):
    torch, args, nelmt = s.torch, s.args, c.nelmt
    x = c.fill(nelmt * c.nmt, 1)
    w = 0.25 + c.fill(nelmt * c.npt, 2).abs()
    o = torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    mass, bwd, ipr = c.op("mass"), c.op("bwdtrans"), c.op("iproduct")
    mean_ms, min_ms = s.timed(lambda: mass(c.ext, *c.bs, w, x, out=o, **c.kw))
    row = {"ms": ms(mean_ms), "ms_min": ms(min_ms), "gdof_s": gdof_s(nelmt * c.nmt, mean_ms),
           **roofline(c.nbytes("mass"), mean_ms, min_ms)}
    if args.chain:
        pts = torch.empty(nelmt * c.npt, dtype=c.dtype, device=s.dev)

        def chain():
            bwd(c.ext, *c.bs, x, out=pts)
            torch.mul(pts, w, out=pts)
            ipr(c.ext, *c.bs, pts, out=o)

        c_mean, _ = s.timed(chain)
        b_mean, _ = s.timed(lambda: bwd(c.ext, *c.bs, x, out=pts))
        i_mean, _ = s.timed(lambda: ipr(c.ext, *c.bs, pts, out=o))
        row.update({"ms_chain": ms(c_mean), "speedup_vs_chain": round(c_mean / mean_ms, 3),
                    "ms_bwd": ms(b_mean), "ms_iprod": ms(i_mean), "ms_bwd_plus_iprod": ms(b_mean + i_mean),
                    "ratio_to_bwd_plus_iprod": round(mean_ms / (b_mean + i_mean), 4)})
    print(f"mass {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, nelmt="single", hex=(opbench.orders, list(range(2, 12))),
                        quad=(opbench.orders, list(range(2, 17))), f32="--no-f32",
                        chain="also time bwdtrans, torch.mul, iproduct on the same buffers")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt} elements, {args.reps} groups of 8 back-to-back launches (bench.py grouped_ms); "
                       "frac = algorithmic bytes sizeof(T)*nelmt*(2 nm^d + nq^d) / mean time / 8 TB/s",
           "device": s.device_name, "mass": {}}
    s.collect(res["mass"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
