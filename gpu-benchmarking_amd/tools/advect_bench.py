#!/usr/bin/env python3
"""Time the weak advection term (sf_advect_*, nf = d) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of
8 back-to-back launches, graph-replayed, mean and min per launch -- in `--repeats` repeats (default 2), each a row of its
own.  Default batch: 262 144 elements in 3D, 1 048 576 in 2D (the shapes and counts of physderiv_bench.py).

DOF are counted as nf * nelmt * nm^d; the roofline fraction uses the operator's own algorithmic bytes
sizeof(T) * nelmt * ((d^2 + d + 1) nq^d + 2 nf nm^d) against 8 TB/s.
--chain also times, in the same process on preallocated buffers, what a user writes without the fused kernel: per field
physderiv_* (which re-reads the d^2 planes of df), mul / addcmul with the planes of c, mul with w, iproduct_*.
--check prints max |fused - chain| / max |fused| of the two on the same data.

    python3 gpu-benchmarking_amd/tools/advect_bench.py [--chain] [--check] [--json FILE] [--hex 4,6,8] [--quad 8,12,16]
                                                       [--f32] [--repeats 2]
"""
import sys

import opbench
from opbench import chain_row, gdof_s, ms, roofline


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, w, c, x, out):
    """The unfused composition on preallocated buffers: returns a callable that leaves out_a in out[a]."""
    ext = (nq,) * dim
    npt = nq ** dim
    phys, ipr = (sf.physderiv_hex, sf.iproduct_hex) if dim == 3 else (sf.physderiv_quad, sf.iproduct_quad)
    grad = phys(ext, *bs, *ds, df, x[0])
    r = torch.empty(nelmt * npt, dtype=w.dtype, device=w.device)

    def chain():
        for a in range(dim):
            phys(ext, *bs, *ds, df, x[a], out=grad)
            torch.mul(c[0], grad[0], out=r)
            for j in range(1, dim):
                r.addcmul_(c[j], grad[j])
            r.mul_(w)
            ipr(ext, *bs, r, out=out[a])

    return chain


def case(s, c):
    torch, args, dim, nelmt = s.torch, s.args, c.dim, c.nelmt
    df = c.fill(nelmt * dim * dim * c.npt, 5)
    w = c.fill(nelmt * c.npt, 2)
    cv = c.fill(dim * nelmt * c.npt, 1).view(dim, nelmt * c.npt)
    x = c.fill(dim * nelmt * c.nmt, 6).view(dim, nelmt * c.nmt)
    adv = c.op("advect")
    o = adv(c.ext, *c.bs, *c.ds, df, w, cv, x, **c.kw)
    nbytes = c.nbytes("advect", nf=dim)
    chain = o2 = None
    if args.chain:
        o2 = torch.empty_like(o)
        chain = make_chain(torch, s.sf, dim, c.nq, nelmt, c.bs, c.ds, df, w, cv, x, o2)
    rows = []
    for rep in range(args.repeats):
        mean_ms, min_ms = s.timed(lambda: adv(c.ext, *c.bs, *c.ds, df, w, cv, x, out=o, **c.kw))
        row = {"repeat": rep, "t_advect": ms(mean_ms), "t_advect_min": ms(min_ms),
               "gdof_s": gdof_s(dim * nelmt * c.nmt, mean_ms), **roofline(nbytes, mean_ms, min_ms)}
        if chain is not None:
            row.update(chain_row(mean_ms, *s.timed(chain)))
        rows.append(row)
        print(f"advect {c.label}: {row}", flush=True)
    if chain is not None and args.check:
        rel = float((o - o2).abs().max() / o.abs().max())
        rows.append({"chain_rel_diff": rel})
        print(f"advect {c.label}: max |fused - chain| / max |fused| = {rel:.3g}", flush=True)
    return rows


def options(argv=None):
    ap = opbench.parser(__doc__, repeats=(2, None), chain="also time physderiv + torch ops + iproduct on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, nf = d, {args.repeats} repeats of {args.reps} "
                       "groups of 8 back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "advect": {}}
    s.collect(res["advect"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
