#!/usr/bin/env python3
"""Time BwdTrans fused with the physical-space gradient (sf_physderiv_*) with the protocol of bench.py's extras():
grouped_ms -- 40 groups of 8 back-to-back launches, graph-replayed, mean and min per launch.  Default batch: 262 144
elements in 3D, 1 048 576 in 2D (the nine planes of df of a 3D nq 8 batch are then 9.7 GB).

DOF are counted as nelmt * nm^d; the roofline fraction uses the operator's own algorithmic bytes
sizeof(T) * nelmt * (nm^d + (d^2 + d) nq^d) against 8 TB/s; the reference-space case (df=None, nm^d + d nq^d) is timed in
the same session, and so are sf_helmholtz_* (lambda = 0.75, its bytes 2 nm^d + (1 + d(d+1)/2) nq^d) and BwdTrans
(nm^d + nq^d) for context.
--chain also times, in the same process on preallocated buffers, what a user can write without the fused kernel:
bwdtrans_*, then torch.matmul for every D_a, then mul / addcmul with the planes of df.  --check prints
max |fused - chain| / max |fused| over all outputs.

    python3 gpu-benchmarking_amd/tools/physderiv_bench.py [--chain] [--check] [--json FILE] [--hex 4,6,8]
                                                          [--quad 8,12,16] [--f32]
"""
import sys

import opbench
from opbench import chain_row, fracs, gdof_s, ms, roofline


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, x, outs):
    """The unfused composition on preallocated buffers: returns a callable that leaves the result in `outs`."""
    ext = (nq,) * dim
    npt = nq ** dim
    bwd = sf.bwdtrans_hex if dim == 3 else sf.bwdtrans_quad
    new = lambda: torch.empty(nelmt * npt, dtype=x.dtype, device=x.device)      # noqa: E731
    u = new()
    du = [new() for _ in range(dim)]
    dp = df.view(nelmt, dim * dim, npt)
    deriv = opbench.ref_derivs(torch, dim, nq, nelmt, ds)

    def chain():
        bwd(ext, *bs, x, out=u)
        deriv(u, du)
        for a in range(dim):
            oa = outs[a].view(nelmt, npt)
            torch.mul(dp[:, a * dim], du[0].view(nelmt, npt), out=oa)
            for b in range(1, dim):
                oa.addcmul_(dp[:, a * dim + b], du[b].view(nelmt, npt))

    return chain


def case(s, c):
    torch, args, dim, nelmt = s.torch, s.args, c.dim, c.nelmt
    x = c.fill(nelmt * c.nmt, 1)
    df = c.fill(nelmt * dim * dim * c.npt, 5)
    phys, helm, bwd = c.op("physderiv"), c.op("helmholtz"), c.op("bwdtrans")
    o = phys(c.ext, *c.bs, *c.ds, df, x, **c.kw)                                # (dim, nelmt * npt), rows aligned
    nbytes = c.nbytes("physderiv")
    mean_ms, min_ms = s.timed(lambda: phys(c.ext, *c.bs, *c.ds, df, x, out=o, **c.kw))
    fused = o.clone() if args.check else None
    r_mean, r_min = s.timed(lambda: phys(c.ext, *c.bs, *c.ds, None, x, out=o, **c.kw))
    row = {"t_physderiv": ms(mean_ms), "t_physderiv_min": ms(min_ms), "gdof_s": gdof_s(nelmt * c.nmt, mean_ms),
           **roofline(nbytes, mean_ms, min_ms), "t_refspace": ms(r_mean), "t_refspace_min": ms(r_min),
           **fracs("refspace", c.nbytes("physderiv", df=False), r_mean, r_min)}
    g = df[:nelmt * (dim * (dim + 1) // 2) * c.npt]                             # timing only: any planes will do
    w = c.fill(nelmt * c.npt, 2)
    om = torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    h_mean, h_min = s.timed(lambda: helm(c.ext, *c.bs, *c.ds, g, w, 0.75, x, out=om))
    b_mean, b_min = s.timed(lambda: bwd(c.ext, *c.bs, x, out=o[0]))
    row.update({"t_helmholtz": ms(h_mean), **fracs("helmholtz", c.nbytes("helmholtz"), h_mean, h_min),
                "t_bwd": ms(b_mean), **fracs("bwd", c.nbytes("bwdtrans"), b_mean, b_min)})
    del w, om, g
    if args.chain:
        o2 = torch.empty_like(o)
        chain = make_chain(torch, s.sf, dim, c.nq, nelmt, c.bs, c.ds, df, x, [o2[a] for a in range(dim)])
        row.update(chain_row(mean_ms, *s.timed(chain)))
        if args.check:
            row["chain_rel_diff"] = float((fused - o2).abs().max() / fused.abs().max())
    print(f"physderiv {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, chain="also time bwdtrans + torch ops on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "physderiv": {}}
    s.collect(res["physderiv"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
