#!/usr/bin/env python3
"""Time IProductWRTDerivBase (sf_iprodderiv_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of 8
back-to-back launches, graph-replayed, mean and min per launch.  Default batch: 262 144 elements in 3D, 1 048 576 in 2D
(the shapes and counts of physderiv_bench.py).

DOF are counted as nelmt * nm^d; the roofline fraction uses the operator's own algorithmic bytes
sizeof(T) * nelmt * ((d^2 + d + 1) nq^d + nm^d) against 8 TB/s; the case df=None, w=None (d nq^d + nm^d) is timed in the
same session, and so are sf_physderiv_* (nm^d + (d^2 + d) nq^d) and sf_iproduct_* (nq^d + nm^d) for context.
--chain also times, in the same process on preallocated buffers, what a user can write without the fused kernel: d^2
mul / addcmul with the planes of df, d mul with w, d torch.matmul with the D_b^T, d - 1 adds, then iproduct_*.
--check runs both on the same data and prints max |fused - chain| / (2 gamma_N absref), absref the fused operator on the
absolute values of every operand (formed on the device): <= 1 says the two agree within the sum of their bounds.

    python3 gpu-benchmarking_amd/tools/iprodderiv_bench.py [--chain] [--check] [--json FILE] [--hex 4,6,8]
                                                           [--quad 8,12,16] [--f32]
"""
import sys

import opbench
from opbench import chain_row, fracs, gdof_s, ms, roofline


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, w, f, out):
    """The unfused composition on preallocated buffers: returns a callable that leaves the result in `out`."""
    ext = (nq,) * dim
    npt = nq ** dim
    ipr = sf.iproduct_hex if dim == 3 else sf.iproduct_quad
    new = lambda: torch.empty(nelmt * npt, dtype=f.dtype, device=f.device)      # noqa: E731
    g = [new() for _ in range(dim)]
    v, t = new(), new()
    dp = df.view(nelmt, dim * dim, npt)
    wv = w.view(nelmt, npt)
    fa = [f[a].view(nelmt, npt) for a in range(dim)]
    d0 = ds[0].view(nq, nq)                                                       # v[.., i'] = sum_i g[.., i] D0[i][i']
    dT = [None] + [d.view(nq, nq).t().contiguous() for d in ds[1:]]               # D_b^T, row-major

    def chain():
        for b in range(dim):
            gb = g[b].view(nelmt, npt)
            torch.mul(dp[:, b], fa[0], out=gb)                                    # t_b = sum_a df[a d + b] f_a
            for a in range(1, dim):
                gb.addcmul_(dp[:, a * dim + b], fa[a])
            gb.mul_(wv)
        torch.matmul(g[0].view(-1, nq), d0, out=v.view(-1, nq))
        torch.matmul(dT[1], g[1].view(-1, nq, nq), out=t.view(-1, nq, nq))        # [.., j', i] = sum_j D1[j][j'] g[.., j, i]
        v.add_(t)
        if dim == 3:
            torch.matmul(dT[2], g[2].view(nelmt, nq, -1), out=t.view(nelmt, nq, -1))
            v.add_(t)
        ipr(ext, *bs, v, out=out)

    return chain


def case(s, c):
    torch, args, dim, nelmt, nq = s.torch, s.args, c.dim, c.nelmt, c.nq
    bs, ds, kw = c.bs, c.ds, c.kw
    f = c.fill(dim * nelmt * c.npt, 1).view(dim, nelmt * c.npt)
    df = c.fill(nelmt * dim * dim * c.npt, 5)
    w = c.fill(nelmt * c.npt, 2)
    x = c.fill(nelmt * c.nmt, 6)
    ipd, phys, ipr = c.op("iprodderiv"), c.op("physderiv"), c.op("iproduct")
    o = torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    nbytes = c.nbytes("iprodderiv")
    mean_ms, min_ms = s.timed(lambda: ipd(c.ext, *bs, *ds, df, w, f, out=o, **kw))
    fused = o.clone() if args.check else None
    r_mean, r_min = s.timed(lambda: ipd(c.ext, *bs, *ds, None, None, f, out=o, **kw))
    row = {"t_iprodderiv": ms(mean_ms), "t_iprodderiv_min": ms(min_ms), "gdof_s": gdof_s(nelmt * c.nmt, mean_ms),
           **roofline(nbytes, mean_ms, min_ms), "t_bothnull": ms(r_mean), "t_bothnull_min": ms(r_min),
           **fracs("bothnull", c.nbytes("iprodderiv", df=False, w=False), r_mean, r_min)}
    po = phys(c.ext, *bs, *ds, df, x)
    p_mean, p_min = s.timed(lambda: phys(c.ext, *bs, *ds, df, x, out=po))
    i_mean, i_min = s.timed(lambda: ipr(c.ext, *bs, f[0], out=o))
    row.update({"t_physderiv": ms(p_mean), **fracs("physderiv", c.nbytes("physderiv"), p_mean, p_min),
                "t_iproduct": ms(i_mean), **fracs("iproduct", c.nbytes("iproduct"), i_mean, i_min)})
    del po, x
    if args.chain:
        o2 = torch.empty_like(o)
        chain = make_chain(torch, s.sf, dim, nq, nelmt, bs, ds, df, w, f, o2)
        row.update(chain_row(mean_ms, *s.timed(chain)))
        del chain
        if args.check:
            s.free()
            diff = (fused - o2).abs_()
            for t in (bs[0], ds[0], f, df, w):                              # the operands are not needed again
                t.abs_()
            absref = ipd(c.ext, *bs, *ds, df, w, f, out=o, **kw)
            n_ops = dim * nq + nq + 2 * dim
            u = 2.0 ** (-53 if c.dtype == torch.float64 else -24)
            gam = n_ops * u / (1 - n_ops * u)
            excess = float((diff / (2 * gam * absref)).max())
            row.update({"chain_excess": round(excess, 4), "chain_agrees": excess <= 1.0,
                        "chain_rel_diff": float(diff.max() / fused.abs().max())})
    print(f"iprodderiv {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, chain="also time torch ops + iproduct on the same buffers",
                        check="print max |fused - chain| / (2 gamma_N absref) (needs --chain)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "iprodderiv": {}}
    s.collect(res["iprodderiv"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
