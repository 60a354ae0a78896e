#!/usr/bin/env python3
"""Time the fused Helmholtz operator (sf_helmholtz_*) with the protocol of bench.py's extras(): grouped_ms -- 40 groups of
8 back-to-back launches, graph-replayed, mean and min per launch.  Default batch: 262 144 elements in 3D, 1 048 576 in 2D
(the six metric planes of a 3D nq 8 batch are then 6.4 GB).

DOF are counted as nelmt * nm^d; the roofline fraction uses the fused algorithmic bytes
sizeof(T) * nelmt * (2 nm^d + (1 + d(d+1)/2) nq^d) against 8 TB/s (--laplacian: lambda = 0, w = None, one plane less).
--chain also times, in the same process on the same buffers, what a user can write without the fused kernel: bwdtrans_*,
then torch ops on the point image (matmul for D_a, mul / addcmul for the metric and lambda w, addmm / baddbmm for D_a^T, all
into preallocated buffers), then iproduct_*.  --mass times sf_mass_* and bwdtrans_* at the same orders for context (their
own algorithmic bytes: 2 nm^d + nq^d and nm^d + nq^d).

    python3 gpu-benchmarking_amd/tools/helmholtz_bench.py [--chain] [--mass] [--laplacian] [--json FILE]
                                                          [--hex 4,6,8] [--quad 8,12,16] [--f32]
"""
import sys

import opbench
from opbench import chain_row, fracs, gdof_s, ms, roofline


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, g, w, lam, x, o):
    """The unfused composition on preallocated buffers: returns a callable that leaves the result in `o`."""
    ext = (nq,) * dim
    npt = nq ** dim
    bwd, ipr = (sf.bwdtrans_hex, sf.iproduct_hex) if dim == 3 else (sf.bwdtrans_quad, sf.iproduct_quad)
    new = lambda: torch.empty(nelmt * npt, dtype=x.dtype, device=x.device)      # noqa: E731
    u, v = new(), new()
    du, fl = [new() for _ in range(dim)], [new() for _ in range(dim)]
    gp = g.view(nelmt, dim * (dim + 1) // 2, npt)
    comp = {}
    c = 0
    for a in range(dim):
        for b in range(a, dim):
            comp[(a, b)] = comp[(b, a)] = gp[:, c]
            c += 1
    deriv = opbench.ref_derivs(torch, dim, nq, nelmt, ds)
    dT = [d.view(nq, nq).t().contiguous() for d in ds]
    d0 = ds[0].view(nq, nq)

    def chain():
        bwd(ext, *bs, x, out=u)
        deriv(u, du)
        for a in range(dim):
            fa = fl[a].view(nelmt, npt)
            torch.mul(comp[(a, 0)], du[0].view(nelmt, npt), out=fa)
            for b in range(1, dim):
                fa.addcmul_(comp[(a, b)], du[b].view(nelmt, npt))
        if w is not None:
            torch.mul(w, u, out=v)
            v.mul_(lam)
        else:
            v.zero_()
        v.view(-1, nq).addmm_(fl[0].view(-1, nq), d0)                      # += sum_i f_0[.., i] D0[i][i']
        vj = v.view(-1, nq, nq)
        vj.baddbmm_(dT[1].expand(vj.shape[0], nq, nq), fl[1].view(-1, nq, nq))
        if dim == 3:
            v.view(nelmt, nq, -1).baddbmm_(dT[2].expand(nelmt, nq, nq), fl[2].view(nelmt, nq, -1))
        ipr(ext, *bs, v, out=o)

    return chain


def case(s, c, lam):
    torch, args = s.torch, s.args
    ncomp = c.dim * (c.dim + 1) // 2
    x = c.fill(c.nelmt * c.nmt, 1)
    g = c.fill(c.nelmt * ncomp * c.npt, 5)
    w = None if args.laplacian else c.fill(c.nelmt * c.npt, 2)
    o = torch.empty(c.nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    helm, mass, bwd = c.op("helmholtz"), c.op("mass"), c.op("bwdtrans")
    nbytes = c.nbytes("helmholtz", w=not args.laplacian)
    mean_ms, min_ms = s.timed(lambda: helm(c.ext, *c.bs, *c.ds, g, w, lam, x, out=o, **c.kw))
    row = {"ms": ms(mean_ms), "ms_min": ms(min_ms), "gdof_s": gdof_s(c.nelmt * c.nmt, mean_ms),
           **roofline(nbytes, mean_ms, min_ms)}
    if args.chain:
        o2 = torch.empty_like(o)
        chain = make_chain(torch, s.sf, c.dim, c.nq, c.nelmt, c.bs, c.ds, g, w, lam, x, o2)
        row.update(chain_row(mean_ms, *s.timed(chain), prefix="ms", bar=False))
        if args.check:
            row["chain_rel_diff"] = float((o - o2).abs().max() / o.abs().max())
        del chain, o2
    if args.mass:
        wm = w if w is not None else c.fill(c.nelmt * c.npt, 2)
        pts = torch.empty(c.nelmt * c.npt, dtype=c.dtype, device=s.dev)
        m_mean, m_min = s.timed(lambda: mass(c.ext, *c.bs, wm, x, out=o))
        b_mean, b_min = s.timed(lambda: bwd(c.ext, *c.bs, x, out=pts))
        row.update({"ms_mass": ms(m_mean), **fracs("mass", c.nbytes("mass"), m_mean, m_min),
                    "ms_bwd": ms(b_mean), **fracs("bwd", c.nbytes("bwdtrans"), b_mean, b_min)})
    print(f"helmholtz {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, chain="also time bwdtrans, torch ops, iproduct on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--laplacian", action="store_true", help="lambda = 0, w = None")
    ap.add_argument("--mass", action="store_true", help="also time sf_mass_* and bwdtrans_* at the same orders")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    lam = 0.0 if args.laplacian else 0.75
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "lambda": lam, "helmholtz": {}}
    s.collect(res["helmholtz"], lambda c: case(s, c, lam))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
