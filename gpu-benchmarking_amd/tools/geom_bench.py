#!/usr/bin/env python3
"""Time the geometric factors from element coordinates (sf_geom_*: df, w, g, detj in one kernel) with the protocol of
bench.py's extras(): grouped_ms -- groups of 8 back-to-back launches, graph-replayed, mean and min per launch -- in
--repeats independent repeats (default two).  Default batch: 262 144 elements in 3D at nq 4 / 6 / 8, 1 048 576 in 2D at
nq 8 / 12 / 16.

The roofline fraction uses the call's own algorithmic traffic, sizeof(T) * nelmt * (d nm^d + (d^2 + d(d+1)/2 + 2) nq^d),
against 8 TB/s.
--chain also times, in the same process on the same buffers, what a user writes without the kernel: d calls of
sf_physderiv_* with df = NULL on the coordinate fields (the d x d entries of J), then torch pointwise operations for the
cofactors, the determinant, the inverse, the weight and the metric.  The bar is "not slower than the chain" in every
repeat.  --check prints max |fused - chain| / max |fused| per output.

    python3 gpu-benchmarking_amd/tools/geom_bench.py [--chain] [--check] [--f32] [--json FILE] [--hex 4,6,8]
                                                     [--quad 8,12,16] [--repeats 2]
"""
import sys

import numpy as np
from numpy.polynomial import legendre as _leg

import opbench
from opbench import chain_row, ms, roofline


def gll(nq):
    """(basis nm x nq of Legendre modes, differentiation matrix nq x nq, weights) at the nq Gauss-Lobatto points."""
    n = nq - 1
    Pn = _leg.Legendre.basis(n)
    xi = np.concatenate(([-1.0], np.sort(np.real(Pn.deriv().roots())), [1.0])) if n > 1 else np.array([-1.0, 1.0])
    pn = Pn(xi)
    wts = 2.0 / (n * (n + 1) * pn * pn)
    D = np.zeros((nq, nq))
    for i in range(nq):
        for m in range(nq):
            if i != m:
                D[i, m] = pn[i] / (pn[m] * (xi[i] - xi[m]))
    D[0, 0], D[n, n] = -n * (n + 1) / 4.0, n * (n + 1) / 4.0
    basis = np.stack([_leg.Legendre.basis(p)(xi) for p in range(nq - 1)])
    return basis.reshape(-1), D.reshape(-1), wts


def coordinates(torch, dim, nq, nelmt, dtype, dev):
    """(dim, nelmt * nm^dim) modal coordinates of deformed elements: A_e = I + 0.3 U(-1, 1) on the linear modes plus
    0.1 U(-1, 1) (1 + sum_d m_d)^-3 on every mode -- det J stays within 12 % of det A_e, which stays in [0.48, 1.76], so
    --check compares well-conditioned inverses."""
    nm = nq - 1
    gen = torch.Generator(device=dev).manual_seed(1)
    x = 0.1 * (2 * torch.rand((dim, nelmt) + (nm,) * dim, dtype=dtype, device=dev, generator=gen) - 1)
    m = torch.arange(nm, dtype=dtype, device=dev)
    order = sum(m.view((-1,) + (1,) * b) for b in range(dim))      # sum_d m_d of every mode, shape (nm,) * dim
    x *= (1 + order) ** -3
    A = torch.eye(dim, dtype=dtype, device=dev)[:, None, :] + 0.3 * (2 * torch.rand((dim, nelmt, dim), dtype=dtype, device=dev,
                                                                                    generator=gen) - 1)
    for b in range(dim):
        at = [0] * dim
        at[dim - 1 - b] = 1
        x[(slice(None), slice(None)) + tuple(at)] += A[:, :, b]
    return x.reshape(dim, -1)


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, qs, x, out):
    """The unfused composition on preallocated buffers: returns a callable that leaves the result in `out`."""
    ext, npt = (nq,) * dim, nq ** dim
    phys = sf.physderiv_hex if dim == 3 else sf.physderiv_quad
    J = [torch.empty((dim, nelmt * npt), dtype=x.dtype, device=x.device) for _ in range(dim)]      # J[a][b]
    cof = torch.empty((dim * dim, nelmt, npt), dtype=x.dtype, device=x.device)
    tmp, r = (torch.empty((nelmt, npt), dtype=x.dtype, device=x.device) for _ in range(2))
    q = qs[0]
    for b in range(1, dim):
        q = torch.outer(qs[b], q).reshape(-1)
    q = q.reshape(1, npt).contiguous()
    df, w, g, det = (out["df"].view(nelmt, dim * dim, npt), out["w"].view(nelmt, npt),
                     out["g"].view(nelmt, dim * (dim + 1) // 2, npt), out["detj"].view(nelmt, npt))
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]

    def chain():
        for a in range(dim):
            phys(ext, *bs, *ds, None, x[a], out=J[a])
        Jv = [[J[a][b].view(nelmt, npt) for b in range(dim)] for a in range(dim)]
        if dim == 3:
            for a in range(3):
                for b in range(3):
                    a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
                    torch.mul(Jv[a1][b2], Jv[a2][b1], out=tmp)
                    torch.mul(Jv[a1][b1], Jv[a2][b2], out=cof[a * 3 + b])
                    cof[a * 3 + b].sub_(tmp)
        else:
            cof[0].copy_(Jv[1][1])
            torch.neg(Jv[1][0], out=cof[1])
            torch.neg(Jv[0][1], out=cof[2])
            cof[3].copy_(Jv[0][0])
        torch.mul(Jv[0][0], cof[0], out=det)
        for b in range(1, dim):
            det.addcmul_(Jv[0][b], cof[b])
        torch.reciprocal(det, out=r)
        for c in range(dim * dim):
            torch.mul(cof[c], r, out=df[:, c])
        torch.abs(det, out=w)
        w.mul_(q)
        for c, (a, b) in enumerate(pairs):
            torch.mul(df[:, a], df[:, b], out=tmp)
            for k in range(1, dim):
                tmp.addcmul_(df[:, k * dim + a], df[:, k * dim + b])
            torch.mul(w, tmp, out=g[:, c])

    return chain


def case(s, c):
    torch, args, dim, nelmt = s.torch, s.args, c.dim, c.nelmt
    b, d, q = (torch.tensor(v, dtype=c.dtype, device=s.dev) for v in gll(c.nq))
    bs, ds, qs = (b,) * dim, (d,) * dim, (q,) * dim
    x = coordinates(torch, dim, c.nq, nelmt, c.dtype, s.dev)
    fn = c.op("geom")
    out = fn(c.ext, *bs, *ds, *qs, x, **c.kw)
    nbytes = c.nbytes("geom")
    row = {"repeats": []}
    chain = out2 = None
    if args.chain:
        out2 = {k: torch.empty_like(t) for k, t in out.items()}
        chain = make_chain(torch, s.sf, dim, c.nq, nelmt, bs, ds, qs, x, out2)
    for _ in range(args.repeats):
        mean_ms, min_ms = s.timed(lambda: fn(c.ext, *bs, *ds, *qs, x, out=out, **c.kw))
        rep = {"t_geom": ms(mean_ms), "t_geom_min": ms(min_ms), **roofline(nbytes, mean_ms, min_ms)}
        if chain is not None:
            rep.update(chain_row(mean_ms, *s.timed(chain)))
        row["repeats"].append(rep)
    if chain is not None:
        row["not_slower_than_chain"] = all(r["not_slower_than_chain"] for r in row["repeats"])
        if args.check:
            row["chain_rel_diff"] = {k: float((out[k] - out2[k]).abs().max() / out[k].abs().max()) for k in out}
    print(f"geom {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, repeats=(2, None),
                        chain="also time d x physderiv + torch pointwise ops on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "geom": {}}
    s.collect(res["geom"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
