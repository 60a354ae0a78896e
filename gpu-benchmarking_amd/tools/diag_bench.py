#!/usr/bin/env python3
"""Time the diagonal of the fused Helmholtz operator (sf_diag_helmholtz_*) with the protocol of bench.py's extras():
grouped_ms -- 40 groups of 8 back-to-back launches, graph-replayed, mean and min per launch.  Default batch: 262 144
elements in 3D, 1 048 576 in 2D, as tools/helmholtz_bench.py.  The tables (sf_diag_tables_*) are built once, outside the
timed region: they depend on the order only.

The roofline fraction uses the call's own algorithmic bytes, sizeof(T) * nelmt * ((1 + d(d+1)/2) nq^d + nm^d), against
8 TB/s (--laplacian: lambda = 0, w = None, one plane less).
--chain also times, in the same process on the same buffers, what a user can write without the kernel: the tables by
matmul (once), then per term one matmul chain k -> r, j -> q, i -> p into preallocated buffers (seven terms in 3D, four in
2D), accumulated with addmm_.  --check prints max |fused - chain| / max |fused|.
--helmholtz times one sf_helmholtz_* application at the same order in the same process (its own algorithmic bytes: nm^d
more).

    python3 gpu-benchmarking_amd/tools/diag_bench.py [--chain] [--check] [--helmholtz] [--laplacian] [--json FILE]
                                                     [--hex 4,6,8] [--quad 8,12,16] [--f32]
"""
import sys

import opbench
from opbench import chain_row, fracs, gdof_s, ms, roofline


def make_chain(torch, dim, nq, nelmt, b, d, g, w, lam, o):
    """The torch formulation on preallocated buffers: returns a callable that leaves the diagonal in `o`."""
    nm, npt = nq - 1, nq ** dim
    B, D = b.view(nm, nq), d.view(nq, nq)
    E = B @ D.t()                                                      # E[p][i] = sum_m D[i][m] B[p][m]
    T = [B * B, E * B, E * E]
    Tt = [t.t().contiguous() for t in T]
    gp = g.view(nelmt, dim * (dim + 1) // 2, npt)
    terms = []                                                         # (plane, tables per direction, factor)
    if w is not None:
        terms.append((w.view(nelmt, npt), (0,) * dim, lam))
    c = 0
    for a in range(dim):
        for bb in range(a, dim):
            terms.append((gp[:, c], tuple(int(x == a) + int(x == bb) for x in range(dim)), 1.0 if a == bb else 2.0))
            c += 1
    t1 = torch.empty(nelmt * nm * nq * nq, dtype=o.dtype, device=o.device) if dim == 3 else None
    t2 = torch.empty(nelmt * nm ** (dim - 1) * nq, dtype=o.dtype, device=o.device)
    om = o.view(-1, nm)

    def chain():
        o.zero_()
        for plane, s, f in terms:
            if dim == 3:
                a1 = t1.view(nelmt, nm, nq * nq)
                torch.matmul(T[s[2]], plane.view(nelmt, nq, nq * nq), out=a1)          # k -> r
                a2 = t2.view(nelmt * nm, nm, nq)
                torch.matmul(T[s[1]], a1.view(nelmt * nm, nq, nq), out=a2)             # j -> q
            else:
                a2 = t2.view(nelmt, nm, nq)
                torch.matmul(T[s[1]], plane.view(nelmt, nq, nq), out=a2)               # j -> q
            om.addmm_(a2.view(-1, nq), Tt[s[0]], alpha=f)                              # i -> p, summed over the terms

    return chain


def case(s, c, lam):
    torch, args, dim, nelmt = s.torch, s.args, c.dim, c.nelmt
    b, d = c.bs[0], c.ds[0]
    g = c.fill(nelmt * (dim * (dim + 1) // 2) * c.npt, 5)
    w = None if args.laplacian else c.fill(nelmt * c.npt, 2)
    o = torch.empty(nelmt * c.nmt, dtype=c.dtype, device=s.dev)
    tabs = (s.sf.diag_tables(c.nq, b, d),) * dim
    diag, helm = c.op("diag_helmholtz"), c.op("helmholtz")
    nbytes = c.nbytes("diag_helmholtz", w=not args.laplacian)
    mean_ms, min_ms = s.timed(lambda: diag(c.ext, *c.bs, *c.ds, g, w, lam, out=o, tabs=tabs, **c.kw))
    row = {"ms": ms(mean_ms), "ms_min": ms(min_ms), "gdof_s": gdof_s(nelmt * c.nmt, mean_ms),
           **roofline(nbytes, mean_ms, min_ms)}
    if args.chain:
        o2 = torch.empty_like(o)
        chain = make_chain(torch, dim, c.nq, nelmt, b, d, g, w, lam, o2)
        row.update(chain_row(mean_ms, *s.timed(chain), prefix="ms", bar=False))
        if args.check:
            diag(c.ext, *c.bs, *c.ds, g, w, lam, out=o, tabs=tabs, **c.kw)
            chain()
            torch.cuda.synchronize()
            row["chain_rel_diff"] = float((o - o2).abs().max() / o.abs().max())
        del chain, o2
    if args.helmholtz:
        x = c.fill(nelmt * c.nmt, 1)
        h_mean, h_min = s.timed(lambda: helm(c.ext, *c.bs, *c.ds, g, w, lam, x, out=o, **c.kw))
        row.update({"ms_helmholtz": ms(h_mean), "ms_helmholtz_min": ms(h_min),
                    **fracs("helmholtz", c.nbytes("helmholtz", w=not args.laplacian), h_mean, h_min),
                    "diag_over_helmholtz": round(mean_ms / h_mean, 3)})
    print(f"diag {c.label}: {row}", flush=True)
    return row


def options(argv=None):
    ap = opbench.parser(__doc__, chain="also time the torch formulation on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--laplacian", action="store_true", help="lambda = 0, w = None")
    ap.add_argument("--helmholtz", action="store_true", help="also time sf_helmholtz_* at the same orders")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    lam = 0.0 if args.laplacian else 0.75
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "lambda": lam, "diag": {}}
    s.collect(res["diag"], lambda c: case(s, c, lam))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
