#!/usr/bin/env python3
"""Time the gradient, divergence and curl of a vector field (sf_vecgrad_*) with the protocol of bench.py's extras():
grouped_ms -- 40 groups of 8 back-to-back launches, graph-replayed, mean and min per launch -- in `--repeats` repeats
(default 2), each a row of its own, for the output selections "all" (grad, div, curl) and "div+curl".  Default batch:
262 144 elements in 3D, 1 048 576 in 2D (the shapes and counts of advect_bench.py).

The roofline fraction uses the call's own algorithmic bytes sizeof(T) * nelmt * (d nm^d + d^2 nq^d + n_out nq^d), n_out
the planes asked for, against 8 TB/s.
--chain also times, in the same process on preallocated buffers, what a user writes without the fused kernel: d calls of
physderiv_* (each re-reads the d^2 planes of df), then torch.add / torch.sub with out= for the divergence and the curl.
The chain forms every plane of grad on the way, so one chain time stands against both selections.
--check prints max |fused - chain| / max |fused| per output on the same data (expected 0: the same bits).

    python3 gpu-benchmarking_amd/tools/vecgrad_bench.py [--chain] [--check] [--json FILE] [--hex 4,6,8] [--quad 8,12,16]
                                                        [--f32] [--repeats 2]
"""
import sys

import opbench
from opbench import chain_row, ms, roofline

SELECTIONS = {"all": ("grad", "div", "curl"), "div+curl": ("div", "curl")}
CURL_PAIRS = {2: (((1, 0), (0, 1)),), 3: (((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))}


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, x, g, div, curl):
    """The unfused composition on preallocated buffers: g[a] takes the d outputs of physderiv_* on in_a, div and the rows
    of curl their sums and differences, in the order of steps 4 and 5 of the operator."""
    ext = (nq,) * dim
    phys = sf.physderiv_hex if dim == 3 else sf.physderiv_quad

    def chain():
        for a in range(dim):
            phys(ext, *bs, *ds, df, x[a], out=g[a])
        torch.add(g[0][0], g[1][1], out=div)
        if dim == 3:
            torch.add(div, g[2][2], out=div)
        for n, ((p, q), (r, s)) in enumerate(CURL_PAIRS[dim]):
            torch.sub(g[p][q], g[r][s], out=curl[n])

    return chain


def case(s, c):
    torch, args, dim, nelmt, npt = s.torch, s.args, c.dim, c.nelmt, c.npt
    ncurl = dim * (dim - 1) // 2
    df = c.fill(nelmt * dim * dim * npt, 5)
    x = c.fill(dim * nelmt * c.nmt, 6).view(dim, nelmt * c.nmt)
    vg = c.op("vecgrad")
    full = vg(c.ext, *c.bs, *c.ds, df, x, **c.kw)
    chain = g = div2 = curl2 = None
    if args.chain:
        g = [torch.empty((dim, nelmt * npt), dtype=c.dtype, device=s.dev) for _ in range(dim)]
        div2 = torch.empty(nelmt * npt, dtype=c.dtype, device=s.dev)
        curl2 = torch.empty((ncurl, nelmt * npt), dtype=c.dtype, device=s.dev)
        chain = make_chain(torch, s.sf, dim, c.nq, nelmt, c.bs, c.ds, df, x, g, div2, curl2)
    rows = []
    for rep in range(args.repeats):
        c_time = s.timed(chain) if chain is not None else None
        for sel, names in SELECTIONS.items():
            out = {k: full[k] for k in names}
            mean_ms, min_ms = s.timed(lambda: vg(c.ext, *c.bs, *c.ds, df, x, outputs=names, out=out, **c.kw))
            row = {"repeat": rep, "outputs": sel, "t_vecgrad": ms(mean_ms), "t_vecgrad_min": ms(min_ms),
                   **roofline(c.nbytes("vecgrad", outputs=names), mean_ms, min_ms)}
            if chain is not None:
                row.update(chain_row(mean_ms, *c_time))
            rows.append(row)
            print(f"vecgrad {c.label}: {row}", flush=True)
    if chain is not None and args.check:
        grad = full["grad"].view(nelmt, dim * dim, npt)
        rel = {"grad": 0.0}
        for a in range(dim):
            for j in range(dim):
                diff = (grad[:, a * dim + j] - g[a][j].view(nelmt, npt)).abs().max()
                rel["grad"] = max(rel["grad"], float(diff / full["grad"].abs().max()))
        rel["div"] = float((full["div"] - div2).abs().max() / full["div"].abs().max())
        rel["curl"] = float((full["curl"].reshape(ncurl, -1) - curl2).abs().max() / full["curl"].abs().max())
        rows.append({"chain_rel_diff": rel})
        print(f"vecgrad {c.label}: max |fused - chain| / max |fused| = {rel}", flush=True)
    return rows


def options(argv=None):
    ap = opbench.parser(__doc__, repeats=(2, None),
                        chain="also time d x physderiv + torch.add / torch.sub on the same buffers",
                        check="print max |fused - chain| / max |fused| per output (needs --chain)")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "vecgrad": {}}
    s.collect(res["vecgrad"], lambda c: case(s, c))
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
