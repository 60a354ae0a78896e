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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())

SELECTIONS = {"all": ("grad", "div", "curl"), "div+curl": ("div", "curl")}
CURL_PAIRS = {2: (((1, 0), (0, 1)),), 3: (((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))}


def _orders(s):
    return [int(x) for x in s.split(",") if x]


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time d x physderiv + torch.add / torch.sub on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| per output (needs --chain)")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "vecgrad": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            ncurl = dim * (dim - 1) // 2
            for nq in orders:
                nm, ext = nq - 1, (nq,) * dim
                nmt, npt = nm ** dim, nq ** dim
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                d = sf.fill_random(nq * nq, 4, dtype=dtype, device=dev)
                bs, ds = (b,) * dim, (d,) * dim
                df = sf.fill_random(nelmt * dim * dim * npt, 5, dtype=dtype, device=dev)
                x = sf.fill_random(dim * nelmt * nmt, 6, dtype=dtype, device=dev).view(dim, nelmt * nmt)
                vg = sf.vecgrad_hex if dim == 3 else sf.vecgrad_quad
                full = vg(ext, *bs, *ds, df, x, **kw)
                chain = g = div2 = curl2 = None
                if args.chain:
                    g = [torch.empty((dim, nelmt * npt), dtype=dtype, device=dev) for _ in range(dim)]
                    div2 = torch.empty(nelmt * npt, dtype=dtype, device=dev)
                    curl2 = torch.empty((ncurl, nelmt * npt), dtype=dtype, device=dev)
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, x, g, div2, curl2)
                rows = []
                for rep in range(args.repeats):
                    c_mean = c_min = None
                    if chain is not None:
                        c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                        replayed = replayed and g1
                    for sel, names in SELECTIONS.items():
                        out = {k: full[k] for k in names}
                        n_out = (dim * dim if "grad" in names else 0) + 1 + ncurl
                        nbytes = size * nelmt * (dim * nmt + dim * dim * npt + n_out * npt)
                        mean_ms, min_ms, g0 = grouped_ms(
                            torch, lambda: vg(ext, *bs, *ds, df, x, outputs=names, out=out, **kw), args.reps)
                        replayed = replayed and g0
                        row = {"repeat": rep, "outputs": sel, "t_vecgrad": round(mean_ms, 5), "t_vecgrad_min": round(min_ms, 5),
                               "gb_s": round(nbytes / mean_ms * 1e-6, 1), "frac_mean": round(nbytes / mean_ms * 1e-6 / HBM_PEAK_GBS, 4),
                               "frac_min": round(nbytes / min_ms * 1e-6 / HBM_PEAK_GBS, 4)}
                        if chain is not None:
                            row.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                        "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                        rows.append(row)
                        print(f"vecgrad {dim}D {tname} nq {nq:2d}: {row}", flush=True)
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
                    print(f"vecgrad {dim}D {tname} nq {nq:2d}: max |fused - chain| / max |fused| = {rel}", flush=True)
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["vecgrad"].setdefault(key, {})[str(nq)] = rows
                del df, x, full, g, div2, curl2, chain
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
