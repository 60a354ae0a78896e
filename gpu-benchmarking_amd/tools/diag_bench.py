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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())


def _orders(s):
    return [int(x) for x in s.split(",") if x]


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--laplacian", action="store_true", help="lambda = 0, w = None")
    ap.add_argument("--chain", action="store_true", help="also time the torch formulation on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--helmholtz", action="store_true", help="also time sf_helmholtz_* at the same orders")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    lam = 0.0 if args.laplacian else 0.75
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "lambda": lam, "diag": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            ncomp = dim * (dim + 1) // 2
            for nq in orders:
                nm, ext = nq - 1, (nq,) * dim
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                d = sf.fill_random(nq * nq, 4, dtype=dtype, device=dev)
                bs, ds = (b,) * dim, (d,) * dim
                g = sf.fill_random(nelmt * ncomp * nq ** dim, 5, dtype=dtype, device=dev)
                w = None if args.laplacian else sf.fill_random(nelmt * nq ** dim, 2, dtype=dtype, device=dev)
                o = torch.empty(nelmt * nm ** dim, dtype=dtype, device=dev)
                tabs = (sf.diag_tables(nq, b, d),) * dim
                diag, helm = ((sf.diag_helmholtz_hex, sf.helmholtz_hex) if dim == 3 else
                              (sf.diag_helmholtz_quad, sf.helmholtz_quad))
                planes = ncomp + (0 if args.laplacian else 1)
                nbytes = size * nelmt * (planes * nq ** dim + nm ** dim)

                def frac(nb, ms):
                    return round(nb / ms * 1e-6 / HBM_PEAK_GBS, 4)

                mean_ms, min_ms, graphed = grouped_ms(torch, lambda: diag(ext, *bs, *ds, g, w, lam, out=o, tabs=tabs, **kw),
                                                      args.reps)
                replayed = replayed and graphed
                row = {"ms": round(mean_ms, 5), "ms_min": round(min_ms, 5),
                       "gdof_s": round(nelmt * nm ** dim / mean_ms * 1e-6, 2),
                       "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                       "frac_mean": frac(nbytes, mean_ms), "frac_min": frac(nbytes, min_ms)}
                if args.chain:
                    o2 = torch.empty_like(o)
                    chain = make_chain(torch, dim, nq, nelmt, b, d, g, w, lam, o2)
                    c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                    replayed = replayed and g1
                    row.update({"ms_chain": round(c_mean, 5), "ms_chain_min": round(c_min, 5),
                                "speedup_vs_chain": round(c_mean / mean_ms, 3)})
                    if args.check:
                        diag(ext, *bs, *ds, g, w, lam, out=o, tabs=tabs, **kw)
                        chain()
                        torch.cuda.synchronize()
                        row["chain_rel_diff"] = float((o - o2).abs().max() / o.abs().max())
                    del chain, o2
                if args.helmholtz:
                    x = sf.fill_random(nelmt * nm ** dim, 1, dtype=dtype, device=dev)
                    h_mean, h_min, g2 = grouped_ms(torch, lambda: helm(ext, *bs, *ds, g, w, lam, x, out=o, **kw), args.reps)
                    replayed = replayed and g2
                    hb = nbytes + size * nelmt * nm ** dim
                    row.update({"ms_helmholtz": round(h_mean, 5), "ms_helmholtz_min": round(h_min, 5),
                                "helmholtz_frac_mean": frac(hb, h_mean), "helmholtz_frac_min": frac(hb, h_min),
                                "diag_over_helmholtz": round(mean_ms / h_mean, 3)})
                    del x
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["diag"].setdefault(key, {})[str(nq)] = row
                print(f"diag {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del g, w, o
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
