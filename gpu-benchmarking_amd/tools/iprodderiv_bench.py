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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time torch ops + iproduct on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / (2 gamma_N absref) (needs --chain)")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "iprodderiv": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            for nq in orders:
                nm, ext = nq - 1, (nq,) * dim
                nmt, npt = nm ** dim, nq ** dim
                b = sf.fill_random(nm * nq, 3, dtype=dtype, device=dev)
                d = sf.fill_random(nq * nq, 4, dtype=dtype, device=dev)
                bs, ds = (b,) * dim, (d,) * dim
                f = sf.fill_random(dim * nelmt * npt, 1, dtype=dtype, device=dev).view(dim, nelmt * npt)
                df = sf.fill_random(nelmt * dim * dim * npt, 5, dtype=dtype, device=dev)
                w = sf.fill_random(nelmt * npt, 2, dtype=dtype, device=dev)
                x = sf.fill_random(nelmt * nmt, 6, dtype=dtype, device=dev)
                ipd, phys, ipr = ((sf.iprodderiv_hex, sf.physderiv_hex, sf.iproduct_hex) if dim == 3 else
                                  (sf.iprodderiv_quad, sf.physderiv_quad, sf.iproduct_quad))
                o = torch.empty(nelmt * nmt, dtype=dtype, device=dev)

                def frac(nb, ms):
                    return round(nb / ms * 1e-6 / HBM_PEAK_GBS, 4)

                nbytes = size * nelmt * ((dim * dim + dim + 1) * npt + nmt)
                rbytes = size * nelmt * (dim * npt + nmt)
                mean_ms, min_ms, g0 = grouped_ms(torch, lambda: ipd(ext, *bs, *ds, df, w, f, out=o, **kw), args.reps)
                fused = o.clone() if args.check else None
                r_mean, r_min, g1 = grouped_ms(torch, lambda: ipd(ext, *bs, *ds, None, None, f, out=o, **kw), args.reps)
                replayed = replayed and g0 and g1
                row = {"t_iprodderiv": round(mean_ms, 5), "t_iprodderiv_min": round(min_ms, 5),
                       "gdof_s": round(nelmt * nmt / mean_ms * 1e-6, 2), "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                       "frac_mean": frac(nbytes, mean_ms), "frac_min": frac(nbytes, min_ms),
                       "t_bothnull": round(r_mean, 5), "t_bothnull_min": round(r_min, 5),
                       "bothnull_frac_mean": frac(rbytes, r_mean), "bothnull_frac_min": frac(rbytes, r_min)}
                po = phys(ext, *bs, *ds, df, x)
                p_mean, p_min, g2 = grouped_ms(torch, lambda: phys(ext, *bs, *ds, df, x, out=po), args.reps)
                i_mean, i_min, g3 = grouped_ms(torch, lambda: ipr(ext, *bs, f[0], out=o), args.reps)
                replayed = replayed and g2 and g3
                pb = size * nelmt * (nmt + (dim * dim + dim) * npt)
                ib = size * nelmt * (nmt + npt)
                row.update({"t_physderiv": round(p_mean, 5), "physderiv_frac_mean": frac(pb, p_mean),
                            "physderiv_frac_min": frac(pb, p_min), "t_iproduct": round(i_mean, 5),
                            "iproduct_frac_mean": frac(ib, i_mean), "iproduct_frac_min": frac(ib, i_min)})
                del po, x
                if args.chain:
                    o2 = torch.empty_like(o)
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, w, f, o2)
                    c_mean, c_min, g4 = grouped_ms(torch, chain, args.reps)
                    replayed = replayed and g4
                    row.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                    del chain
                    if args.check:
                        torch.cuda.empty_cache()
                        diff = (fused - o2).abs_()
                        for t in (b, d, f, df, w):                              # the operands are not needed again
                            t.abs_()
                        absref = ipd(ext, *bs, *ds, df, w, f, out=o, **kw)
                        n_ops = dim * nq + nq + 2 * dim
                        u = 2.0 ** (-53 if dtype == torch.float64 else -24)
                        gam = n_ops * u / (1 - n_ops * u)
                        excess = float((diff / (2 * gam * absref)).max())
                        row.update({"chain_excess": round(excess, 4), "chain_agrees": excess <= 1.0,
                                    "chain_rel_diff": float(diff.max() / fused.abs().max())})
                        del diff
                    del o2
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["iprodderiv"].setdefault(key, {})[str(nq)] = row
                print(f"iprodderiv {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del f, df, w, o, fused
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
