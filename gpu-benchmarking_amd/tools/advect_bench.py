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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time physderiv + torch ops + iproduct on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, nf = d, {args.repeats} repeats of {args.reps} "
                       "groups of 8 back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "advect": {}}
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
                df = sf.fill_random(nelmt * dim * dim * npt, 5, dtype=dtype, device=dev)
                w = sf.fill_random(nelmt * npt, 2, dtype=dtype, device=dev)
                c = sf.fill_random(dim * nelmt * npt, 1, dtype=dtype, device=dev).view(dim, nelmt * npt)
                x = sf.fill_random(dim * nelmt * nmt, 6, dtype=dtype, device=dev).view(dim, nelmt * nmt)
                adv = sf.advect_hex if dim == 3 else sf.advect_quad
                o = adv(ext, *bs, *ds, df, w, c, x, **kw)
                nbytes = size * nelmt * ((dim * dim + dim + 1) * npt + 2 * dim * nmt)
                chain = o2 = None
                if args.chain:
                    o2 = torch.empty_like(o)
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, w, c, x, o2)
                rows = []
                for rep in range(args.repeats):
                    mean_ms, min_ms, g0 = grouped_ms(torch, lambda: adv(ext, *bs, *ds, df, w, c, x, out=o, **kw), args.reps)
                    replayed = replayed and g0
                    row = {"repeat": rep, "t_advect": round(mean_ms, 5), "t_advect_min": round(min_ms, 5),
                           "gdof_s": round(dim * nelmt * nmt / mean_ms * 1e-6, 2), "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                           "frac_mean": round(nbytes / mean_ms * 1e-6 / HBM_PEAK_GBS, 4),
                           "frac_min": round(nbytes / min_ms * 1e-6 / HBM_PEAK_GBS, 4)}
                    if chain is not None:
                        c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                        replayed = replayed and g1
                        row.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                    "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                    rows.append(row)
                    print(f"advect {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                if chain is not None and args.check:
                    rel = float((o - o2).abs().max() / o.abs().max())
                    rows.append({"chain_rel_diff": rel})
                    print(f"advect {dim}D {tname} nq {nq:2d}: max |fused - chain| / max |fused| = {rel:.3g}", flush=True)
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["advect"].setdefault(key, {})[str(nq)] = rows
                del df, w, c, x, o, o2, chain
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
