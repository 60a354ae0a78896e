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


def make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, x, outs):
    """The unfused composition on preallocated buffers: returns a callable that leaves the result in `outs`."""
    ext = (nq,) * dim
    npt = nq ** dim
    bwd = sf.bwdtrans_hex if dim == 3 else sf.bwdtrans_quad
    new = lambda: torch.empty(nelmt * npt, dtype=x.dtype, device=x.device)      # noqa: E731
    u = new()
    du = [new() for _ in range(dim)]
    dp = df.view(nelmt, dim * dim, npt)
    dT0 = ds[0].view(nq, nq).t().contiguous()
    dm = [d.view(nq, nq) for d in ds]

    def chain():
        bwd(ext, *bs, x, out=u)
        torch.matmul(u.view(-1, nq), dT0, out=du[0].view(-1, nq))               # du_0[.., i] = sum_m D0[i][m] u[.., m]
        torch.matmul(dm[1], u.view(-1, nq, nq), out=du[1].view(-1, nq, nq))     # du_1[.., j, i] = sum_m D1[j][m] u[.., m, i]
        if dim == 3:
            torch.matmul(dm[2], u.view(nelmt, nq, -1), out=du[2].view(nelmt, nq, -1))
        for a in range(dim):
            oa = outs[a].view(nelmt, npt)
            torch.mul(dp[:, a * dim], du[0].view(nelmt, npt), out=oa)
            for b in range(1, dim):
                oa.addcmul_(dp[:, a * dim + b], du[b].view(nelmt, npt))

    return chain


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time bwdtrans + torch ops on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.reps} groups of 8 back-to-back launches "
                       "(bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "physderiv": {}}
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
                x = sf.fill_random(nelmt * nmt, 1, dtype=dtype, device=dev)
                df = sf.fill_random(nelmt * dim * dim * npt, 5, dtype=dtype, device=dev)
                phys, helm, bwd = ((sf.physderiv_hex, sf.helmholtz_hex, sf.bwdtrans_hex) if dim == 3 else
                                   (sf.physderiv_quad, sf.helmholtz_quad, sf.bwdtrans_quad))
                o = phys(ext, *bs, *ds, df, x, **kw)                            # (dim, nelmt * npt), rows aligned

                def frac(nb, ms):
                    return round(nb / ms * 1e-6 / HBM_PEAK_GBS, 4)

                nbytes = size * nelmt * (nmt + (dim * dim + dim) * npt)
                rbytes = size * nelmt * (nmt + dim * npt)
                mean_ms, min_ms, g0 = grouped_ms(torch, lambda: phys(ext, *bs, *ds, df, x, out=o, **kw), args.reps)
                fused = o.clone() if args.check else None
                r_mean, r_min, g1 = grouped_ms(torch, lambda: phys(ext, *bs, *ds, None, x, out=o, **kw), args.reps)
                replayed = replayed and g0 and g1
                row = {"t_physderiv": round(mean_ms, 5), "t_physderiv_min": round(min_ms, 5),
                       "gdof_s": round(nelmt * nmt / mean_ms * 1e-6, 2), "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                       "frac_mean": frac(nbytes, mean_ms), "frac_min": frac(nbytes, min_ms),
                       "t_refspace": round(r_mean, 5), "t_refspace_min": round(r_min, 5),
                       "refspace_frac_mean": frac(rbytes, r_mean), "refspace_frac_min": frac(rbytes, r_min)}
                ncomp = dim * (dim + 1) // 2
                g = df[:nelmt * ncomp * npt]                                # timing only: any planes will do
                w = sf.fill_random(nelmt * npt, 2, dtype=dtype, device=dev)
                om = torch.empty(nelmt * nmt, dtype=dtype, device=dev)
                h_mean, h_min, g2 = grouped_ms(torch, lambda: helm(ext, *bs, *ds, g, w, 0.75, x, out=om), args.reps)
                b_mean, b_min, g3 = grouped_ms(torch, lambda: bwd(ext, *bs, x, out=o[0]), args.reps)
                replayed = replayed and g2 and g3
                hb = size * nelmt * (2 * nmt + (1 + ncomp) * npt)
                bb = size * nelmt * (nmt + npt)
                row.update({"t_helmholtz": round(h_mean, 5), "helmholtz_frac_mean": frac(hb, h_mean),
                            "helmholtz_frac_min": frac(hb, h_min), "t_bwd": round(b_mean, 5),
                            "bwd_frac_mean": frac(bb, b_mean), "bwd_frac_min": frac(bb, b_min)})
                del w, om, g
                if args.chain:
                    o2 = torch.empty_like(o)
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, df, x, [o2[a] for a in range(dim)])
                    c_mean, c_min, g4 = grouped_ms(torch, chain, args.reps)
                    replayed = replayed and g4
                    row.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                    if args.check:
                        row["chain_rel_diff"] = float((fused - o2).abs().max() / fused.abs().max())
                    del chain, o2
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["physderiv"].setdefault(key, {})[str(nq)] = row
                print(f"physderiv {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del x, df, o, fused
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
