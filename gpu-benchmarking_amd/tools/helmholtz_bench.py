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
    dT = [d.view(nq, nq).t().contiguous() for d in ds]
    dm = [d.view(nq, nq) for d in ds]

    def views(t):
        """the three matrix views of a point image: rows over i, batches (e,k) of j x i, batches e of k x (j i)"""
        return (t.view(-1, nq), t.view(-1, nq, nq), t.view(nelmt, nq, -1) if dim == 3 else None)

    def chain():
        bwd(ext, *bs, x, out=u)
        ui, uj, uk = views(u)
        torch.matmul(ui, dT[0], out=views(du[0])[0])                       # du_0[.., i] = sum_m D0[i][m] u[.., m]
        torch.matmul(dm[1], uj, out=views(du[1])[1])                       # du_1[.., j, i] = sum_m D1[j][m] u[.., m, i]
        if dim == 3:
            torch.matmul(dm[2], uk, out=views(du[2])[2])
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
        vi, vj, vk = views(v)
        vi.addmm_(views(fl[0])[0], dm[0])                                  # += sum_i f_0[.., i] D0[i][i']
        vj.baddbmm_(dT[1].expand(vj.shape[0], nq, nq), views(fl[1])[1])
        if dim == 3:
            vk.baddbmm_(dT[2].expand(nelmt, nq, nq), views(fl[2])[2])
        ipr(ext, *bs, v, out=o)

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
    ap.add_argument("--chain", action="store_true", help="also time bwdtrans, torch ops, iproduct on the same buffers")
    ap.add_argument("--mass", action="store_true", help="also time sf_mass_* and bwdtrans_* at the same orders")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
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
           "device": sf.device_info()["name"], "lambda": lam, "helmholtz": {}}
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
                x = sf.fill_random(nelmt * nm ** dim, 1, dtype=dtype, device=dev)
                g = sf.fill_random(nelmt * ncomp * nq ** dim, 5, dtype=dtype, device=dev)
                w = None if args.laplacian else sf.fill_random(nelmt * nq ** dim, 2, dtype=dtype, device=dev)
                o = torch.empty(nelmt * nm ** dim, dtype=dtype, device=dev)
                helm, mass, bwd = ((sf.helmholtz_hex, sf.mass_hex, sf.bwdtrans_hex) if dim == 3 else
                                   (sf.helmholtz_quad, sf.mass_quad, sf.bwdtrans_quad))
                planes = ncomp + (0 if args.laplacian else 1)
                nbytes = size * nelmt * (2 * nm ** dim + planes * nq ** dim)

                def frac(nb, ms):
                    return round(nb / ms * 1e-6 / HBM_PEAK_GBS, 4)

                mean_ms, min_ms, graphed = grouped_ms(torch, lambda: helm(ext, *bs, *ds, g, w, lam, x, out=o, **kw),
                                                      args.reps)
                replayed = replayed and graphed
                row = {"ms": round(mean_ms, 5), "ms_min": round(min_ms, 5),
                       "gdof_s": round(nelmt * nm ** dim / mean_ms * 1e-6, 2),
                       "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                       "frac_mean": frac(nbytes, mean_ms), "frac_min": frac(nbytes, min_ms)}
                if args.chain:
                    o2 = torch.empty_like(o)
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, g, w, lam, x, o2)
                    c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                    replayed = replayed and g1
                    row.update({"ms_chain": round(c_mean, 5), "ms_chain_min": round(c_min, 5),
                                "speedup_vs_chain": round(c_mean / mean_ms, 3)})
                    if args.check:
                        row["chain_rel_diff"] = float((o - o2).abs().max() / o.abs().max())
                    del chain, o2
                if args.mass:
                    wm = w if w is not None else sf.fill_random(nelmt * nq ** dim, 2, dtype=dtype, device=dev)
                    pts = torch.empty(nelmt * nq ** dim, dtype=dtype, device=dev)
                    m_mean, m_min, g2 = grouped_ms(torch, lambda: mass(ext, *bs, wm, x, out=o), args.reps)
                    b_mean, b_min, g3 = grouped_ms(torch, lambda: bwd(ext, *bs, x, out=pts), args.reps)
                    replayed = replayed and g2 and g3
                    mb = size * nelmt * (2 * nm ** dim + nq ** dim)
                    bb = size * nelmt * (nm ** dim + nq ** dim)
                    row.update({"ms_mass": round(m_mean, 5), "mass_frac_mean": frac(mb, m_mean),
                                "mass_frac_min": frac(mb, m_min), "ms_bwd": round(b_mean, 5),
                                "bwd_frac_mean": frac(bb, b_mean), "bwd_frac_min": frac(bb, b_min)})
                    del pts, wm
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["helmholtz"].setdefault(key, {})[str(nq)] = row
                print(f"helmholtz {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del x, g, w, o
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
