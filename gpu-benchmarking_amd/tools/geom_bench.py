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
import argparse
import json
import os
import sys

import numpy as np
from numpy.polynomial import legendre as _leg

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())


def _orders(s):
    return [int(x) for x in s.split(",") if x]


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--hex", type=_orders, default=[4, 6, 8])
    ap.add_argument("--quad", type=_orders, default=[8, 12, 16])
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time d x physderiv + torch pointwise ops on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--variant", default="auto", help="fp64 route: auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "geom": {}}
    replayed = True
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])
    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        kw = {"variant": args.variant} if dtype == torch.float64 else {}
        for dim, orders, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            for nq in orders:
                nm, ext = nq - 1, (nq,) * dim
                nmt, npt, ncomp = nm ** dim, nq ** dim, dim * (dim + 1) // 2
                b, d, q = (torch.tensor(v, dtype=dtype, device=dev) for v in gll(nq))
                bs, ds, qs = (b,) * dim, (d,) * dim, (q,) * dim
                x = coordinates(torch, dim, nq, nelmt, dtype, dev)
                fn = sf.geom_hex if dim == 3 else sf.geom_quad
                out = fn(ext, *bs, *ds, *qs, x, **kw)
                nbytes = size * nelmt * (dim * nmt + (dim * dim + ncomp + 2) * npt)
                row = {"repeats": []}
                chain = out2 = None
                if args.chain:
                    out2 = {k: torch.empty_like(t) for k, t in out.items()}
                    chain = make_chain(torch, sf, dim, nq, nelmt, bs, ds, qs, x, out2)
                for _ in range(args.repeats):
                    mean_ms, min_ms, g0 = grouped_ms(torch, lambda: fn(ext, *bs, *ds, *qs, x, out=out, **kw), args.reps)
                    replayed = replayed and g0
                    rep = {"t_geom": round(mean_ms, 5), "t_geom_min": round(min_ms, 5),
                           "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                           "frac_mean": round(nbytes / mean_ms * 1e-6 / HBM_PEAK_GBS, 4),
                           "frac_min": round(nbytes / min_ms * 1e-6 / HBM_PEAK_GBS, 4)}
                    if chain is not None:
                        c_mean, c_min, g1 = grouped_ms(torch, chain, args.reps)
                        replayed = replayed and g1
                        rep.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                    "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                    row["repeats"].append(rep)
                if chain is not None:
                    row["not_slower_than_chain"] = all(r["not_slower_than_chain"] for r in row["repeats"])
                    if args.check:
                        row["chain_rel_diff"] = {k: float((out[k] - out2[k]).abs().max() / out[k].abs().max()) for k in out}
                key = f"{'hex' if dim == 3 else 'quad'}_{tname}"
                res["geom"].setdefault(key, {})[str(nq)] = row
                print(f"geom {dim}D {tname} nq {nq:2d}: {row}", flush=True)
                del x, out, out2, chain
                torch.cuda.empty_cache()
    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
