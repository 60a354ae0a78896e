#!/usr/bin/env python3
"""Time the tensor-product apply with independent input / output extents (sf_tensor_*) with the protocol of bench.py's
extras(): grouped_ms -- groups of 8 back-to-back launches, graph-replayed, mean and min per launch -- in --repeats
independent repeats (default two).  Default batch: 262 144 elements in 3D at 8>8, 4>6, 6>9 and 9>6 (trans = 1),
1 048 576 in 2D at 8>8, 16>16 and 10>15.

The roofline fraction uses the call's own algorithmic traffic, sizeof(T) * nelmt * (prod ni + prod no), against 8 TB/s.
--chain also times, in the same process on the same preallocated buffers, what a caller writes without the kernel: one
torch.matmul per direction over permuted views.  The bar is "not slower than the chain" at every shape in every repeat.
--check prints max |fused - chain| / max |fused|.
--bwdtrans adds, in the same session, the run-time specialised tensor kernel at (7>8)^3 and (15>16)^2 beside sf_bwdtrans_*
AUTO at nq 8 / 16 (the flagship's tuned rows), with the compile seconds of each specialisation.

    python3 gpu-benchmarking_amd/tools/tensor_bench.py [--chain] [--check] [--f32] [--bwdtrans] [--json FILE]
                                                       [--hex 8>8,4>6,6>9,9>6:t] [--quad 8>8,16>16,10>15] [--repeats 2]
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())


def _pairs(s):
    """"8>8,9>6:t" -> [(8, 8, 0), (9, 6, 1)]"""
    out = []
    for tok in (t for t in s.split(",") if t):
        trans = tok.endswith(":t")
        a, b = tok[:-2 if trans else None].split(">")
        out.append((int(a), int(b), int(trans)))
    return out


def make_chain(torch, dim, ni, no, trans, nelmt, mats, x, out):
    """One torch.matmul per direction over permuted views, on preallocated buffers; the result lands in `out`."""
    M = [m.view(no, ni).t() if trans else m.view(ni, no) for m in mats]       # ni x no views of the caller's arrays
    if dim == 3:
        w1 = torch.empty((nelmt * ni * ni, no), dtype=x.dtype, device=x.device)
        w2 = torch.empty((nelmt * ni, no, no), dtype=x.dtype, device=x.device)
        xv, ov = x.view(nelmt * ni * ni, ni), out.view(nelmt, no, no * no)

        def chain():
            torch.matmul(xv, M[0], out=w1)                                    # [e r q][i]
            torch.matmul(M[1].t(), w1.view(nelmt * ni, ni, no), out=w2)       # [e r][j][i]
            torch.matmul(M[2].t(), w2.view(nelmt, ni, no * no), out=ov)       # [e][k][j i]
    else:
        w1 = torch.empty((nelmt * ni, no), dtype=x.dtype, device=x.device)
        xv, ov = x.view(nelmt * ni, ni), out.view(nelmt, no, no)

        def chain():
            torch.matmul(xv, M[0], out=w1)                                    # [e q][i]
            torch.matmul(M[1].t(), w1.view(nelmt, ni, no), out=ov)            # [e][j][i]
    return chain


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nelmt3", type=int, default=1 << 18)
    ap.add_argument("--nelmt2", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--hex", type=_pairs, default=_pairs("8>8,4>6,6>9,9>6:t"))
    ap.add_argument("--quad", type=_pairs, default=_pairs("8>8,16>16,10>15"))
    ap.add_argument("--f32", action="store_true", help="fp32 as well")
    ap.add_argument("--chain", action="store_true", help="also time one torch.matmul per direction on the same buffers")
    ap.add_argument("--check", action="store_true", help="print max |fused - chain| / max |fused| (needs --chain)")
    ap.add_argument("--bwdtrans", action="store_true", help="the specialised (7>8)^3 / (15>16)^2 beside sf_bwdtrans_* AUTO")
    ap.add_argument("--variant", default="auto", help="auto, wave or generic")
    ap.add_argument("--json", default=None, help="write the result here as well")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    sf = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": sf.device_info()["name"], "tensor": {}}
    replayed = True
    gen = torch.Generator(device=dev).manual_seed(1)
    dtypes = [("f64", torch.float64)] + ([("f32", torch.float32)] if args.f32 else [])

    def timed(call):
        nonlocal replayed
        mean_ms, min_ms, g = grouped_ms(torch, call, args.reps)
        replayed = replayed and g
        return mean_ms, min_ms

    for tname, dtype in dtypes:
        size = torch.finfo(dtype).bits // 8
        for dim, pairs, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            fn = sf.tensor_hex if dim == 3 else sf.tensor_quad
            for ni, no, trans in pairs:
                mats = [2 * torch.rand(ni * no, dtype=dtype, device=dev, generator=gen) - 1 for _ in range(dim)]
                x = 2 * torch.rand(nelmt * ni ** dim, dtype=dtype, device=dev, generator=gen) - 1
                out = fn((ni,) * dim, (no,) * dim, *mats, x, trans=trans, variant=args.variant)
                nbytes = size * nelmt * (ni ** dim + no ** dim)
                row = {"repeats": []}
                chain = out2 = None
                if args.chain:
                    out2 = torch.empty_like(out)
                    chain = make_chain(torch, dim, ni, no, trans, nelmt, mats, x, out2)
                for _ in range(args.repeats):
                    mean_ms, min_ms = timed(lambda: fn((ni,) * dim, (no,) * dim, *mats, x, trans=trans, out=out,
                                                       variant=args.variant))
                    rep = {"t_tensor": round(mean_ms, 5), "t_tensor_min": round(min_ms, 5),
                           "gb_s": round(nbytes / mean_ms * 1e-6, 1),
                           "frac_mean": round(nbytes / mean_ms * 1e-6 / HBM_PEAK_GBS, 4),
                           "frac_min": round(nbytes / min_ms * 1e-6 / HBM_PEAK_GBS, 4)}
                    if chain is not None:
                        c_mean, c_min = timed(chain)
                        rep.update({"t_chain": round(c_mean, 5), "t_chain_min": round(c_min, 5),
                                    "speedup_vs_chain": round(c_mean / mean_ms, 3), "not_slower_than_chain": mean_ms <= c_mean})
                    row["repeats"].append(rep)
                if chain is not None:
                    row["not_slower_than_chain"] = all(r["not_slower_than_chain"] for r in row["repeats"])
                    if args.check:
                        row["chain_rel_diff"] = float((out - out2).abs().max() / out.abs().max())
                label = f"{ni}>{no}" + (":t" if trans else "")
                res["tensor"].setdefault(f"{'hex' if dim == 3 else 'quad'}_{tname}", {})[label] = row
                print(f"tensor {dim}D {tname} {label}: {row}", flush=True)
                del x, out, out2, chain
                torch.cuda.empty_cache()

        if args.bwdtrans:
            for dim, nq, nelmt in ((3, 8, args.nelmt3), (2, 16, args.nelmt2)):
                ni, no = (nq - 1,) * dim, (nq,) * dim
                rc = sf.specialise_tensor(ni, no, False, dtype)
                m = re.search(r"compile #\d+, ([\d.]+) s", sf.specialise_log())
                row = {"specialise_rc": rc, "compile_s": float(m.group(1)) if m else None, "repeats": []}
                b = 2 * torch.rand((nq - 1) * nq, dtype=dtype, device=dev, generator=gen) - 1
                x = 2 * torch.rand(nelmt * (nq - 1) ** dim, dtype=dtype, device=dev, generator=gen) - 1
                fn = sf.tensor_hex if dim == 3 else sf.tensor_quad
                bwd = sf.bwdtrans_hex if dim == 3 else sf.bwdtrans_quad
                out = fn(ni, no, *(b,) * dim, x)
                out2 = bwd(no, *(b,) * dim, x)
                row["launched_specialisation"] = sf.tensor_specialisation_state(ni, no, False, dtype)[1] > 0
                row["equal_values"] = bool((out == out2).all())
                nbytes = size * nelmt * ((nq - 1) ** dim + nq ** dim)
                for _ in range(args.repeats):
                    t_mean, t_min = timed(lambda: fn(ni, no, *(b,) * dim, x, out=out))
                    b_mean, b_min = timed(lambda: bwd(no, *(b,) * dim, x, out=out2))
                    row["repeats"].append({"t_tensor": round(t_mean, 5), "t_bwdtrans": round(b_mean, 5),
                                           "frac_tensor": round(nbytes / t_mean * 1e-6 / HBM_PEAK_GBS, 4),
                                           "frac_bwdtrans": round(nbytes / b_mean * 1e-6 / HBM_PEAK_GBS, 4),
                                           "bwdtrans_ahead_by": round(t_mean / b_mean, 3)})
                label = f"{'hex' if dim == 3 else 'quad'}_{tname}_{nq - 1}>{nq}"
                res.setdefault("specialised_vs_bwdtrans", {})[label] = row
                print(f"specialised tensor vs bwdtrans {dim}D {tname} {nq - 1}>{nq}: {row}", flush=True)
                del x, out, out2
                torch.cuda.empty_cache()

    res["hip_graph_replay"] = replayed
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
