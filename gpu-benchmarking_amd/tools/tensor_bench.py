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
import re
import sys

import opbench
from opbench import chain_row, frac, ms, roofline, scalars


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


def options(argv=None):
    ap = opbench.parser(__doc__, hex=(_pairs, _pairs("8>8,4>6,6>9,9>6:t")), quad=(_pairs, _pairs("8>8,16>16,10>15")),
                        repeats=(2, None), chain="also time one torch.matmul per direction on the same buffers",
                        check="print max |fused - chain| / max |fused| (needs --chain)", variant="auto, wave or generic")
    ap.add_argument("--bwdtrans", action="store_true", help="the specialised (7>8)^3 / (15>16)^2 beside sf_bwdtrans_* AUTO")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)
    s = opbench.Session(args)
    torch, sf, dev, timed = s.torch, s.sf, s.dev, s.timed
    res = {"protocol": f"{args.nelmt3} (3D) / {args.nelmt2} (2D) elements, {args.repeats} repeats of {args.reps} groups of 8 "
                       "back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / time / 8 TB/s",
           "device": s.device_name, "tensor": {}}
    gen = torch.Generator(device=dev).manual_seed(1)

    def rand(n, dtype):
        return 2 * torch.rand(n, dtype=dtype, device=dev, generator=gen) - 1

    for tname, dtype, size in s.dtypes():
        for dim, pairs, nelmt in ((3, args.hex, args.nelmt3), (2, args.quad, args.nelmt2)):
            shape = "hex" if dim == 3 else "quad"
            fn = getattr(sf, f"tensor_{shape}")
            for ni, no, trans in pairs:
                mats = [rand(ni * no, dtype) for _ in range(dim)]
                x = rand(nelmt * ni ** dim, dtype)
                out = fn((ni,) * dim, (no,) * dim, *mats, x, trans=trans, variant=args.variant)
                nbytes = size * nelmt * scalars("tensor", dim, ni=ni, no=no)
                row = {"repeats": []}
                chain = out2 = None
                if args.chain:
                    out2 = torch.empty_like(out)
                    chain = make_chain(torch, dim, ni, no, trans, nelmt, mats, x, out2)
                for _ in range(args.repeats):
                    mean_ms, min_ms = timed(lambda: fn((ni,) * dim, (no,) * dim, *mats, x, trans=trans, out=out,
                                                       variant=args.variant))
                    rep = {"t_tensor": ms(mean_ms), "t_tensor_min": ms(min_ms), **roofline(nbytes, mean_ms, min_ms)}
                    if chain is not None:
                        rep.update(chain_row(mean_ms, *timed(chain)))
                    row["repeats"].append(rep)
                if chain is not None:
                    row["not_slower_than_chain"] = all(r["not_slower_than_chain"] for r in row["repeats"])
                    if args.check:
                        row["chain_rel_diff"] = float((out - out2).abs().max() / out.abs().max())
                label = f"{ni}>{no}" + (":t" if trans else "")
                res["tensor"].setdefault(f"{shape}_{tname}", {})[label] = row
                print(f"tensor {dim}D {tname} {label}: {row}", flush=True)
                del x, out, out2, chain
                s.free()

        if args.bwdtrans:
            for dim, nq, nelmt in ((3, 8, args.nelmt3), (2, 16, args.nelmt2)):
                shape = "hex" if dim == 3 else "quad"
                ni, no = (nq - 1,) * dim, (nq,) * dim
                rc = sf.specialise_tensor(ni, no, False, dtype)
                m = re.search(r"compile #\d+, ([\d.]+) s", sf.specialise_log())
                row = {"specialise_rc": rc, "compile_s": float(m.group(1)) if m else None, "repeats": []}
                b = rand((nq - 1) * nq, dtype)
                x = rand(nelmt * (nq - 1) ** dim, dtype)
                fn, bwd = getattr(sf, f"tensor_{shape}"), getattr(sf, f"bwdtrans_{shape}")
                out = fn(ni, no, *(b,) * dim, x)
                out2 = bwd(no, *(b,) * dim, x)
                row["launched_specialisation"] = sf.tensor_specialisation_state(ni, no, False, dtype)[1] > 0
                row["equal_values"] = bool((out == out2).all())
                nbytes = size * nelmt * scalars("bwdtrans", dim, nq)
                for _ in range(args.repeats):
                    t_mean, t_min = timed(lambda: fn(ni, no, *(b,) * dim, x, out=out))
                    b_mean, b_min = timed(lambda: bwd(no, *(b,) * dim, x, out=out2))
                    row["repeats"].append({"t_tensor": ms(t_mean), "t_bwdtrans": ms(b_mean),
                                           "frac_tensor": frac(nbytes, t_mean), "frac_bwdtrans": frac(nbytes, b_mean),
                                           "bwdtrans_ahead_by": round(t_mean / b_mean, 3)})
                res.setdefault("specialised_vs_bwdtrans", {})[f"{shape}_{tname}_{nq - 1}>{nq}"] = row
                print(f"specialised tensor vs bwdtrans {dim}D {tname} {nq - 1}>{nq}: {row}", flush=True)
                del x, out, out2
                s.free()

    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
