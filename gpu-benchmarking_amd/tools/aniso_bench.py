#!/usr/bin/env python3
"""Anisotropic extents (3D nq0 != nq1 != nq2, 2D nq0 != nq1; fp64 and fp32): SF_VARIANT_AUTO before and after
sf_specialise() of the shape, the specialised kernel alone, and for 3D fp64 the run-time-extent wave kernel
(bwdtrans_rt.h) and the barrier-per-sweep generic kernel; mean / min over reps of HIP-event-timed launches, fraction of
the 8 TB/s HBM roofline (algorithmic bytes sizeof(T) (nm_tot + nq_tot) per element), and the seconds sf_specialise took
(compile + load).  1 048 576 elements, 131 072 above 1 024 points per element.
Usage: aniso_bench.py [nelmt] [reps]"""
import os
import re
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import __graft_entry__ as ge  # noqa: E402

F64, F32 = torch.float64, torch.float32
SHAPES = [((8, 8, 4), F64), ((4, 8, 6), F64), ((10, 6, 8), F64), ((6, 6, 12), F64), ((12, 10, 8), F64),
          ((3, 5, 4), F64), ((5, 9, 7), F64), ((16, 12, 14), F64), ((16, 16, 14), F64),
          ((4, 9), F64), ((16, 3), F64), ((12, 20), F64), ((23, 5), F64),
          ((3, 5, 4), F32), ((6, 6, 12), F32), ((4, 9), F32), ((12, 20), F32)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sum(ts) / len(ts), min(ts)


def main():
    nelmt = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    sf = ge.load_package()
    for nq, dtype in SHAPES:
        nm = [q - 1 for q in nq]
        nmt, nqt = 1, 1
        for q in nq:
            nmt, nqt = nmt * (q - 1), nqt * q
        n = nelmt if nqt <= 1024 else nelmt // 8
        bs = [sf.fill_basis(nm[d], nq[d], dtype=dtype) for d in range(len(nq))]
        x = sf.fill_random(n * nmt, 1, dtype=dtype)
        out = torch.empty(n * nqt, dtype=dtype, device="cuda")
        byt = n * (8 if dtype == F64 else 4) * (nmt + nqt)
        hexq = len(nq) == 3

        def auto(variant="auto"):
            if hexq:
                sf.bwdtrans_hex(nq, *bs, x, out=out, variant=variant)
            else:
                sf.bwdtrans_quad(nq, *bs, x, out=out, variant=variant)

        res = {"auto-before": timed(auto, reps)}
        s0 = time.perf_counter()
        rc = sf.specialise(nq, dtype)
        spec_s = time.perf_counter() - s0
        m = re.search(r"compile #\d+, ([\d.]+) s", sf.specialise_log())
        compile_s = float(m.group(1)) if m else -1.0
        cols = [("auto", auto)]
        if rc == sf.capi.SF_OK:
            cols.append(("specialised", lambda: sf.bwdtrans_specialised(nq, *bs, inp=x, out=out)))
        if hexq and dtype == F64:
            cols += [("wave-rt", lambda: auto("wave-rt")), ("generic", lambda: auto("generic"))]
        for name, fn in cols:
            if name == "wave-rt" and max(nq) > 16:
                continue
            res[name] = timed(fn, reps)
        shape = "x".join(f"{q}" for q in nq)
        row = (f"{'fp64' if dtype == F64 else 'fp32'} {len(nq)}D {shape:>9s} nelmt {n:>8d} specialise "
               f"{'ready' if rc == 0 else 'refused'} compile {compile_s:5.2f} s (call {spec_s:5.2f} s)")
        for name, (tmean, tmin) in res.items():
            row += (f" | {name:11s} {n * nmt / tmean * 1e-6:7.2f} GDOF/s {byt / tmean * 1e-6:7.1f} GB/s "
                    f"frac {byt / tmean * 1e-6 / 8000:.3f} (min-time {byt / tmin * 1e-6 / 8000:.3f})")
        print(row, flush=True)
        del x, out


if __name__ == "__main__":
    main()
