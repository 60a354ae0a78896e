#!/usr/bin/env python3
"""Time the gather-scatter calls (sf_global_to_local_*, sf_assemble_*, sf_gs_*) with the protocol of bench.py's extras():
grouped_ms -- groups of 8 back-to-back launches, graph-replayed, mean and min per launch -- against torch's formulation
on the same buffers: assemble against zero_() + index_add_ (float atomics), global_to_local against index_select, gs
against index_add_ + index_select; torch's int64 index is converted outside the timed region.

Meshes: a structured hex mesh of 64^3 elements and a quad mesh of 1024^2 elements at nq 8 (nm 7), local numbering
element-major, global numbering lexicographic (tests/gs_ref.py structured_map).  The roofline fraction uses each call's own
algorithmic bytes against 8 TB/s:
    global_to_local  nlocal (4 + sizeof T) + nglobal sizeof T   (+ nlocal sizeof T with --sign)
    assemble         the same + 4 nglobal
    gs               4 nglobal + (4 + 2 sizeof T) per shared coefficient
The setup (sf_gs_setup, blocking) is timed with the host clock, best of three.
--helmholtz also times global_to_local -> sf_helmholtz_hex_f64 -> assemble at nq 8 beside the operator alone: what assembly
costs a solver iteration.  --check compares every call with torch's result (assemble: to rounding, the orders differ).

    python3 gpu-benchmarking_amd/tools/gs_bench.py [--sign] [--f32] [--helmholtz] [--check] [--hex 64] [--quad 1024]
                                                   [--json FILE]
"""
import sys
import time

import opbench
from opbench import ms, roofline

opbench.importable("tests")
from gs_ref import multiplicity, structured_map  # noqa: E402  (the map builder the tests use)


def options(argv=None):
    ap = opbench.parser(__doc__, nelmt=None, reps=20, hex=(int, 64, "elements per direction of the hex mesh (0: skip)"),
                        quad=(int, 1024, "elements per direction of the quad mesh (0: skip)"),
                        check="compare with torch's results", variant=None)
    ap.add_argument("--nq", type=int, default=8)
    ap.add_argument("--sign", action="store_true", help="with a sign array (torch: a multiply more)")
    ap.add_argument("--helmholtz", action="store_true", help="hex fp64: the operator alone and between Q and Q^T")
    return ap.parse_args(argv)


def main(argv=None):
    args = options(argv)

    import numpy as np
    s = opbench.Session(args)
    torch, sf, dev, timed = s.torch, s.sf, s.dev, s.timed
    nq, nm = args.nq, args.nq - 1
    res = {"protocol": f"{args.reps} groups of 8 back-to-back launches (bench.py grouped_ms); frac = algorithmic bytes / "
                       "time / 8 TB/s; *_torch = torch's formulation on the same buffers",
           "device": s.device_name, "nq": nq, "sign": args.sign, "gs": {}}

    meshes = [("hex", (args.hex,) * 3)] * bool(args.hex) + [("quad", (args.quad,) * 2)] * bool(args.quad)
    for shape, nel in meshes:
        l2g_h, nglobal = structured_map(nel, nm)
        nlocal = l2g_h.size
        nshared = int(np.count_nonzero(multiplicity(l2g_h, nglobal)[l2g_h] >= 2))
        l2g = torch.from_numpy(l2g_h).to(dev)
        idx64 = l2g.to(torch.int64)                                   # torch's index, outside the timed region
        del l2g_h
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gsmap = sf.gs_setup(l2g, nglobal)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        mesh = {"nel": list(nel), "nlocal": nlocal, "nglobal": nglobal, "shared": nshared, "setup_ms": round(best, 3)}
        print(f"gs {shape} {nel}: nlocal {nlocal} nglobal {nglobal} shared {nshared} setup {best:.3f} ms", flush=True)
        for tname, dtype, size in s.dtypes():
            loc = sf.fill_random(nlocal, 1, dtype=dtype, device=dev)
            glo = sf.fill_random(nglobal, 2, dtype=dtype, device=dev)
            out_l, out_g = torch.empty_like(loc), torch.empty_like(glo)
            t_l, t_g, tmp = torch.empty_like(loc), torch.empty_like(glo), torch.empty_like(loc)
            sign = None
            if args.sign:
                sign = torch.where(sf.fill_random(nlocal, 3, dtype=dtype, device=dev) < 0, -1.0, 1.0).to(dtype)
            # not per element, so not in opbench's table: index and value traffic of the map (module docstring)
            nb_l = nlocal * (4 + size) + nglobal * size + (nlocal * size if args.sign else 0)
            nb_g = nb_l + 4 * nglobal
            nb_s = 4 * nglobal + (4 + 2 * size) * nshared

            def torch_g2l(dst=t_l, src=glo):
                torch.index_select(src, 0, idx64, out=dst)
                if sign is not None:
                    dst.mul_(sign)

            def torch_asm(dst=t_g, src=loc):
                dst.zero_()
                if sign is not None:
                    torch.mul(src, sign, out=tmp)
                    src = tmp
                dst.index_add_(0, idx64, src)

            work = loc.clone()

            def torch_gs():
                torch_asm(t_g, work)
                torch_g2l(work, t_g)

            cases = [("global_to_local", lambda: sf.global_to_local(gsmap, glo, sign=sign, out=out_l), torch_g2l, nb_l),
                     ("assemble", lambda: sf.assemble(gsmap, loc, sign=sign, out=out_g), torch_asm, nb_g),
                     ("gs", lambda: sf.gs(gsmap, work, sign=sign), torch_gs, nb_s)]
            rows = {}
            for name, ours, theirs, nb in cases:
                work.copy_(loc)                     # gs runs in place over and over: the values overflow, the time is theirs
                mean_ms, min_ms = timed(ours)
                work.copy_(loc)
                t_mean, t_min = timed(theirs)
                rows[name] = {"ms": ms(mean_ms), "ms_min": ms(min_ms), **roofline(nb, mean_ms, min_ms),
                              "ms_torch": ms(t_mean), "ms_torch_min": ms(t_min),
                              "speedup_vs_torch": round(t_mean / mean_ms, 3), "at_least_as_fast": bool(mean_ms <= t_mean)}
                print(f"gs {shape} {tname} {name}: {rows[name]}", flush=True)
            if args.check:
                ours_l = sf.global_to_local(gsmap, glo, sign=sign, out=out_l)
                ours_g = sf.assemble(gsmap, loc, sign=sign, out=out_g)
                torch_g2l()
                torch_asm()
                work.copy_(loc)
                sf.gs(gsmap, work, sign=sign)
                mine = work.clone()
                work.copy_(loc)
                torch_gs()
                torch.cuda.synchronize()
                rows["check"] = {"global_to_local_equal": bool(torch.equal(ours_l, t_l)),
                                 "assemble_rel_diff": float((ours_g - t_g).abs().max() / t_g.abs().max()),
                                 "gs_rel_diff": float((mine - work).abs().max() / work.abs().max())}
                print(f"gs {shape} {tname} check: {rows['check']}", flush=True)
            if args.helmholtz and shape == "hex" and tname == "f64":
                nelmt, ext = int(np.prod(nel)), (nq,) * 3
                b = sf.fill_random(nm * nq, 3, device=dev)
                d = sf.fill_random(nq * nq, 4, device=dev)
                g = sf.fill_random(nelmt * 6 * nq ** 3, 5, device=dev)
                w = sf.fill_random(nelmt * nq ** 3, 6, device=dev)
                y = torch.empty_like(loc)

                def operator():
                    sf.helmholtz_hex(ext, b, b, b, d, d, d, g, w, 0.75, out_l, out=y)

                def assembled():
                    sf.global_to_local(gsmap, glo, sign=sign, out=out_l)
                    operator()
                    sf.assemble(gsmap, y, sign=sign, out=out_g)

                sf.global_to_local(gsmap, glo, sign=sign, out=out_l)
                o_mean, o_min = timed(operator)
                a_mean, a_min = timed(assembled)
                rows["helmholtz"] = {"ms_operator": ms(o_mean), "ms_operator_min": ms(o_min),
                                     "ms_assembled": ms(a_mean), "ms_assembled_min": ms(a_min),
                                     "assembled_over_operator": round(a_mean / o_mean, 3)}
                print(f"gs {shape} {tname} helmholtz nq {nq}: {rows['helmholtz']}", flush=True)
                del b, d, g, w, y
            mesh[tname] = rows
            del loc, glo, out_l, out_g, t_l, t_g, tmp, work, sign
            s.free()
        res["gs"][shape] = mesh
        del gsmap, l2g, idx64
        s.free()
    s.emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
