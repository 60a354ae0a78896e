"""What the operator timing tools (tools/*_bench.py) share: the command line, the session (library, device, grouped_ms
with the graph-replay flag), the sweep over dtype x dimension x order, the rates with their rounding, the JSON line, the
table of algorithmic scalars per element behind every roofline fraction, and the two chain pieces several tools use.

Importing this module needs no GPU and does not load the library: torch and the package are loaded by Session().  A new
family's tool is its docstring, its own flags, its chain and the body of one case:

    ap = opbench.parser(__doc__, chain="...", check="...")
    s = opbench.Session(ap.parse_args(argv))
    res = {"protocol": ..., "device": s.device_name, "family": {}}
    s.collect(res["family"], lambda c: case(s, c))      # case() returns the row of one (dtype, dim, nq)
    s.emit(res)
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def importable(*parts):
    """Put ROOT/parts on the module search path."""
    p = os.path.join(ROOT, *parts)
    if p not in sys.path:
        sys.path.insert(0, p)


importable()

from bench import HBM_PEAK_GBS, grouped_ms  # noqa: E402  (the protocol of bench.py extras())


# ---- command line ----------------------------------------------------------------------------------------------------

def orders(s):
    return [int(x) for x in s.split(",") if x]


def parser(doc, *, nelmt="split", reps=40, hex=(orders, [4, 6, 8]), quad=(orders, [8, 12, 16]), f32="--f32",
           repeats=None, chain=None, check=None, variant="fp64 route: auto, wave or generic"):
    """The options the tools share; the caller adds its own.  nelmt: "split" (--nelmt3 / --nelmt2), "single" (--nelmt) or
    None; hex / quad: (type, default[, help]); f32: "--f32" (opt in) or "--no-f32" (opt out); repeats: None or
    (default, help); chain / check / variant: the help text, None for a tool without the option."""
    ap = argparse.ArgumentParser(description=doc.splitlines()[0])
    if nelmt == "split":
        ap.add_argument("--nelmt3", type=int, default=1 << 18)
        ap.add_argument("--nelmt2", type=int, default=1 << 20)
    elif nelmt == "single":
        ap.add_argument("--nelmt", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=reps)
    if repeats is not None:
        ap.add_argument("--repeats", type=int, default=repeats[0], help=repeats[1])
    for flag, (kind, default, *text) in (("--hex", hex), ("--quad", quad)):
        ap.add_argument(flag, type=kind, default=default, help=text[0] if text else None)
    ap.add_argument(f32, action="store_true", help="fp32 as well" if f32 == "--f32" else "fp64 only")
    for flag, text in (("--chain", chain), ("--check", check)):
        if text is not None:
            ap.add_argument(flag, action="store_true", help=text)
    if variant is not None:
        ap.add_argument("--variant", default="auto", help=variant)
    ap.add_argument("--json", default=None, help="write the result here as well")
    return ap


# ---- rates, with the rounding of every recorded log ------------------------------------------------------------------

def ms(t):
    return round(t, 5)


def frac(nbytes, t_ms):
    return round(nbytes / t_ms * 1e-6 / HBM_PEAK_GBS, 4)


def gb_s(nbytes, t_ms):
    return round(nbytes / t_ms * 1e-6, 1)


def gdof_s(ndof, t_ms):
    return round(ndof / t_ms * 1e-6, 2)


def roofline(nbytes, mean_ms, min_ms):
    return {"gb_s": gb_s(nbytes, mean_ms), "frac_mean": frac(nbytes, mean_ms), "frac_min": frac(nbytes, min_ms)}


def fracs(name, nbytes, mean_ms, min_ms):
    return {f"{name}_frac_mean": frac(nbytes, mean_ms), f"{name}_frac_min": frac(nbytes, min_ms)}


def chain_row(mean_ms, c_mean, c_min, prefix="t", bar=True):
    """The chain's columns beside a fused time: t_chain, t_chain_min, speedup_vs_chain and, with `bar`, the verdict."""
    row = {f"{prefix}_chain": ms(c_mean), f"{prefix}_chain_min": ms(c_min), "speedup_vs_chain": round(c_mean / mean_ms, 3)}
    if bar:
        row["not_slower_than_chain"] = mean_ms <= c_mean
    return row


# ---- algorithmic scalars per element: the denominator of every roofline fraction -------------------------------------
# k: nmt = nm^d, npt = nq^d (nm = nq - 1), dd = d^2, ncomp = d(d+1)/2, ncurl = d(d-1)/2.  Reads of the basis, derivative
# and quadrature arrays are not counted: they depend on the order only.

_SCALARS = {
    "bwdtrans": lambda k: k.nmt + k.npt,
    "iproduct": lambda k: k.nmt + k.npt,
    "mass": lambda k: 2 * k.nmt + k.npt,
    "helmholtz": lambda k, w=True: 2 * k.nmt + (k.ncomp + bool(w)) * k.npt,
    "affine_helmholtz": lambda k, je=True: 2 * k.nmt + k.ncomp + bool(je),
    "affine_helmholtz_deformed": lambda k, je=True: 2 * k.nmt + (k.ncomp + bool(je)) * k.npt,
    "diag_helmholtz": lambda k, w=True: (k.ncomp + bool(w)) * k.npt + k.nmt,
    "physderiv": lambda k, df=True: k.nmt + (k.dd * bool(df) + k.d) * k.npt,
    "iprodderiv": lambda k, df=True, w=True: (k.dd * bool(df) + k.d + bool(w)) * k.npt + k.nmt,
    "affine_physderiv": lambda k: k.nmt + k.d * k.npt + k.dd,
    "affine_iprodderiv": lambda k, je=True: k.d * k.npt + k.nmt + k.dd + bool(je),
    "geom": lambda k: k.d * k.nmt + (k.dd + k.ncomp + 2) * k.npt,
    "advect": lambda k, nf=None: (k.dd + k.d + 1) * k.npt + 2 * (k.d if nf is None else nf) * k.nmt,
    "affine_advect": lambda k, je=True: k.d * k.npt + 2 * k.d * k.nmt + k.dd + bool(je),
    "vecgrad": lambda k, outputs=("grad", "div", "curl"):
        k.d * k.nmt + (k.dd + k.dd * ("grad" in outputs) + ("div" in outputs) + k.ncurl * ("curl" in outputs)) * k.npt,
    "tensor": lambda k, ni, no: ni ** k.d + no ** k.d,
}


def scalars(op, dim, nq=None, **options):
    """Scalars one element reads and writes in `op` at nq points (nq - 1 modes) per direction; tensor takes ni, no."""
    k = SimpleNamespace(d=dim, dd=dim * dim, ncomp=dim * (dim + 1) // 2, ncurl=dim * (dim - 1) // 2,
                        nmt=None if nq is None else (nq - 1) ** dim, npt=None if nq is None else nq ** dim)
    return int(_SCALARS[op](k, **options))


# ---- chain pieces more than one tool uses ----------------------------------------------------------------------------

def ref_derivs(torch, dim, nq, nelmt, ds):
    """deriv(u, du): du[a] = D_a u on a point image u by torch.matmul over views, into the preallocated du."""
    dT0 = ds[0].view(nq, nq).t().contiguous()
    dm = [d.view(nq, nq) for d in ds]

    def deriv(u, du):
        torch.matmul(u.view(-1, nq), dT0, out=du[0].view(-1, nq))               # du_0[.., i] = sum_m D0[i][m] u[.., m]
        torch.matmul(dm[1], u.view(-1, nq, nq), out=du[1].view(-1, nq, nq))     # du_1[.., j, i] = sum_m D1[j][m] u[.., m, i]
        if dim == 3:
            torch.matmul(dm[2], u.view(nelmt, nq, -1), out=du[2].view(nelmt, nq, -1))

    return deriv


def point_weights(torch, dim, qw):
    """The quadrature weights of one element's points, qw x ... x qw."""
    q = qw
    for _ in range(dim - 1):
        q = torch.outer(qw, q.reshape(-1)).reshape(-1)                          # qw_d * (the product so far)
    return q


def expand_affine(torch, dim, nelmt, npt, qw, dfe=None, je=None):
    """The planes (df, w) of a deformed call from an affine call's constants, expanded on the device in the working
    precision: df repeats dfe at every point, w = je x point weights.  A constant left out gives None."""
    df = w = None
    if dfe is not None:
        n = dfe.numel() // nelmt
        df = dfe.view(nelmt, n, 1).expand(nelmt, n, npt).contiguous().reshape(-1)
    if je is not None:
        w = (je.view(nelmt, 1) * point_weights(torch, dim, qw).view(1, -1)).reshape(-1).contiguous()
    return df, w


# ---- session and sweep -----------------------------------------------------------------------------------------------

class Session:
    """The library on cuda:0, the parsed options, and the graph-replay flag of everything timed so far."""

    def __init__(self, args):
        import torch
        import __graft_entry__ as ge
        self.args, self.torch, self.sf = args, torch, ge.load_package()
        self.dev = torch.device("cuda:0")
        self.device_name = self.sf.device_info()["name"]
        self.replayed = True

    def timed(self, fn):
        mean_ms, min_ms, graphed = grouped_ms(self.torch, fn, self.args.reps)
        self.replayed = self.replayed and graphed
        return mean_ms, min_ms

    def dtypes(self):
        """(tname, dtype, sizeof) of every precision asked for."""
        f32 = not self.args.no_f32 if hasattr(self.args, "no_f32") else self.args.f32
        for tname, dtype in [("f64", self.torch.float64)] + ([("f32", self.torch.float32)] if f32 else []):
            yield tname, dtype, self.torch.finfo(dtype).bits // 8

    def free(self):
        self.torch.cuda.empty_cache()

    def _case(self, tname, dtype, size, dim, nq, nelmt):
        sf, dev, nm, shape = self.sf, self.dev, nq - 1, "hex" if dim == 3 else "quad"
        f64_kw = hasattr(self.args, "variant") and dtype == self.torch.float64

        def fill(n, seed):
            return sf.fill_random(n, seed, dtype=dtype, device=dev)

        def nbytes(op, **options):
            return size * nelmt * scalars(op, dim, nq, **options)

        return SimpleNamespace(
            tname=tname, dtype=dtype, size=size, kw={"variant": self.args.variant} if f64_kw else {},
            dim=dim, nq=nq, nm=nm, nmt=nm ** dim, npt=nq ** dim, ext=(nq,) * dim, nelmt=nelmt, key=f"{shape}_{tname}",
            label=f"{dim}D {tname} nq {nq:2d}", fill=fill, nbytes=nbytes, op=lambda name: getattr(sf, f"{name}_{shape}"),
            bs=(fill(nm * nq, 3),) * dim, ds=(fill(nq * nq, 4),) * dim)

    def sweep(self):
        """One case per dtype, dimension and order; the cache is freed after each."""
        a = self.args
        n3, n2 = (a.nelmt, a.nelmt) if hasattr(a, "nelmt") else (a.nelmt3, a.nelmt2)
        for tname, dtype, size in self.dtypes():
            for dim, nqs, nelmt in ((3, a.hex, n3), (2, a.quad, n2)):
                for nq in nqs:
                    yield self._case(tname, dtype, size, dim, nq, nelmt)
                    self.free()

    def collect(self, table, case):
        """table[hex_f64 | quad_f32 | ...][nq] = case(c) over the sweep; case's buffers die with its frame."""
        for c in self.sweep():
            table.setdefault(c.key, {})[str(c.nq)] = case(c)

    def versus_deformed(self, c, affine, deformed, a_sc, d_sc, oa, od):
        """The row of an affine call beside its deformed call on expanded planes; with --check also whether their
        outputs oa, od hold the same bits (and are not all zero)."""
        a_mean, a_min = self.timed(affine)
        d_mean, d_min = self.timed(deformed)
        abytes, dbytes = c.size * c.nelmt * a_sc, c.size * c.nelmt * d_sc
        row = {"ms": ms(a_mean), "ms_min": ms(a_min), "scalars_per_element": a_sc, **roofline(abytes, a_mean, a_min),
               "ms_deformed": ms(d_mean), "ms_deformed_min": ms(d_min), "deformed_scalars_per_element": d_sc,
               "deformed_frac_mean": frac(dbytes, d_mean), "ratio": round(d_mean / a_mean, 3),
               "ratio_min": round(d_min / a_min, 3), "ok": bool(a_mean <= d_mean)}
        if self.args.check:
            self.torch.cuda.synchronize()
            row["bits_equal"] = bool(self.torch.equal(oa, od)) and float(oa.abs().max()) > 0
        return row

    def emit(self, res, **trailer):
        """Close `res` with the replay flag and the trailer, print it as one JSON line and write --json."""
        res["hip_graph_replay"] = self.replayed
        res.update(trailer)
        line = json.dumps(res)
        print(line)
        if self.args.json:
            with open(self.args.json, "w") as fh:
                fh.write(line + "\n")
