#!/usr/bin/env python3
"""Record what every operator entry point of libsumfact.so answers to calls it refuses before any HIP call.

Output: tests/golden/capi_return_codes.json -- pure data: per symbol one string, one character per case in the order of
cases(), the digit -rc of the SF_* code (0 SF_OK, 1 SF_EINVAL, 2 SF_EALIGN, 3 SF_ENOTBUILT).  It pins the validation
order of include/sumfact.h and, through the pair cases, which operand an output may not lie over, so that a change of the
host boundary can be replayed against it (tests/test_cabi_cpu.py::test_recorded_return_codes).  Record it from a build
of the commit *before* such a change:

    python3 tests/golden/make_capi_codes.py --lib <the parent's build>/lib/libsumfact.so

The calls are built from the argument types of capi.SYMBOLS alone, on dummy addresses that are never dereferenced: every
case is one the library answers without reaching the HIP runtime.  The symbols with a variant ask for SF_VARIANT_WAVE at
isotropic extents off every wave table (3D 12, 2D 25: BwdTrans has wave kernels for 2D 2..24 and 32); the others (AUTO only) get extents beyond the bounds of the
any-extent kernels (3D 17, 2D 33).  sf_bwdtrans_*_{f64,f32} have neither an overlap rule nor an extent bound, so a call
without a defect would launch: they take the cases with a defect only (EXCLUDED_FOR_BWDTRANS_AUTO), and so does the
case count.  A positive return code (a hipError_t) stops the run.  No GPU: the script refuses to start on a machine with
one, because a dummy pointer must never meet a real device.
"""
import argparse
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "capi_return_codes.json")

STEMS = ("bwdtrans", "iproduct", "mass", "helmholtz", "affine_helmholtz", "physderiv", "iprodderiv", "diag_helmholtz",
         "aff_physderiv", "aff_iprodderiv", "geom", "geom_affine", "advect", "aff_advect", "vecgrad", "tensor")
SYMBOL = re.compile(r"sf_(%s)_(hex|quad)_(f64|f32)(_variant)?$" % "|".join(STEMS))
WAVE, BLOCK_LDS = 1, 3                  # SF_VARIANT_WAVE; SF_VARIANT_BLOCK_LDS, which no family but BwdTrans takes
STEP = 0x10000000                       # the clean layout: pointer k at (k + 1) * 256 MiB, far beyond any operand's length
NELMT = 4
EXCLUDED_FOR_BWDTRANS_AUTO = ("clean", "+8", "alias")     # the kinds of case that sf_bwdtrans_*_{f64,f32} would launch


def operator_symbols(symbols):
    """The operator entry points among capi.SYMBOLS, in sorted order: sixteen stems, hex and quad, f64 / f64_variant / f32
    (sf_tensor_* also f32_variant, sf_geom_affine_* without a variant)."""
    names = sorted(n for n in symbols if SYMBOL.match(n))
    assert {SYMBOL.match(n).group(1) for n in names} == set(STEMS), "a stem has no symbol"
    return names


def _layout(name, argtypes):
    """Where the arguments of `name` are, from their types alone: [variant,] the extents (c_uint in front of the c_size_t
    nelmt), ints and a count (c_uint) behind them, the pointers (a c_double lambda among them), the stream last."""
    m = SYMBOL.match(name)
    dim, scalar, has_variant = (3 if m.group(2) == "hex" else 2), (8 if m.group(3) == "f64" else 4), bool(m.group(4))
    nelmt_at = argtypes.index(ctypes.c_size_t)
    assert argtypes[-1] is ctypes.c_void_p and argtypes.count(ctypes.c_size_t) == 1
    assert has_variant == (argtypes[0] is ctypes.c_int)
    extents = [k for k in range(nelmt_at) if argtypes[k] is ctypes.c_uint]
    pointers = [k for k in range(nelmt_at + 1, len(argtypes) - 1) if argtypes[k] is ctypes.c_void_p]
    assert len(extents) in (dim, 2 * dim) and len(pointers) >= 3
    return dim, scalar, has_variant, nelmt_at, extents, pointers


def cases(name, argtypes):
    """[(kind, label, args)] of `name`, deterministic.  kind is what EXCLUDED_FOR_BWDTRANS_AUTO names."""
    dim, scalar, has_variant, nelmt_at, extents, pointers = _layout(name, argtypes)
    extent = (12 if dim == 3 else 25) if has_variant else (17 if dim == 3 else 33)
    base = []
    for k, t in enumerate(argtypes):
        if k == 0 and has_variant:
            base.append(WAVE)
        elif k in extents:
            base.append(extent)
        elif k == nelmt_at:
            base.append(NELMT)
        elif t is ctypes.c_uint:
            base.append(dim)            # a count of fields behind nelmt: all of them
        elif t is ctypes.c_int:
            base.append(0)              # trans
        elif t is ctypes.c_double:
            base.append(1.0)            # lambda != 0: the weight is looked at
        elif k in pointers:
            base.append((pointers.index(k) + 1) * STEP)
        else:
            base.append(None)           # the stream
    out = []

    def case(kind, label, **changes):
        args = list(base)
        for k, v in changes.items():
            args[int(k[1:])] = v
        out.append((kind, label, tuple(args)))

    at = lambda k: "a%d" % k            # noqa: E731  keyword for argument k
    P = pointers
    case("clean", "clean")
    for n, k in enumerate(P):
        case("null", f"p{n} null", **{at(k): None})
    for n, k in enumerate(P):
        case("misaligned", f"p{n} +{scalar // 2}", **{at(k): base[k] + scalar // 2})
    for n, k in enumerate(P):
        case("+8", f"p{n} +8", **{at(k): base[k] + 8})
    for i, ki in enumerate(P):
        for j, kj in enumerate(P):
            if i != j:
                case("alias", f"p{j} = p{i}", **{at(kj): base[ki]})
                case("alias", f"p{j} = p{i} + {scalar}", **{at(kj): base[ki] + scalar})
    case("empty", "nelmt 0, every pointer null", **{at(nelmt_at): 0}, **{at(k): None for k in P})
    case("extent", "an extent of 1", **{at(extents[0]): 1})
    if has_variant:
        case("variant", "variant -1", a0=-1)
        case("variant", "variant 99", a0=99)
    # two defects at once: which one answers
    case("null", "p0 null, p1 misaligned", **{at(P[0]): None, at(P[1]): base[P[1]] + scalar // 2})
    case("misaligned", "p0 misaligned, last pointer = the one before", **{at(P[0]): base[P[0]] + scalar // 2,
                                                                          at(P[-1]): base[P[-2]]})
    bwdtrans = SYMBOL.match(name).group(1) == "bwdtrans"
    if has_variant and not bwdtrans:    # BwdTrans takes block-lds, and refuses no alias: it would launch
        case("alias", "last pointer = the one before, variant block-lds", a0=BLOCK_LDS, **{at(P[-1]): base[P[-2]]})
    if bwdtrans and not has_variant:
        out = [c for c in out if c[0] not in EXCLUDED_FOR_BWDTRANS_AUTO]
    assert len(out) == case_count(name, argtypes), name
    return out


def case_count(name, argtypes):
    """The number of cases of `name`, from the number of its pointers: asserted by cases() and by the replay test."""
    _, _, has_variant, _, _, pointers = _layout(name, argtypes)
    p = len(pointers)
    if SYMBOL.match(name).group(1) == "bwdtrans" and not has_variant:
        return 2 * p + 2 + 2            # null, misaligned; empty, extent; the two defect pairs that are kept
    if not has_variant:
        return 1 + 3 * p + 2 * p * (p - 1) + 2 + 2
    return 1 + 3 * p + 2 * p * (p - 1) + 2 + 2 + 2 + (SYMBOL.match(name).group(1) != "bwdtrans")


def replay(lib, symbols):
    """{symbol: [(label, rc)]} of every case, in order.  A positive rc stops the run: the call reached the HIP runtime."""
    got = {}
    for name in operator_symbols(symbols):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = symbols[name]
        rows = []
        for _, label, args in cases(name, symbols[name][1]):
            rc = fn(*args)
            if rc > 0:
                raise RuntimeError(f"{name}, {label}: rc {rc} is a hipError_t -- the case reached the HIP runtime")
            rows.append((label, rc))
        got[name] = rows
    return got


def encode(rows):
    assert all(-9 <= rc <= 0 for _, rc in rows)
    return "".join(str(-rc) for _, rc in rows)


def refuse_on_a_gpu():
    import torch
    if torch.cuda.is_available():
        raise SystemExit("make_capi_codes.py: this machine has a GPU; the dummy pointers must never meet a real device")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="libsumfact.so of the build to record (the parent commit's)")
    opts = ap.parse_args()
    refuse_on_a_gpu()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    symbols = ge.load_package().capi.SYMBOLS
    got = replay(ctypes.CDLL(os.path.abspath(opts.lib)), symbols)
    doc = {"_provenance": "recorded by tests/golden/make_capi_codes.py; one digit -rc per case, in the order of cases()",
           "symbols": {name: encode(rows) for name, rows in got.items()}}
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    total = sum(len(rows) for rows in got.values())
    print(f"wrote {OUT}: {len(got)} symbols, {total} cases")


if __name__ == "__main__":
    main()
