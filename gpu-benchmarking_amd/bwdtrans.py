"""Host-side mirror of the reference's kernel call sites, over torch device tensors.

torch is plumbing only (device memory, streams); all arithmetic happens in libsumfact.so.
Argument meaning follows the reference kernels (benchmark05/benchmark05.cc:291-297,
benchmark04/benchmark04.cc:353-358): extents nq (nm = nq-1), basis row-major nm x nq,
in[e][r][q][p], out[e][k][j][i].
"""
import collections
import ctypes
import itertools

import torch

from . import capi

VARIANTS = {"auto": 0, "wave": 1, "thread": 2, "block-lds": 3, "block-glb": 4, "generic": 5,
            "mfma": 6, "mfma4": 7, "wave-rt": 8}


def _stream(stream, device=None):
    """hipStream_t of `stream`, or of the current stream of `device` (the tensor's device, not the thread's)."""
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return ctypes.c_void_p(stream.cuda_stream)


def _check_operands(what, operands, inp, lam=None):
    """The C ABI takes raw pointers: a short operand would be read / written out of bounds, one of another dtype or device
    misread.  `operands`: (name, tensor, expected numel, may be None); a None stands for a term that lam == 0 switches off
    (in a family without lam: for an operand the call may leave out)."""
    for name, t, need, optional in operands:
        if t is None and optional:
            if lam is not None and lam != 0.0:
                raise ValueError(f"{what}: {name}=None needs lam == 0")
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor")
        if t.numel() != need:
            raise ValueError(f"{what}: {name} has {t.numel()} values, not {need}")
        if t.dtype != inp.dtype:
            raise ValueError(f"{what}: {name} is {t.dtype}, in is {inp.dtype}")
        if t.device != inp.device:
            raise ValueError(f"{what}: {name} is on {t.device}, in is on {inp.device}")


def _dev_ptr(t, name, dtype=torch.float64):
    """The device address of `t` as a ctypes pointer."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous {dtype} CUDA/HIP tensor")
    return ctypes.c_void_p(t.data_ptr())


def _variant(v):
    return VARIANTS[v] if isinstance(v, str) else int(v)


# ---- the steps every call path below shares ----------------------------------------------------------------------------
def _extents(what, nq):
    """(nq as ints, modes per element, points per element): nm = nq - 1 modes per direction."""
    nq = tuple(int(q) for q in nq)
    nmt, nqt = 1, 1
    for q in nq:
        nmt, nqt = nmt * (q - 1), nqt * q
    if nmt <= 0:
        raise capi.SumfactError(capi.SF_EINVAL, what)
    return nq, nmt, nqt


def _batch(what, t, per, name, unit):
    """The number of elements, from the operand that sizes the batch: t holds `per` `unit` per element."""
    nelmt = t.numel() // per
    if nelmt * per != t.numel():
        raise ValueError(f"{what}: {name}.numel() is not a multiple of the {unit} per element ({per})")
    return nelmt


def _entry(what, stem, f32, variant, f32_takes="auto"):
    """(the entry point, its leading arguments) of sf_<stem>_*.  variant None: the call has none.  float64 goes to
    _f64_variant; float32 to _f32, which is the AUTO route: f32_takes "auto" refuses any other variant, "any" quietly
    drops it (BwdTrans), "all" says there is an _f32_variant (sf_tensor_*)."""
    sfx = "f32" if f32 else "f64"
    if variant is None:
        return getattr(capi.lib(), f"sf_{stem}_{sfx}"), ()
    v = _variant(variant)
    if f32 and f32_takes == "auto" and v != VARIANTS["auto"]:
        raise ValueError(f"{what}: float32 has the AUTO route only")
    if f32 and f32_takes != "all":
        return getattr(capi.lib(), f"sf_{stem}_f32"), ()
    return getattr(capi.lib(), f"sf_{stem}_{sfx}_variant"), (v,)


def _refuse_overlap(what, outs, reads):
    """An output may not overlap what the call reads or an earlier output, as byte ranges.  outs, reads: (name, tensor)."""
    span = lambda t: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())       # noqa: E731
    for n, (oname, o) in enumerate(outs):
        lo, hi = span(o)
        for name, t in reads + outs[:n]:
            tl, th = span(t)
            if lo < th and tl < hi:
                raise capi.SumfactError(capi.SF_EINVAL, f"{what}: {oname} overlaps {name}")


def _launch(what, fn, like, stream, args):
    """fn(*args, stream) on like's device and its current stream; `args` may be lazy, it is read on that device."""
    with torch.cuda.device(like.device):
        rc = fn(*args, _stream(stream, like.device))
    capi.check(rc, what)


def hex_wsp_doubles(nq, nelmt):
    """Workspace the block-glb / thread variants need (benchmark05/benchmark05.cc:1243-1244)."""
    nq0, nq1, nq2 = nq
    return nelmt * (nq0 * (nq1 - 1) * (nq2 - 1) + nq0 * nq1 * (nq2 - 1))


def quad_wsp_doubles(nq, nelmt):
    """Workspace of the 2D block-glb / thread variants (benchmark04/benchmark04.cc:894)."""
    nq0, nq1 = nq
    return nelmt * nq0 * (nq1 - 1)


# What one operator family is to _operator_call: the stem of its symbols (sf_<stem>_{hex,quad}_{f64_variant,f32}); whether
# `inp` / `out` hold quadrature points per element (else modes); extras(nelmt, points per element) -> the operands between
# the bases and `in`, in the order of the C signature, as (name, tensor, expected numel, may be None); lam, or None for a
# family without one; whether float32 quietly takes the AUTO route for any `variant` (BwdTrans) or refuses all but "auto";
# BwdTrans only: wsp_need(nelmt) -> {variant: numel of the caller-owned workspace it needs}; out_parts: the number of
# separate output arrays of the C call (1: `out` is one flat tensor; d: `out` is a (d, n) tensor or a sequence of d tensors);
# inp_parts: the same for the input arrays (1: `inp` is one flat tensor; d: a (d, n) tensor or a sequence of d tensors; 0:
# the C call has no input array -- `inp` is then the operand that sizes the batch, `anchor`(points per element) values per
# element, listed among the extras and passed there only).
_Family = collections.namedtuple("_Family", "stem inp_points out_points extras lam f32_ignores_variant wsp_need out_parts "
                                 "inp_parts anchor", defaults=(lambda nelmt, nqt: [], None, False, None, 1, 1, None))


def _output_parts(what, out, parts, numel, inp):
    """(what the call returns, the `parts` flat tensors the C call writes) of a family with several outputs.  `out` is
    None: a (parts, numel) tensor is allocated whose rows each start 256-byte aligned, as a fresh allocation would (the
    rows are contiguous, the tensor as a whole need not be), so that an odd numel does not cost the wave route.  `out` is
    a tensor: (parts, numel) with contiguous rows, or any contiguous tensor of parts * numel values.  `out` is a sequence
    of `parts` tensors: returned as a tuple."""
    if out is None:
        per = 256 // inp.element_size()
        out = torch.empty((parts, (numel + per - 1) // per * per), dtype=inp.dtype, device=inp.device)[:, :numel]
    if isinstance(out, torch.Tensor):
        if out.numel() != parts * numel:
            raise ValueError(f"{what}: out has {out.numel()} values, not {parts} x {numel}")
        if not (out.dim() == 2 and out.shape[0] == parts and (numel <= 1 or out.stride(1) == 1)):
            if not out.is_contiguous():
                raise TypeError(f"{what}: out must be contiguous, or ({parts}, {numel}) with contiguous rows")
            out = out.view(parts, numel)
        return out, [out[a] for a in range(parts)]
    outs = list(out)
    if len(outs) != parts:
        raise ValueError(f"{what}: out holds {len(outs)} tensors, not {parts}")
    return tuple(outs), outs


def _input_parts(what, inp, parts):
    """The `parts` flat tensors the C call reads, of a family with several inputs.  `inp` is a (parts, n) tensor with
    contiguous rows (what physderiv_* returns: taken row by row, no copy, the tensor as a whole need not be contiguous),
    any contiguous tensor of parts * n values, or a sequence of `parts` flat tensors.  Every part has the size, dtype and
    device of the first."""
    if isinstance(inp, torch.Tensor):
        if not (inp.dim() == 2 and inp.shape[0] == parts and (inp.shape[1] <= 1 or inp.stride(1) == 1)):
            if inp.numel() % parts:
                raise ValueError(f"{what}: in has {inp.numel()} values, no multiple of its {parts} parts")
            if not inp.is_contiguous():
                raise TypeError(f"{what}: in must be contiguous, or ({parts}, n) with contiguous rows")
            inp = inp.view(parts, -1)
        ins = [inp[a] for a in range(parts)]
    else:
        ins = list(inp)
        if len(ins) != parts:
            raise ValueError(f"{what}: in holds {len(ins)} tensors, not {parts}")
        for a, t in enumerate(ins):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}: in{a} must be a tensor")
    _check_operands(what, [(f"in{a}", t, ins[0].numel(), False) for a, t in enumerate(ins)], ins[0])
    return ins


def _operator_call(what, fam, nq, bases, inp, out, variant, stream, wsp=None):
    """The one call path of bwdtrans_* / iproduct_* / mass_* / helmholtz_* / affine_helmholtz_* / physderiv_* /
    iprodderiv_* / affine_physderiv_* / affine_iprodderiv_* / diag_helmholtz_*: sizes, dtypes and devices are checked here (before any library call), pointers, alignment and overlap in
    the C ABI."""
    ins = None
    if fam.inp_parts > 1:               # every part like the first, which stands for them below
        ins = _input_parts(what, inp, fam.inp_parts)
        inp = ins[0]
    nq, nmt, nqt = _extents(what, nq)
    n_in, n_out = nqt if fam.inp_points else nmt, nqt if fam.out_points else nmt
    if fam.inp_parts == 0:
        if not isinstance(inp, torch.Tensor):
            raise TypeError(f"{what}: the operand that sizes the batch must be a tensor")
        n_in = fam.anchor(nqt)
    nelmt = _batch(what, inp, n_in, "in" if fam.inp_parts else "the operand that sizes the batch",
                   "values" if not fam.inp_parts else "points" if fam.inp_points else "modes")
    if fam.out_parts > 1:
        out, outs = _output_parts(what, out, fam.out_parts, nelmt * n_out, inp)
    else:
        if out is None:
            out = torch.empty(nelmt * n_out, dtype=inp.dtype, device=inp.device)
        outs = [out]
    out_names = ["out"] if len(outs) == 1 else [f"out{a}" for a in range(len(outs))]
    lam = None if fam.lam is None else float(fam.lam)
    operands = [(f"basis{d}", b, (q - 1) * q, False) for d, (b, q) in enumerate(zip(bases, nq))]
    operands += fam.extras(nelmt, nqt)
    _check_operands(what, operands + [(name, t, nelmt * n_out, False) for name, t in zip(out_names, outs)], inp, lam)
    v, f32 = _variant(variant), inp.dtype == torch.float32
    if fam.wsp_need is not None:        # BwdTrans: the caller-owned workspace of the thread and block-glb variants
        need = fam.wsp_need(nelmt)
        if wsp is not None and wsp.numel() < need.get(v, 0):
            raise ValueError(f"{what}: wsp has {wsp.numel()} values, the variant needs {need[v]}")
        if wsp is None and not f32 and v in need and nelmt:
            wsp = torch.empty(max(need.values()), dtype=torch.float64, device=inp.device)
    fn, head = _entry(what, f"{fam.stem}_{'hex' if len(nq) == 3 else 'quad'}", f32, v,
                      "any" if fam.f32_ignores_variant else "auto")
    dtype = torch.float32 if f32 else torch.float64
    ptrs = [None if t is None else _dev_ptr(t, name, dtype) for name, t, _, _ in operands]
    if lam is not None:
        ptrs.append(ctypes.c_double(lam))
    if ins is not None:
        ptrs += [_dev_ptr(t, f"in{a}", dtype) for a, t in enumerate(ins)]
    elif fam.inp_parts:
        ptrs.append(_dev_ptr(inp, "in", dtype))
    if fam.wsp_need is not None and not f32:
        ptrs.append(None if wsp is None else _dev_ptr(wsp, "wsp", dtype))
    ptrs += [_dev_ptr(t, name, dtype) for name, t in zip(out_names, outs)]
    _launch(what, fn, inp, stream, (*head, *nq, nelmt, *ptrs))
    return out


def bwdtrans_hex(nq, basis0, basis1, basis2, inp, out=None, variant="auto", wsp=None, stream=None):
    """out[e][k][j][i] = sum_rqp in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k] on inp's device."""
    _, nq1, nq2 = nq
    fam = _Family("bwdtrans", False, True, f32_ignores_variant=True,       # T = float: AUTO strategy only
                  wsp_need=lambda n: {2: n * ((nq1 - 1) * (nq2 - 1) + (nq2 - 1)), 4: hex_wsp_doubles(nq, n)})
    return _operator_call("bwdtrans_hex", fam, nq, (basis0, basis1, basis2), inp, out, variant, stream, wsp)


def bwdtrans_hex_mfma4(nq, basis0, basis1, basis2, inp, direct, out=None, stream=None):
    """For tests and tuning: bwdtrans_hex((nq,) * 3, ..., variant="mfma4") in float64 with the kernel's output path named
    -- direct false: the element is assembled in LDS and streamed out flat; true: the accumulators of the third sweep are
    stored as they are.  variant="mfma4" and "auto" choose per order."""
    what, nq = "bwdtrans_hex_mfma4", int(nq)
    if nq < 2:
        raise capi.SumfactError(capi.SF_EINVAL, what)
    if not isinstance(inp, torch.Tensor):
        raise TypeError(f"{what}: in must be a tensor")
    nmt, nqt = (nq - 1) ** 3, nq ** 3
    nelmt = _batch(what, inp, nmt, "in", "modes")
    if out is None:
        out = torch.empty(nelmt * nqt, dtype=inp.dtype, device=inp.device)
    operands = [(f"basis{d}", b, (nq - 1) * nq, False) for d, b in enumerate((basis0, basis1, basis2))]
    operands += [("in", inp, nelmt * nmt, False), ("out", out, nelmt * nqt, False)]
    _check_operands(what, operands, inp)
    _launch(what, capi.lib().sf_bwdtrans_hex_f64_mfma4, inp, stream,
            itertools.chain((int(bool(direct)), nq, nelmt), (_dev_ptr(t, name) for name, t, _, _ in operands)))
    return out


def bwdtrans_quad(nq, basis0, basis1, inp, out=None, variant="auto", wsp=None, stream=None):
    """out[e][j][i] = sum_qp in[e][q][p] B0[p][i] B1[q][j] on inp's device."""
    fam = _Family("bwdtrans", False, True, f32_ignores_variant=True,
                  wsp_need=lambda n: {2: n * (nq[1] - 1), 4: quad_wsp_doubles(nq, n)})
    return _operator_call("bwdtrans_quad", fam, nq, (basis0, basis1), inp, out, variant, stream, wsp)


_IPROD = _Family("iproduct", True, False)


def iproduct_hex(nq, basis0, basis1, basis2, inp, out=None, variant="auto", stream=None):
    """IProductWRTBase, the transpose of bwdtrans_hex: out[e][r][q][p] = sum_kji in[e][k][j][i] B0[p][i] B1[q][j]
    B2[r][k] on inp's device.  Same bases as bwdtrans_hex; inp holds nq0*nq1*nq2 values per element, out nm0*nm1*nm2.
    float64 takes variant "auto", "wave" or "generic"; float32 the AUTO route."""
    return _operator_call("iproduct_hex", _IPROD, nq, (basis0, basis1, basis2), inp, out, variant, stream)


def iproduct_quad(nq, basis0, basis1, inp, out=None, variant="auto", stream=None):
    """IProductWRTBase, the transpose of bwdtrans_quad: out[e][q][p] = sum_ji in[e][j][i] B0[p][i] B1[q][j]."""
    return _operator_call("iproduct_quad", _IPROD, nq, (basis0, basis1), inp, out, variant, stream)


def _mass(w):
    return _Family("mass", False, False, lambda nelmt, nqt: [("w", w, nelmt * nqt, False)])


def mass_hex(nq, basis0, basis1, basis2, w, inp, out=None, variant="auto", stream=None):
    """The fused mass operator B^T diag(w) B in one kernel: out[e][r'][q'][p'] = sum_kji B0[p'][i] B1[q'][j] B2[r'][k]
    w[e][k][j][i] (sum_rqp in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k]) on inp's device.  The bases of bwdtrans_hex; inp and
    out hold nm0*nm1*nm2 modes per element, w nq0*nq1*nq2 weights per element.  out may not overlap inp or w.  float64
    takes variant "auto", "wave" or "generic"; float32 the AUTO route.  A plain function: no autograd."""
    return _operator_call("mass_hex", _mass(w), nq, (basis0, basis1, basis2), inp, out, variant, stream)


def mass_quad(nq, basis0, basis1, w, inp, out=None, variant="auto", stream=None):
    """The fused mass operator in 2D: out[e][q'][p'] = sum_ji B0[p'][i] B1[q'][j] w[e][j][i] (sum_qp in[e][q][p] B0[p][i]
    B1[q][j])."""
    return _operator_call("mass_quad", _mass(w), nq, (basis0, basis1), inp, out, variant, stream)


def _per_direction(name, tensors, numel, nq):
    return [(f"{name}{d}", t, numel(int(q)), False) for d, (t, q) in enumerate(zip(tensors, nq))]


def _helmholtz(nq, derivs, g, w, lam):
    ncomp = len(nq) * (len(nq) + 1) // 2
    return _Family("helmholtz", False, False, lambda nelmt, nqt: _per_direction("deriv", derivs, lambda q: q * q, nq) + [
        ("g", g, nelmt * ncomp * nqt, False), ("w", w, nelmt * nqt, True)], lam)


def helmholtz_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, g, w, lam, inp, out=None, variant="auto",
                  stream=None):
    """The fused Helmholtz operator y_e = B^T [lam diag(w_e) + sum_ab D_a^T diag(G_ab,e) D_b] B x_e in one kernel, on
    inp's device.  The bases of bwdtrans_hex; deriv_d row-major nq_d x nq_d with (D_d u)[i] = sum_m deriv_d[i][m] u[m];
    g[e][c][k][j][i] with c = 0..5 for (00, 01, 02, 11, 12, 22); w[e][k][j][i], or None with lam == 0 (the Laplacian);
    inp and out hold nm0*nm1*nm2 modes per element.  out may not overlap inp, g or w.  float64 takes variant "auto",
    "wave" or "generic"; float32 the AUTO route.  A plain function: no autograd."""
    return _operator_call("helmholtz_hex", _helmholtz(nq, (deriv0, deriv1, deriv2), g, w, lam), nq,
                          (basis0, basis1, basis2), inp, out, variant, stream)


def helmholtz_quad(nq, basis0, basis1, deriv0, deriv1, g, w, lam, inp, out=None, variant="auto", stream=None):
    """The fused Helmholtz operator in 2D: g[e][c][j][i] with c = 0..2 for (00, 01, 11), w[e][j][i] or None with
    lam == 0."""
    return _operator_call("helmholtz_quad", _helmholtz(nq, (deriv0, deriv1), g, w, lam), nq, (basis0, basis1), inp, out,
                          variant, stream)


def _affine(nq, derivs, qws, ge, je, lam):
    ncomp = len(nq) * (len(nq) + 1) // 2
    return _Family("affine_helmholtz", False, False, lambda nelmt, nqt: (
        _per_direction("deriv", derivs, lambda q: q * q, nq) + _per_direction("qw", qws, lambda q: q, nq)
        + [("ge", ge, nelmt * ncomp, False), ("je", je, nelmt, True)]), lam)


def affine_helmholtz_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, qw0, qw1, qw2, ge, je, lam, inp, out=None,
                         variant="auto", stream=None):
    """The fused Helmholtz operator on affine elements in one kernel, on inp's device: helmholtz_hex with
    g[e][c][k][j][i] = ge[e][c] qw2[k] qw1[j] qw0[i] and w[e][k][j][i] = je[e] qw2[k] qw1[j] qw0[i].  The bases and
    derivative matrices of helmholtz_hex; qw_d the nq_d one-dimensional quadrature weights; ge[e][c] with c = 0..5 for
    (00, 01, 02, 11, 12, 22), the element's |det J| J^-1 J^-T; je[e] = |det J|, or None with lam == 0 (the Laplacian).
    out may not overlap inp, ge or je.  float64 takes variant "auto", "wave" or "generic"; float32 the AUTO route.  A
    plain function: no autograd."""
    return _operator_call("affine_helmholtz_hex", _affine(nq, (deriv0, deriv1, deriv2), (qw0, qw1, qw2), ge, je, lam), nq,
                          (basis0, basis1, basis2), inp, out, variant, stream)


def affine_helmholtz_quad(nq, basis0, basis1, deriv0, deriv1, qw0, qw1, ge, je, lam, inp, out=None, variant="auto",
                          stream=None):
    """The fused Helmholtz operator on affine elements in 2D: ge[e][c] with c = 0..2 for (00, 01, 11), je[e] or None with
    lam == 0."""
    return _operator_call("affine_helmholtz_quad", _affine(nq, (deriv0, deriv1), (qw0, qw1), ge, je, lam), nq,
                          (basis0, basis1), inp, out, variant, stream)


def _physderiv(nq, derivs, df):
    d = len(nq)
    return _Family("physderiv", False, True, lambda nelmt, nqt: _per_direction("deriv", derivs, lambda q: q * q, nq) + [
        ("df", df, nelmt * d * d * nqt, True)], out_parts=d)


def physderiv_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, df, inp, out=None, variant="auto", stream=None):
    """BwdTrans fused with the physical-space gradient in one kernel, on inp's device: with u = B x_e and du_b = D_b u,
    out[a][e][k][j][i] = sum_b df[e][3 a + b][k][j][i] du_b[e][k][j][i].  The bases and derivative matrices of
    helmholtz_hex; df[e][c][k][j][i] the nine planes of the inverse Jacobian, c = 3 a + b for d xi_b / d x_a, or None for
    the reference-space derivatives out[a] = du_a (df is then never read); inp holds nm0*nm1*nm2 modes per element.
    Returns one tensor of shape (3, nelmt * nq0*nq1*nq2) whose rows are the three outputs of the C call, each in the
    layout of bwdtrans_hex's output (rows contiguous and 256-byte aligned; the tensor as a whole need not be
    contiguous); `out` may be such a tensor, or a sequence of three flat tensors (then returned as a tuple).  No output may overlap inp, df or another output.  float64 takes variant "auto", "wave" or "generic"; float32
    the AUTO route.  A plain function: no autograd."""
    return _operator_call("physderiv_hex", _physderiv(nq, (deriv0, deriv1, deriv2), df), nq, (basis0, basis1, basis2), inp,
                          out, variant, stream)


def physderiv_quad(nq, basis0, basis1, deriv0, deriv1, df, inp, out=None, variant="auto", stream=None):
    """BwdTrans fused with the physical-space gradient in 2D: out[a][e][j][i] = sum_b df[e][2 a + b][j][i] du_b[e][j][i],
    four planes of df (or None), a (2, nelmt * nq0*nq1) result."""
    return _operator_call("physderiv_quad", _physderiv(nq, (deriv0, deriv1), df), nq, (basis0, basis1), inp, out, variant,
                          stream)


def _iprodderiv(nq, derivs, df, w):
    d = len(nq)
    return _Family("iprodderiv", True, False, lambda nelmt, nqt: _per_direction("deriv", derivs, lambda q: q * q, nq) + [
        ("df", df, nelmt * d * d * nqt, True), ("w", w, nelmt * nqt, True)], inp_parts=d)


def iprodderiv_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, df, w, inp, out=None, variant="auto", stream=None):
    """IProductWRTDerivBase, the weak divergence and the transpose of physderiv_hex, in one kernel on inp's device: with
    g_b = w sum_a df[e][3 a + b] inp[a] per point, out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p].  The bases,
    derivative matrices and df of physderiv_hex (the sum runs over the row index a of df), or df=None for g_b = w inp[b];
    w[e][k][j][i] as in mass_hex, or None for no weight (then the exact transpose of physderiv_hex on the same df); df and
    w are never read when None.  inp: the three point arrays, each in the layout of bwdtrans_hex's output -- a (3, n)
    tensor with contiguous rows (what physderiv_hex returns, taken without a copy), a contiguous tensor of 3 n values, or
    a sequence of three flat tensors.  out holds nm0*nm1*nm2 modes per element and may not overlap an input, df or w.
    float64 takes variant "auto", "wave" or "generic"; float32 the AUTO route.  A plain function: no autograd."""
    return _operator_call("iprodderiv_hex", _iprodderiv(nq, (deriv0, deriv1, deriv2), df, w), nq, (basis0, basis1, basis2),
                          inp, out, variant, stream)


def iprodderiv_quad(nq, basis0, basis1, deriv0, deriv1, df, w, inp, out=None, variant="auto", stream=None):
    """IProductWRTDerivBase in 2D: g_b = w sum_a df[e][2 a + b] inp[a], out[e][q][p] = sum_b (B^T D_b^T g_b)[e][q][p]; four
    planes of df (or None), one of w (or None), inp a (2, n) tensor or a sequence of two flat tensors."""
    return _operator_call("iprodderiv_quad", _iprodderiv(nq, (deriv0, deriv1), df, w), nq, (basis0, basis1), inp, out,
                          variant, stream)


def _affine_physderiv(nq, derivs, dfe):
    d = len(nq)
    return _Family("aff_physderiv", False, True, lambda nelmt, nqt: _per_direction("deriv", derivs, lambda q: q * q, nq) + [
        ("dfe", dfe, nelmt * d * d, False)], out_parts=d)


def affine_physderiv_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, dfe, inp, out=None, variant="auto",
                         stream=None):
    """physderiv_hex on affine elements in one kernel, on inp's device: out[a][e][k][j][i] = sum_b dfe[e][3 a + b]
    du_b[e][k][j][i], with dfe[e][c] the nine constants of the element's inverse Jacobian, c = 3 a + b for d xi_b / d x_a
    (the order of the planes of physderiv_hex's df; required).  Bit for bit physderiv_hex on planes filled with the
    constants.  The bases, derivative matrices, inp, out and variants of physderiv_hex.  A plain function: no autograd."""
    return _operator_call("affine_physderiv_hex", _affine_physderiv(nq, (deriv0, deriv1, deriv2), dfe), nq,
                          (basis0, basis1, basis2), inp, out, variant, stream)


def affine_physderiv_quad(nq, basis0, basis1, deriv0, deriv1, dfe, inp, out=None, variant="auto", stream=None):
    """physderiv_quad on affine elements: out[a][e][j][i] = sum_b dfe[e][2 a + b] du_b[e][j][i], four constants per
    element, a (2, nelmt * nq0*nq1) result."""
    return _operator_call("affine_physderiv_quad", _affine_physderiv(nq, (deriv0, deriv1), dfe), nq, (basis0, basis1), inp,
                          out, variant, stream)


def _affine_iprodderiv(nq, derivs, qws, dfe, je):
    d = len(nq)
    unweighted = je is None             # the quadrature weights are then never read and may be None as well
    return _Family("aff_iprodderiv", True, False, lambda nelmt, nqt: (
        _per_direction("deriv", derivs, lambda q: q * q, nq)
        + [(f"qw{i}", t, int(q), unweighted) for i, (t, q) in enumerate(zip(qws, nq))]
        + [("dfe", dfe, nelmt * d * d, False), ("je", je, nelmt, True)]), inp_parts=d)


def affine_iprodderiv_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, qw0, qw1, qw2, dfe, je, inp, out=None,
                          variant="auto", stream=None):
    """iprodderiv_hex on affine elements in one kernel, the transpose of affine_physderiv_hex: with g_b = (je[e] qw2[k]
    (qw1[j] qw0[i])) sum_a dfe[e][3 a + b] inp[a] per point, out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p].  qw_d
    the one-dimensional quadrature weights and je[e] = |det J| as in affine_helmholtz_hex, dfe as in affine_physderiv_hex
    (required).  je=None: no weight at all, je and qw_d are never read (qw_d may then be None too) -- the exact transpose
    of affine_physderiv_hex.  With je, bit for bit iprodderiv_hex on df planes filled with the constants and w = je *
    (qw2 * (qw1 * qw0)).  inp, out and variants as iprodderiv_hex.  A plain function: no autograd."""
    return _operator_call("affine_iprodderiv_hex",
                          _affine_iprodderiv(nq, (deriv0, deriv1, deriv2), (qw0, qw1, qw2), dfe, je), nq,
                          (basis0, basis1, basis2), inp, out, variant, stream)


def affine_iprodderiv_quad(nq, basis0, basis1, deriv0, deriv1, qw0, qw1, dfe, je, inp, out=None, variant="auto",
                           stream=None):
    """iprodderiv_quad on affine elements: g_b = (je[e] qw1[j] qw0[i]) sum_a dfe[e][2 a + b] inp[a]; four constants per
    element, je[e] or None (then qw_d are never read)."""
    return _operator_call("affine_iprodderiv_quad", _affine_iprodderiv(nq, (deriv0, deriv1), (qw0, qw1), dfe, je), nq,
                          (basis0, basis1), inp, out, variant, stream)


def diag_tables(nq_d, basis, deriv, stream=None):
    """The three tables of one direction for diag_helmholtz_*: with E[p][i] = sum_m deriv[i][m] basis[p][m] (the
    derivative of mode p at point i), a flat tensor tab[t][p][i], t = 0, 1, 2, of basis * basis, E * basis and E * E: 3 nm nq
    values, on basis's device, in one small kernel.  They depend on the order only: build them once."""
    nq_d = int(nq_d)
    if nq_d < 2:
        raise capi.SumfactError(capi.SF_EINVAL, "diag_tables")
    if not isinstance(basis, torch.Tensor) or basis.dtype not in (torch.float64, torch.float32):
        raise TypeError("diag_tables: basis must be a float64 or float32 tensor")
    if basis.numel() != (nq_d - 1) * nq_d:
        raise ValueError(f"diag_tables: basis has {basis.numel()} values, not {(nq_d - 1) * nq_d}")
    _check_operands("diag_tables", [("deriv", deriv, nq_d * nq_d, False)], basis)
    f32 = basis.dtype == torch.float32
    ptrs = [_dev_ptr(basis, "basis", basis.dtype), _dev_ptr(deriv, "deriv", basis.dtype)]
    tab = torch.empty(3 * (nq_d - 1) * nq_d, dtype=basis.dtype, device=basis.device)
    with torch.cuda.device(basis.device):
        rc = (capi.lib().sf_diag_tables_f32 if f32 else capi.lib().sf_diag_tables_f64)(
            nq_d, *ptrs, _dev_ptr(tab, "tab", basis.dtype), _stream(stream, basis.device))
    capi.check(rc, "sf_diag_tables")
    return tab


def _diag(what, nq, bases, derivs, g, w, lam, out, variant, stream, tabs):
    nq = tuple(int(q) for q in nq)
    ncomp = len(nq) * (len(nq) + 1) // 2
    if tabs is None:
        if any(q < 2 for q in nq):
            raise capi.SumfactError(capi.SF_EINVAL, what)
        tabs = [diag_tables(q, b, d, stream) for q, b, d in zip(nq, bases, derivs)]
    tabs = tuple(tabs)
    if len(tabs) != len(nq):
        raise ValueError(f"{what}: tabs holds {len(tabs)} tensors, not {len(nq)}")
    fam = _Family("diag_helmholtz", False, False, lambda nelmt, nqt: _per_direction("tab", tabs, lambda q: 3 * (q - 1) * q, nq) + [
        ("g", g, nelmt * ncomp * nqt, False), ("w", w, nelmt * nqt, True)], lam, inp_parts=0, anchor=lambda nqt: ncomp * nqt)
    return _operator_call(what, fam, nq, (), g, out, variant, stream)


def diag_helmholtz_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, g, w, lam, out=None, variant="auto", stream=None,
                       tabs=None):
    """The diagonal of helmholtz_hex's operator, per element, in one kernel on g's device: out[e][r][q][p] =
    (B^T [lam diag(w_e) + sum_ab D_a^T diag(G_ab,e) D_b] B)[rqp][rqp] -- what a Jacobi preconditioner or a Chebyshev smoother
    needs.  The bases, derivative matrices, g, w (or None with lam == 0) and lam of helmholtz_hex; out holds nm0*nm1*nm2
    modes per element and may not overlap g, w or a table.  tabs: the three tensors of diag_tables(nq_d, basis_d, deriv_d),
    built here when None; when given, the bases and derivative matrices are not looked at.  float64 takes variant
    "auto", "wave" or "generic"; float32 the AUTO route.  A plain function: no autograd."""
    return _diag("diag_helmholtz_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2), g, w, lam, out, variant,
                 stream, tabs)


def diag_helmholtz_quad(nq, basis0, basis1, deriv0, deriv1, g, w, lam, out=None, variant="auto", stream=None, tabs=None):
    """The diagonal of helmholtz_quad's operator: g[e][c][j][i] with c = 0..2 for (00, 01, 11), w[e][j][i] or None with
    lam == 0; tabs: the two tensors of diag_tables, built here when None."""
    return _diag("diag_helmholtz_quad", nq, (basis0, basis1), (deriv0, deriv1), g, w, lam, out, variant, stream, tabs)


GEOM_OUTPUTS = ("df", "w", "g", "detj")


def _geom_call(what, nq, bases, derivs, qws, x, names, per, out, variant, stream):
    """The one call path of geom_* and geom_affine_*: sizes, dtypes and devices are checked here (before any library
    call), pointers, alignment and overlap in the C ABI.  names: the outputs asked for, a subset of the keys of `per`
    (name -> scalars per element, in the order of the C signature); out: None or a dict name -> flat tensor (a name that
    is asked for and missing is allocated); variant None: the call has none (the affine form).  Returns the dict of the
    outputs asked for."""
    xs = _input_parts(what, x, len(nq))
    inp = xs[0]
    nq, nmt, _ = _extents(what, nq)
    nelmt = _batch(what, inp, nmt, "x_a", "modes")
    names = tuple(names)
    for name in names:
        if name not in per:
            raise ValueError(f"{what}: unknown output {name!r}; the outputs are {tuple(per)}")
    if not names:
        raise capi.SumfactError(capi.SF_EINVAL, what)
    outs = dict(out or {})
    for name in outs:
        if name not in names:
            raise ValueError(f"{what}: out holds {name!r}, which is not asked for")
    for name in names:
        if outs.get(name) is None:
            outs[name] = torch.empty(nelmt * per[name], dtype=inp.dtype, device=inp.device)
    need_q = qws is not None and any(n in names for n in ("w", "g"))
    operands = [(f"basis{a}", b, (q - 1) * q, False) for a, (b, q) in enumerate(zip(bases, nq))]
    operands += _per_direction("deriv", derivs, lambda q: q * q, nq)
    if qws is not None:
        operands += [(f"qw{a}", t if need_q else None, int(q), not need_q) for a, (t, q) in enumerate(zip(qws, nq))]
    _check_operands(what, operands + [(name, outs[name], nelmt * per[name], False) for name in names], inp)
    f32 = inp.dtype == torch.float32
    dtype = torch.float32 if f32 else torch.float64
    fn, head = _entry(what, what, f32, variant)
    ptrs = [None if t is None else _dev_ptr(t, name, dtype) for name, t, _, _ in operands]
    ptrs += [_dev_ptr(t, f"x{a}", dtype) for a, t in enumerate(xs)]
    ptrs += [_dev_ptr(outs[name], name, dtype) if name in names else None for name in per]
    _launch(what, fn, inp, stream, (*head, *nq, nelmt, *ptrs))
    return {name: outs[name] for name in names}


def _geom(what, nq, bases, derivs, qws, x, outputs, out, variant, stream):
    d = len(nq)
    nqt = 1
    for q in nq:
        nqt *= int(q)
    per = {"df": d * d * nqt, "w": nqt, "g": d * (d + 1) // 2 * nqt, "detj": nqt}
    return _geom_call(what, nq, bases, derivs, qws, x, outputs, per, out, variant, stream)


def geom_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, qw0, qw1, qw2, x, outputs=GEOM_OUTPUTS, out=None,
             variant="auto", stream=None):
    """The geometric factors of isoparametric hexahedra from their modal coordinates, in one kernel on x's device.  x: a
    (3, nelmt * nm0*nm1*nm2) tensor with contiguous rows or a sequence of three flat tensors, coordinate a of every element
    in the layout of bwdtrans_hex's input, expanded in the bases of bwdtrans_hex; deriv_d as in helmholtz_hex; qw_d the
    one-dimensional quadrature weights (looked at only when "w" or "g" is asked for; may be None otherwise).  Returns a
    dict of flat tensors with the keys of `outputs`: "df" (nine planes per element, c = 3 a + b for d xi_b / d x_a: what
    physderiv_hex / iprodderiv_hex take), "w" (|det J| qw2[k] qw1[j] qw0[i]) and "g" (six planes, 00 01 02 11 12 22: what
    helmholtz_hex / diag_helmholtz_hex take), "detj" (the signed determinant).  out: a dict name -> flat tensor for the
    outputs the caller owns.  No output may overlap x or another output.  float64 takes variant "auto", "wave" or
    "generic"; float32 the AUTO route.  A plain function: no autograd."""
    return _geom("geom_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2), (qw0, qw1, qw2), x, outputs, out,
                 variant, stream)


def geom_quad(nq, basis0, basis1, deriv0, deriv1, qw0, qw1, x, outputs=GEOM_OUTPUTS, out=None, variant="auto", stream=None):
    """The geometric factors of isoparametric quadrilaterals: x holds two coordinates, "df" four planes (c = 2 a + b), "g"
    three (00 01 11), w = |det J| qw1[j] qw0[i]."""
    return _geom("geom_quad", nq, (basis0, basis1), (deriv0, deriv1), (qw0, qw1), x, outputs, out, variant, stream)


def _advect_planes(d, df, w):
    return lambda nelmt, nqt: [("df", df, nelmt * d * d * nqt, False), ("w", w, nelmt * nqt, False)]


def _advect(what, nq, bases, derivs, geometry, c, inp, out, variant, stream):
    """The one call path of advect_* and affine_advect_*: the number of fields, sizes, dtypes, devices and overlap are
    checked here (before any library call), pointers and alignment in the C ABI.  geometry(nelmt, nqt): the operands
    between the derivative matrices and c, as _check_operands takes them; one that is None and may be goes as NULL."""
    nq, nmt, nqt = _extents(what, nq)
    d = len(nq)
    if isinstance(inp, torch.Tensor):
        nf = inp.shape[0] if inp.dim() == 2 else 1
    else:
        inp = list(inp)
        nf = len(inp)
    if nf not in (1, d):
        raise capi.SumfactError(capi.SF_EINVAL, f"{what}: {nf} fields, not 1 or {d}")
    ins = _input_parts(what, inp, nf)
    first = ins[0]
    nelmt = _batch(what, first, nmt, "in_a", "modes")
    if isinstance(c, torch.Tensor) and c.numel() != d * nelmt * nqt:
        raise ValueError(f"{what}: c has {c.numel()} values, not {d} x {nelmt * nqt}")
    cs = _input_parts(what, c, d)
    ret, outs = _output_parts(what, out, nf, nelmt * nmt, first)
    operands = [(f"basis{a}", b, (q - 1) * q, False) for a, (b, q) in enumerate(zip(bases, nq))]
    operands += _per_direction("deriv", derivs, lambda q: q * q, nq)
    operands += geometry(nelmt, nqt)
    operands += [(f"c{j}", t, nelmt * nqt, False) for j, t in enumerate(cs)]
    _check_operands(what, operands + [(f"out{a}", t, nelmt * nmt, False) for a, t in enumerate(outs)], first)
    reads = [(name, t) for name, t, _, _ in operands if t is not None] + [(f"in{a}", t) for a, t in enumerate(ins)]
    _refuse_overlap(what, [(f"out{a}", t) for a, t in enumerate(outs)], reads)
    f32 = first.dtype == torch.float32
    dtype = torch.float32 if f32 else torch.float64
    fn, head = _entry(what, what.replace("affine_", "aff_"), f32, variant)
    ptrs = [None if t is None else _dev_ptr(t, name, dtype) for name, t, _, _ in operands]
    ptrs += [_dev_ptr(t, f"in{a}", dtype) for a, t in enumerate(ins)] + [None] * (d - nf)
    ptrs += [_dev_ptr(t, f"out{a}", dtype) for a, t in enumerate(outs)] + [None] * (d - nf)
    _launch(what, fn, first, stream, (*head, *nq, nelmt, nf, *ptrs))
    return ret


def advect_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, df, w, c, inp, out=None, variant="auto", stream=None):
    """The weak advection term (c . grad) u tested against the basis, in one kernel on inp's device: with u_a = B in_a and
    J[a][b] = D_b u_a, beta_b = sum_j c[j] df[3 j + b] and r_a = w (sum_b beta_b J[a][b]) per point, out[a] = B^T r_a.  The
    bases and derivative matrices of helmholtz_hex; df the nine planes of physderiv_hex / geom_hex, w the weight plane of
    mass_hex / geom_hex; c a (3, nelmt * nq0*nq1*nq2) tensor with contiguous rows or a sequence of three flat tensors, the
    advecting velocity at the quadrature points in the layout of bwdtrans_hex's output; inp a (nf, nelmt * nm0*nm1*nm2)
    tensor with contiguous rows or a sequence of nf flat tensors, nf = 1 (scalar transport; a flat tensor is one field) or
    3 (a vector field: one read of df, w, c for all three).  Returns a (nf, nelmt * nm0*nm1*nm2) tensor, rows aligned as
    physderiv_hex returns them; `out` may be such a tensor or a sequence of nf flat tensors (then returned as a tuple).
    No output may overlap an input or another output.  float64 takes variant "auto", "wave" or "generic"; float32 the AUTO
    route.  A plain function: no autograd."""
    return _advect("advect_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2), _advect_planes(3, df, w), c, inp,
                   out, variant, stream)


def advect_quad(nq, basis0, basis1, deriv0, deriv1, df, w, c, inp, out=None, variant="auto", stream=None):
    """The weak advection term in 2D: four planes of df (c = 2 a + b), two planes of c, nf = 1 or 2 fields."""
    return _advect("advect_quad", nq, (basis0, basis1), (deriv0, deriv1), _advect_planes(2, df, w), c, inp, out, variant,
                   stream)


def _advect_constants(nq, qws, dfe, je):
    d = len(nq)
    unweighted = je is None             # the quadrature weights are then never read and may be None as well
    return lambda nelmt, nqt: (
        [(f"qw{i}", t, int(q), unweighted) for i, (t, q) in enumerate(zip(qws, nq))]
        + [("dfe", dfe, nelmt * d * d, False), ("je", je, nelmt, True)])


def affine_advect_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, qw0, qw1, qw2, dfe, je, c, inp, out=None,
                      variant="auto", stream=None):
    """advect_hex on affine elements in one kernel: beta_b = sum_j c[j] dfe[e][3 j + b] and r_a = (je[e] qw2[k] (qw1[j]
    qw0[i])) (sum_b beta_b J[a][b]) per point, out[a] = B^T r_a.  qw_d the one-dimensional quadrature weights and je[e] =
    |det J| as in affine_iprodderiv_hex, dfe the nine constants per element of affine_physderiv_hex / geom_affine_hex
    (required).  je=None: no weight at all, je and qw_d are never read (qw_d may then be None too).  With je, bit for bit
    advect_hex on df planes filled with the constants and w = je * (qw2 * (qw1 * qw0)); without, advect_hex with w a plane
    of ones.  c, inp, out, nf and variants as advect_hex.  A plain function: no autograd."""
    return _advect("affine_advect_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2),
                   _advect_constants(nq, (qw0, qw1, qw2), dfe, je), c, inp, out, variant, stream)


def affine_advect_quad(nq, basis0, basis1, deriv0, deriv1, qw0, qw1, dfe, je, c, inp, out=None, variant="auto",
                       stream=None):
    """advect_quad on affine elements: four constants per element (c = 2 a + b), je[e] or None (then qw_d are never read),
    two planes of c, nf = 1 or 2 fields."""
    return _advect("affine_advect_quad", nq, (basis0, basis1), (deriv0, deriv1), _advect_constants(nq, (qw0, qw1), dfe, je),
                   c, inp, out, variant, stream)


VECGRAD_OUTPUTS = ("grad", "div", "curl")


def _vecgrad(what, nq, bases, derivs, df, inp, outputs, out, variant, stream):
    """The one call path of vecgrad_*: the outputs asked for, sizes, dtypes, devices and overlap are checked here (before
    any library call), pointers and alignment in the C ABI.  Returns the dict of the outputs asked for."""
    nq, nmt, nqt = _extents(what, nq)
    d = len(nq)
    ins = _input_parts(what, inp, d)
    first = ins[0]
    nelmt = _batch(what, first, nmt, "in_a", "modes")
    names = tuple(outputs)
    for name in names:
        if name not in VECGRAD_OUTPUTS:
            raise ValueError(f"{what}: unknown output {name!r}; the outputs are {VECGRAD_OUTPUTS}")
    if not names:
        raise capi.SumfactError(capi.SF_EINVAL, what)
    given = dict(out or {})
    for name in given:
        if name not in names:
            raise ValueError(f"{what}: out holds {name!r}, which is not asked for")
    ret, parts = {}, []                 # parts: (name, flat tensor, numel) in the order of the C signature
    for name, per in (("grad", d * d * nqt), ("div", nqt)):
        if name in names:
            t = given.get(name)
            ret[name] = torch.empty(nelmt * per, dtype=first.dtype, device=first.device) if t is None else t
            parts.append((name, ret[name], nelmt * per))
    ncurl = d * (d - 1) // 2
    if "curl" in names:
        if ncurl == 1:
            t = given.get("curl")
            ret["curl"] = torch.empty(nelmt * nqt, dtype=first.dtype, device=first.device) if t is None else t
            parts.append(("curl0", ret["curl"], nelmt * nqt))
        else:
            ret["curl"], rows = _output_parts(f"{what}: curl", given.get("curl"), ncurl, nelmt * nqt, first)
            parts += [(f"curl{n}", t, nelmt * nqt) for n, t in enumerate(rows)]
    operands = [(f"basis{a}", b, (q - 1) * q, False) for a, (b, q) in enumerate(zip(bases, nq))]
    operands += _per_direction("deriv", derivs, lambda q: q * q, nq)
    operands += [("df", df, nelmt * d * d * nqt, False)]
    _check_operands(what, operands + [(name, t, need, False) for name, t, need in parts], first)
    reads = [(name, t) for name, t, _, _ in operands] + [(f"in{a}", t) for a, t in enumerate(ins)]
    _refuse_overlap(what, [(name, t) for name, t, _ in parts], reads)
    f32 = first.dtype == torch.float32
    dtype = torch.float32 if f32 else torch.float64
    fn, head = _entry(what, what, f32, variant)
    ptrs = [_dev_ptr(t, name, dtype) for name, t, _, _ in operands]
    ptrs += [_dev_ptr(t, f"in{a}", dtype) for a, t in enumerate(ins)]
    by_name = {name: t for name, t, _ in parts}
    ptrs += [_dev_ptr(by_name[name], name, dtype) if name in by_name else None
             for name in ["grad", "div"] + [f"curl{n}" for n in range(ncurl)]]
    _launch(what, fn, first, stream, (*head, *nq, nelmt, *ptrs))
    return {name: ret[name] for name in names}


def vecgrad_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, df, inp, outputs=VECGRAD_OUTPUTS, out=None,
                variant="auto", stream=None):
    """The gradient, divergence and curl of a vector field at the quadrature points, in one kernel on inp's device: with
    u_a = B in_a and J[a][b] = D_b u_a, grad[a][j] = sum_b df[3 j + b] J[a][b] = d u_a / d x_j per point.  The bases and
    derivative matrices of helmholtz_hex; df the nine planes of physderiv_hex / geom_hex (required); inp a (3, nelmt *
    nm0*nm1*nm2) tensor with contiguous rows or a sequence of three flat tensors.  Returns a dict of tensors with the keys
    of `outputs`: "grad" (flat, nine planes per element in the layout of df, plane 3 a + j equal to output j of
    physderiv_hex on in_a bit for bit), "div" (flat, grad[0][0] + grad[1][1] + grad[2][2]) and "curl" (a (3, nelmt *
    nq0*nq1*nq2) tensor, rows aligned as advect_hex returns them: grad[2][1] - grad[1][2], grad[0][2] - grad[2][0],
    grad[1][0] - grad[0][1]); every plane in the layout of bwdtrans_hex's output.  out: a dict name -> tensor for the
    outputs the caller owns ("curl": such a (3, n) tensor or a sequence of three flat tensors, then returned as a tuple).
    No output may overlap an input or another output.  float64 takes variant "auto", "wave" or "generic"; float32 the
    AUTO route.  A plain function: no autograd."""
    return _vecgrad("vecgrad_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2), df, inp, outputs, out, variant,
                    stream)


def vecgrad_quad(nq, basis0, basis1, deriv0, deriv1, df, inp, outputs=VECGRAD_OUTPUTS, out=None, variant="auto",
                 stream=None):
    """vecgrad_hex in 2D: two fields, four planes of df and of "grad" (c = 2 a + j), "div" = grad[0][0] + grad[1][1],
    "curl" one flat plane, grad[1][0] - grad[0][1]."""
    return _vecgrad("vecgrad_quad", nq, (basis0, basis1), (deriv0, deriv1), df, inp, outputs, out, variant, stream)


def _geom_affine(what, nq, bases, derivs, x, stream):
    d = len(nq)
    per = {"dfe": d * d, "ge": d * (d + 1) // 2, "je": 1}
    got = _geom_call(what, nq, bases, derivs, None, x, tuple(per), per, None, None, stream)
    return got["dfe"], got["ge"], got["je"]


def geom_affine_hex(nq, basis0, basis1, basis2, deriv0, deriv1, deriv2, x, stream=None):
    """geom_hex for elements known to be affine: the same formulas at the point (0, 0, 0) of every element.  Returns
    (dfe, ge, je), the per-element constants of affine_physderiv_hex / affine_iprodderiv_hex (dfe[e][3 a + b]) and of
    affine_helmholtz_hex (ge[e][c] = je sum_x dfe dfe, je[e] = |det J|); dfe and je equal point 0 of geom_hex bit for bit.
    Any extents the "generic" route of geom_hex takes; float64 and float32.  A plain function: no autograd."""
    return _geom_affine("geom_affine_hex", nq, (basis0, basis1, basis2), (deriv0, deriv1, deriv2), x, stream)


def geom_affine_quad(nq, basis0, basis1, deriv0, deriv1, x, stream=None):
    """geom_affine_hex in 2D: dfe[e][2 a + b], ge[e][c] with c = 0..2 for (00, 01, 11), je[e]."""
    return _geom_affine("geom_affine_quad", nq, (basis0, basis1), (deriv0, deriv1), x, stream)


class GsMap:
    """What gs_setup returns: the local-to-global map `l2g` (int32, nlocal entries) and its inverted index `rows` (nglobal
    words) / `perm` (nlocal words), all on one device.  rows / perm are opaque: only the library reads them."""

    def __init__(self, l2g, rows, perm, nlocal, nglobal):
        self.l2g, self.rows, self.perm, self.nlocal, self.nglobal = l2g, rows, perm, nlocal, nglobal


def gs_setup(l2g, nglobal, stream=None):
    """Invert the local-to-global map once (blocking): l2g[i] is the global degree of freedom of local coefficient i, a
    negative entry a coefficient that belongs to none; every entry must be < nglobal (else SumfactError SF_EINVAL).
    Returns the GsMap that global_to_local, assemble and gs take."""
    nglobal = int(nglobal)
    if not (isinstance(l2g, torch.Tensor) and l2g.dtype == torch.int32):
        raise TypeError("gs_setup: l2g must be an int32 tensor")
    if nglobal < 0:
        raise ValueError("gs_setup: nglobal is negative")
    l2g = l2g.reshape(-1)
    nlocal = l2g.numel()
    rows = torch.zeros(nglobal, dtype=torch.int32, device=l2g.device)    # a map of no coefficients: rows of none
    perm = torch.empty(nlocal, dtype=torch.int32, device=l2g.device)
    with torch.cuda.device(l2g.device):
        rc = capi.lib().sf_gs_setup(nlocal, nglobal, _dev_ptr(l2g, "l2g", torch.int32), _dev_ptr(rows, "rows", torch.int32),
                                    _dev_ptr(perm, "perm", torch.int32), _stream(stream, l2g.device))
    capi.check(rc, "sf_gs_setup")
    return GsMap(l2g, rows, perm, nlocal, nglobal)


def _gs_map(what, gsmap):
    if not isinstance(gsmap, GsMap):
        raise TypeError(f"{what}: gsmap must come from gs_setup")


def _gs_values(what, gsmap, values, sign):
    """The checks of the gather-scatter calls before the library sees a pointer: `values` is (name, tensor, numel) of the
    float64 / float32 arrays, the first of which sets dtype and device; sign, if given, has nlocal values of that dtype.
    Returns (suffix of the symbol, dtype, pointer of sign or None)."""
    first = values[0][1]
    if not isinstance(first, torch.Tensor) or first.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"{what}: {values[0][0]} must be a float64 or float32 tensor")
    if first.device != gsmap.l2g.device:
        raise ValueError(f"{what}: {values[0][0]} is on {first.device}, the map is on {gsmap.l2g.device}")
    _check_operands(what, [(name, t, need, False) for name, t, need in values] + [("sign", sign, gsmap.nlocal, True)], first)
    return _sfx(first.dtype), first.dtype, None if sign is None else _dev_ptr(sign, "sign", first.dtype)


def global_to_local(gsmap, glob, sign=None, out=None, stream=None):
    """Q: out[i] = sign[i] * glob[l2g[i]], 0 where l2g[i] < 0 (Nektar++'s AssemblyMap::GlobalToLocal).  glob holds nglobal
    values, out and sign nlocal; sign None: all +1."""
    _gs_map("global_to_local", gsmap)
    if out is None and isinstance(glob, torch.Tensor):
        out = torch.empty(gsmap.nlocal, dtype=glob.dtype, device=glob.device)
    sfx, dtype, sp = _gs_values("global_to_local", gsmap, [("glob", glob, gsmap.nglobal), ("out", out, gsmap.nlocal)], sign)
    with torch.cuda.device(glob.device):
        rc = getattr(capi.lib(), "sf_global_to_local_" + sfx)(
            gsmap.nlocal, _dev_ptr(gsmap.l2g, "l2g", torch.int32), sp, _dev_ptr(glob, "glob", dtype),
            _dev_ptr(out, "out", dtype), _stream(stream, glob.device))
    capi.check(rc, "sf_global_to_local")
    return out


def assemble(gsmap, local, sign=None, out=None, stream=None):
    """Q^T: out[g] = sum of sign[i] * local[i] over the local coefficients of g, added in ascending i (Nektar++'s
    AssemblyMap::Assemble); 0 for a g with none.  No float atomics: bitwise reproducible.  Every out[g] is written."""
    _gs_map("assemble", gsmap)
    if out is None and isinstance(local, torch.Tensor):
        out = torch.empty(gsmap.nglobal, dtype=local.dtype, device=local.device)
    sfx, dtype, sp = _gs_values("assemble", gsmap, [("local", local, gsmap.nlocal), ("out", out, gsmap.nglobal)], sign)
    with torch.cuda.device(local.device):
        rc = getattr(capi.lib(), "sf_assemble_" + sfx)(
            gsmap.nglobal, _dev_ptr(gsmap.rows, "rows", torch.int32), _dev_ptr(gsmap.perm, "perm", torch.int32), sp,
            _dev_ptr(local, "local", dtype), _dev_ptr(out, "out", dtype), _stream(stream, local.device))
    capi.check(rc, "sf_assemble")
    return out


def gs(gsmap, local, sign=None, stream=None):
    """Q Q^T in place: local[i] <- sign[i] * sum_j sign[j] * local[j] over the coefficients that share l2g[i], the sum in
    assemble's order; coefficients with l2g[i] < 0 or alone on their degree of freedom stay as they are.  Returns local."""
    _gs_map("gs", gsmap)
    sfx, dtype, sp = _gs_values("gs", gsmap, [("local", local, gsmap.nlocal)], sign)
    with torch.cuda.device(local.device):
        rc = getattr(capi.lib(), "sf_gs_" + sfx)(
            gsmap.nglobal, _dev_ptr(gsmap.rows, "rows", torch.int32), _dev_ptr(gsmap.perm, "perm", torch.int32), sp,
            _dev_ptr(local, "local", dtype), _stream(stream, local.device))
    capi.check(rc, "sf_gs")
    return local


class _BwdTrans(torch.autograd.Function):
    """AUTO BwdTrans forward; its input gradient is IProductWRTBase of the output gradient (the exact transpose)."""

    @staticmethod
    def forward(ctx, inp, nq, *bases):
        ctx.nq, ctx.shape = nq, inp.shape
        ctx.save_for_backward(*bases)
        x = inp.contiguous()
        return bwdtrans_hex(nq, *bases, x) if len(nq) == 3 else bwdtrans_quad(nq, *bases, x)

    @staticmethod
    def backward(ctx, grad_out):
        bases, g = ctx.saved_tensors, grad_out.contiguous()
        gin = iproduct_hex(ctx.nq, *bases, g) if len(ctx.nq) == 3 else iproduct_quad(ctx.nq, *bases, g)
        return (gin.reshape(ctx.shape), None) + (None,) * len(bases)


def bwdtrans_autograd(nq, bases, inp):
    """BwdTrans (AUTO) with a backward pass: the gradient with respect to `inp` is iproduct_*(grad_out), enqueued on
    the current stream.  The bases are constants: a basis that requires grad is refused.  Returns the flat output."""
    nq, bases = tuple(int(x) for x in nq), tuple(bases)
    if len(nq) not in (2, 3) or len(bases) != len(nq):
        raise ValueError("bwdtrans_autograd: 2 or 3 extents, one basis per extent")
    if any(b.requires_grad for b in bases):
        raise ValueError("bwdtrans_autograd: the bases are constants; detach them (no gradient flows to a basis)")
    return _BwdTrans.apply(inp, nq, *bases)


class _PhysDeriv(torch.autograd.Function):
    """AUTO physderiv_* forward; its input gradient is iprodderiv_*(df, None, grad_out) (the exact transpose)."""

    @staticmethod
    def forward(ctx, inp, nq, df, *mats):
        ctx.nq, ctx.shape, ctx.has_df = nq, inp.shape, df is not None
        ctx.save_for_backward(*mats, *((df,) if df is not None else ()))
        x = inp.contiguous()
        return physderiv_hex(nq, *mats, df, x) if len(nq) == 3 else physderiv_quad(nq, *mats, df, x)

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        mats, df = saved[:2 * len(ctx.nq)], saved[-1] if ctx.has_df else None
        g = grad_out if grad_out.shape[1] <= 1 or grad_out.stride(1) == 1 else grad_out.contiguous()
        f = iprodderiv_hex if len(ctx.nq) == 3 else iprodderiv_quad
        return (f(ctx.nq, *mats, df, None, g).reshape(ctx.shape), None, None) + (None,) * len(mats)


def physderiv_autograd(nq, bases, derivs, df, inp):
    """physderiv_* (AUTO) with a backward pass: the gradient with respect to `inp` is iprodderiv_*(df, None, grad_out),
    enqueued on the current stream.  The bases, the derivative matrices and df (which may be None) are constants: one that
    requires grad is refused.  Returns the (d, n) output of physderiv_*."""
    nq, bases, derivs = tuple(int(x) for x in nq), tuple(bases), tuple(derivs)
    if len(nq) not in (2, 3) or len(bases) != len(nq) or len(derivs) != len(nq):
        raise ValueError("physderiv_autograd: 2 or 3 extents, one basis and one derivative matrix per extent")
    if any(t.requires_grad for t in bases + derivs + ((df,) if df is not None else ())):
        raise ValueError("physderiv_autograd: the bases, the derivative matrices and df are constants; detach them (no "
                         "gradient flows to them)")
    return _PhysDeriv.apply(inp, nq, df, *bases, *derivs)


class _AffinePhysDeriv(torch.autograd.Function):
    """AUTO affine_physderiv_* forward; its input gradient is affine_iprodderiv_*(dfe, je=None, grad_out) (the exact
    transpose)."""

    @staticmethod
    def forward(ctx, inp, nq, dfe, *mats):
        ctx.nq, ctx.shape = nq, inp.shape
        ctx.save_for_backward(*mats, dfe)
        x = inp.contiguous()
        return affine_physderiv_hex(nq, *mats, dfe, x) if len(nq) == 3 else affine_physderiv_quad(nq, *mats, dfe, x)

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        mats, dfe, d = saved[:-1], saved[-1], len(ctx.nq)
        g = grad_out if grad_out.shape[1] <= 1 or grad_out.stride(1) == 1 else grad_out.contiguous()
        f = affine_iprodderiv_hex if d == 3 else affine_iprodderiv_quad
        return (f(ctx.nq, *mats, *(None,) * d, dfe, None, g).reshape(ctx.shape), None, None) + (None,) * len(mats)


def affine_physderiv_autograd(nq, bases, derivs, dfe, inp):
    """affine_physderiv_* (AUTO) with a backward pass: the gradient with respect to `inp` is affine_iprodderiv_*(dfe,
    je=None, grad_out), enqueued on the current stream.  The bases, the derivative matrices and dfe are constants: one
    that requires grad is refused.  Returns the (d, n) output of affine_physderiv_*."""
    nq, bases, derivs = tuple(int(x) for x in nq), tuple(bases), tuple(derivs)
    if len(nq) not in (2, 3) or len(bases) != len(nq) or len(derivs) != len(nq):
        raise ValueError("affine_physderiv_autograd: 2 or 3 extents, one basis and one derivative matrix per extent")
    if not isinstance(dfe, torch.Tensor):
        raise TypeError("affine_physderiv_autograd: dfe must be a tensor")
    if any(t.requires_grad for t in bases + derivs + (dfe,)):
        raise ValueError("affine_physderiv_autograd: the bases, the derivative matrices and dfe are constants; detach "
                         "them (no gradient flows to them)")
    return _AffinePhysDeriv.apply(inp, nq, dfe, *bases, *derivs)


def _tensor_extents(what, ni, no, dim):
    ni, no = tuple(int(x) for x in ni), tuple(int(x) for x in no)
    if len(ni) != dim or len(no) != dim:
        raise ValueError(f"{what}: {dim} input and {dim} output extents")
    return ni, no


def _tensor_call(what, shape, ni, no, mats, inp, trans, out, variant, stream):
    dim = 3 if shape == "hex" else 2
    ni, no = _tensor_extents(what, ni, no, dim)
    if len(mats) != dim:
        raise ValueError(f"{what}: {dim} extents need {dim} matrices")
    if not isinstance(inp, torch.Tensor):
        raise TypeError(f"{what}: in must be a tensor")
    if inp.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"{what}: in must be float64 or float32")
    if min(ni + no) < 1:
        raise capi.SumfactError(capi.SF_EINVAL, what)
    nin, nout = 1, 1
    for a, b in zip(ni, no):
        nin, nout = nin * a, nout * b
    nelmt = _batch(what, inp, nin, "in", "input values")
    if out is None:
        out = torch.empty(nelmt * nout, dtype=inp.dtype, device=inp.device)
    operands = [(f"m{d}", m, a * b, False) for d, (m, a, b) in enumerate(zip(mats, ni, no))]
    operands += [("in", inp, nelmt * nin, False), ("out", out, nelmt * nout, False)]
    _check_operands(what, operands, inp)
    fn, head = _entry(what, f"tensor_{shape}", inp.dtype == torch.float32, variant, "all")
    _launch(what, fn, inp, stream, itertools.chain(head, ni, no, (int(bool(trans)), nelmt),
                                                   (_dev_ptr(t, name, inp.dtype) for name, t, _, _ in operands)))
    return out


def tensor_hex(ni, no, m0, m1, m2, x, trans=False, out=None, variant="auto", stream=None):
    """The tensor-product apply with independent input / output extents on x's device: out[e][k][j][i] = sum_rqp
    x[e][r][q][p] M0(p,i) M1(q,j) M2(r,k), M_d(a,b) = m_d[a*no_d + b] (trans false: m_d row-major ni_d x no_d) or
    m_d[b*ni_d + a] (trans true: row-major no_d x ni_d).  x holds ni0*ni1*ni2 values per element, out no0*no1*no2; out
    may not overlap x.  float64 and float32; variant "auto", "wave" (the compiled table) or "generic"."""
    return _tensor_call("tensor_hex", "hex", ni, no, (m0, m1, m2), x, trans, out, variant, stream)


def tensor_quad(ni, no, m0, m1, x, trans=False, out=None, variant="auto", stream=None):
    """tensor_hex in 2D: out[e][j][i] = sum_qp x[e][q][p] M0(p,i) M1(q,j)."""
    return _tensor_call("tensor_quad", "quad", ni, no, (m0, m1), x, trans, out, variant, stream)


def _tensor_spec_args(ni, no, trans, dtype):
    dim = len(tuple(ni))
    if dim not in (2, 3):
        raise ValueError("ni / no must hold 2 (quad) or 3 (hex) extents")
    ni, no = _tensor_extents("specialise_tensor", ni, no, dim)
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("dtype must be torch.float64 or torch.float32")
    pad = (1,) * (3 - dim)
    return (dim,) + ni + pad + no + pad + (int(bool(trans)), 8 if dtype == torch.float64 else 4)


def specialise_tensor(ni, no, trans=False, dtype=torch.float64, device=None):
    """Compile (once per process) and load (once per device) the wave kernel of the tensor shape ni -> no, `trans`, on
    `device` (default: the current device).  Returns SF_OK, or SF_ECOMPILE when the shape is refused (its slab exceeds the
    limit, it would spill, hiprtc is missing, or the current stream is capturing: nothing is compiled then): AUTO calls
    of tensor_hex / tensor_quad then keep the any-extent kernel.  The log is specialise_log()."""
    args = _tensor_spec_args(ni, no, trans, dtype)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        if torch.cuda.is_current_stream_capturing():
            return capi.SF_ECOMPILE
        rc = capi.lib().sf_specialise_tensor(*args)
    if rc not in (capi.SF_OK, capi.SF_ECOMPILE):
        capi.check(rc, "sf_specialise_tensor")
    return rc


def tensor_specialisation_state(ni, no, trans=False, dtype=torch.float64, device=None):
    """(state, launches) of the tensor specialisation on `device`: state 0 none, 1 ready, SF_ECOMPILE refused."""
    n = ctypes.c_uint64(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        rc = capi.lib().sf_tensor_specialisation_state(*_tensor_spec_args(ni, no, trans, dtype), ctypes.byref(n))
    if rc not in (0, 1, capi.SF_ECOMPILE):
        capi.check(rc, "sf_tensor_specialisation_state")
    return rc, n.value


class _Tensor(torch.autograd.Function):
    """AUTO tensor apply forward; its input gradient is the same call with trans flipped and ni / no swapped."""

    @staticmethod
    def forward(ctx, inp, ni, no, trans, *mats):
        ctx.ni, ctx.no, ctx.trans, ctx.shape = ni, no, trans, inp.shape
        ctx.save_for_backward(*mats)
        fn = tensor_hex if len(ni) == 3 else tensor_quad
        return fn(ni, no, *mats, inp.contiguous(), trans=trans)

    @staticmethod
    def backward(ctx, grad_out):
        mats = ctx.saved_tensors
        fn = tensor_hex if len(ctx.ni) == 3 else tensor_quad
        gin = fn(ctx.no, ctx.ni, *mats, grad_out.contiguous(), trans=not ctx.trans)
        return (gin.reshape(ctx.shape), None, None, None) + (None,) * len(mats)


def tensor_autograd(ni, no, mats, inp, trans=False):
    """tensor_hex / tensor_quad (AUTO) with a backward pass: the gradient with respect to `inp` is the transposed apply
    of grad_out, the same matrices with `trans` flipped and ni / no swapped.  The matrices are constants: one that requires
    grad is refused.  Returns the flat output."""
    ni, no, mats = tuple(int(x) for x in ni), tuple(int(x) for x in no), tuple(mats)
    if len(ni) not in (2, 3) or len(no) != len(ni) or len(mats) != len(ni):
        raise ValueError("tensor_autograd: 2 or 3 extents in and out, one matrix per extent")
    if any(m.requires_grad for m in mats):
        raise ValueError("tensor_autograd: the matrices are constants; detach them (no gradient flows to a matrix)")
    return _Tensor.apply(inp, ni, no, bool(trans), *mats)


def _spec_args(nq, dtype):
    nq = tuple(int(x) for x in nq)
    if len(nq) not in (2, 3):
        raise ValueError("nq must hold 2 (quad) or 3 (hex) extents")
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("dtype must be torch.float64 or torch.float32")
    return (len(nq),) + nq + (0,) * (3 - len(nq)) + (8 if dtype == torch.float64 else 4,)


def specialise(nq, dtype=torch.float64, device=None):
    """Compile (once per process) and load (once per device) the wave-per-chunk kernel for extents `nq` (2 or 3 of
    them) on `device` (default: the current device).  Returns SF_OK, or SF_ECOMPILE when the shape cannot be
    specialised (hiprtc missing, compile failed, it would spill): AUTO then keeps its usual route.  AUTO calls of
    bwdtrans_hex / bwdtrans_quad launch a ready specialisation for shapes the compiled tables miss."""
    args = _spec_args(nq, dtype)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        rc = capi.lib().sf_specialise(*args)
    if rc not in (capi.SF_OK, capi.SF_ECOMPILE):
        capi.check(rc, "sf_specialise")
    return rc


def specialisation_state(nq, dtype=torch.float64, device=None):
    """(state, launches) of the specialisation of `nq` on `device`: state 0 none, 1 ready, SF_ECOMPILE failed."""
    n = ctypes.c_uint64(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        rc = capi.lib().sf_specialisation_state(*_spec_args(nq, dtype), ctypes.byref(n))
    if rc not in (0, 1, capi.SF_ECOMPILE):
        capi.check(rc, "sf_specialisation_state")
    return rc, n.value


def specialise_log():
    """This thread's last specialise() log (compile number, seconds, instantiation, compiler remarks)."""
    return capi.lib().sf_last_specialise_log().decode()


def bwdtrans_specialised(nq, *bases, inp, out=None, stream=None):
    """Launch only the specialised kernel of `nq` (ready after specialise()); same layouts as bwdtrans_hex / _quad.
    Raises SumfactError SF_ENOTBUILT when it is not ready, SF_EALIGN unless inp / out are 16-byte aligned."""
    args = _spec_args(nq, inp.dtype)
    dim, ext = args[0], args[1:1 + len(nq)]
    if len(bases) != dim:
        raise ValueError(f"{dim} extents need {dim} bases")
    nmt, nqt = 1, 1
    for q in ext:
        nmt, nqt = nmt * (q - 1), nqt * q
    nelmt = inp.numel() // nmt
    if nelmt * nmt != inp.numel():
        raise ValueError("in.numel() is not a multiple of the modes per element")
    if out is None:
        out = torch.empty(nelmt * nqt, dtype=inp.dtype, device=inp.device)
    _check_operands("bwdtrans_specialised", [(f"basis{d}", b, (q - 1) * q, False) for d, (b, q) in enumerate(zip(bases, ext))]
                    + [("out", out, nelmt * nqt, False)], inp)
    ptrs = [_dev_ptr(b, f"basis{d}", inp.dtype) for d, b in enumerate(bases)] + [None] * (3 - dim)
    with torch.cuda.device(inp.device):
        rc = capi.lib().sf_bwdtrans_specialised(*args, nelmt, *ptrs, _dev_ptr(inp, "in", inp.dtype),
                                                _dev_ptr(out, "out", inp.dtype), _stream(stream, inp.device))
    capi.check(rc, "sf_bwdtrans_specialised")
    return out


def interleave64(src, nelmt, n, inverse=False, stream=None):
    """[e][n] -> [(e/64)][n][e%64] (padded to whole groups of 64 elements), or back."""
    padded = (nelmt + 63) // 64 * 64
    dst = torch.zeros((nelmt if inverse else padded) * n, dtype=torch.float64, device=src.device)
    with torch.cuda.device(src.device):
        capi.check(capi.lib().sf_interleave64_f64(_dev_ptr(src, "src"), _dev_ptr(dst, "dst"), nelmt,
                                                  n, 1 if inverse else 0, _stream(stream, src.device)),
                   "sf_interleave64_f64")
    return dst


def bwdtrans_hex_interleaved(nq, basis0, basis1, basis2, in_il, nelmt, stream=None):
    """Thread-per-element kernel on the wave-64 interleaved layout (the corrected `_Coa`,
    benchmark05/benchmark05.cc:104-201).  Returns out_il (interleaved)."""
    nq0, nq1, nq2 = (int(x) for x in nq)
    padded = (nelmt + 63) // 64 * 64
    out = torch.empty(padded * nq0 * nq1 * nq2, dtype=torch.float64, device=in_il.device)
    wsp = torch.empty(padded * ((nq1 - 1) * (nq2 - 1) + (nq2 - 1)), dtype=torch.float64,
                      device=in_il.device)
    with torch.cuda.device(in_il.device):
        rc = capi.lib().sf_bwdtrans_hex_f64_interleaved(
            nq0, nq1, nq2, nelmt, _dev_ptr(basis0, "basis0"), _dev_ptr(basis1, "basis1"),
            _dev_ptr(basis2, "basis2"), _dev_ptr(in_il, "in_il"), _dev_ptr(wsp, "wsp"),
            _dev_ptr(out, "out_il"), _stream(stream, in_il.device))
    capi.check(rc, "sf_bwdtrans_hex_f64_interleaved")
    return out


def sumsq(x, stream=None):
    """sum x^2 (blocking; deterministic) -- the reference's thrust::transform_reduce."""
    res = ctypes.c_double(0.0)
    with torch.cuda.device(x.device):
        if x.dtype == torch.float32:
            rc = capi.lib().sf_sumsq_f32(_dev_ptr(x, "x", torch.float32), x.numel(), ctypes.byref(res),
                                         _stream(stream, x.device))
        else:
            rc = capi.lib().sf_sumsq_f64(_dev_ptr(x, "x"), x.numel(), ctypes.byref(res),
                                         _stream(stream, x.device))
    capi.check(rc, "sf_sumsq")
    return res.value


def _filled(n, device, call, what, dtype=torch.float64):
    x = torch.empty(n, dtype=dtype, device=device)
    with torch.cuda.device(x.device):
        capi.check(call(ctypes.c_void_p(x.data_ptr())), what)
    return x


def _sfx(dtype):
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("dtype must be torch.float64 or torch.float32")
    return "f32" if dtype == torch.float32 else "f64"


def fill_sincos(nelmt, nm_tot, device="cuda", stream=None, dtype=torch.float64):
    """in[e][f] = sin((T)(f+1)) (benchmark05/benchmark05.cc:1206-1207), generated on the device."""
    st, fn = _stream(stream, device), getattr(capi.lib(), "sf_fill_sincos_" + _sfx(dtype))
    return _filled(nelmt * nm_tot, device, lambda p: fn(p, nelmt, nm_tot, st), "sf_fill_sincos",
                   dtype)


def fill_basis(nm, nq, device="cuda", stream=None, dtype=torch.float64):
    """basis[x] = cos((T)x) (benchmark05/benchmark05.cc:1220)."""
    st, fn = _stream(stream, device), getattr(capi.lib(), "sf_fill_basis_" + _sfx(dtype))
    return _filled(nm * nq, device, lambda p: fn(p, nm, nq, st), "sf_fill_basis", dtype)


def fill_random(n, seed, first_idx=0, device="cuda", stream=None, dtype=torch.float64):
    """Seeded per-value-distinct U[-1,1) data; bit-identical to oracle.fill_random (rounded to
    float for dtype=float32)."""
    st, fn = _stream(stream, device), getattr(capi.lib(), "sf_fill_random_" + _sfx(dtype))
    return _filled(n, device, lambda p: fn(p, n, seed, first_idx, st), "sf_fill_random", dtype)


def fill_l2norm(n, device="cuda", stream=None):
    """x[i] = i%13 + (0.2 + 1e-5*(i%100191)) (benchmark01/benchmark01.cc:178)."""
    st = _stream(stream, device)
    return _filled(n, device, lambda p: capi.lib().sf_fill_l2norm_f64(p, n, st),
                   "sf_fill_l2norm_f64")


def stream_copy(src, dst, stream=None):
    with torch.cuda.device(src.device):
        capi.check(capi.lib().sf_stream_copy_f64(_dev_ptr(src, "src"), _dev_ptr(dst, "dst"),
                                                 src.numel(), _stream(stream, src.device)),
                   "sf_stream_copy_f64")
    return dst


def fill_vecadd(n, device="cuda", stream=None):
    """benchmark02 data (benchmark02/benchmark02.cc:84-85) -> (x, y)."""
    x = torch.empty(n, dtype=torch.float64, device=device)
    y = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(x.device):
        capi.check(capi.lib().sf_fill_vecadd_f64(_dev_ptr(x, "x"), _dev_ptr(y, "y"), n,
                                                 _stream(stream, x.device)), "sf_fill_vecadd_f64")
    return x, y


def vector_add(x, y, stream=None):
    """x += y in place (benchmark02's operation)."""
    with torch.cuda.device(x.device):
        capi.check(capi.lib().sf_vector_add_f64(_dev_ptr(x, "x"), _dev_ptr(y, "y"), x.numel(),
                                                _stream(stream, x.device)), "sf_vector_add_f64")
    return x


def fill_matvec(m, n, device="cuda", stream=None):
    """benchmark03 data -> (A row-major m*n, x)."""
    a = torch.empty(m * n, dtype=torch.float64, device=device)
    x = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(a.device):
        capi.check(capi.lib().sf_fill_matvec_f64(_dev_ptr(a, "A"), _dev_ptr(x, "x"), m, n,
                                                 _stream(stream, a.device)), "sf_fill_matvec_f64")
    return a, x


def matvec(m, n, a, x, y=None, stream=None):
    """y = A x (benchmark03's operation)."""
    if y is None:
        y = torch.empty(m, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        capi.check(capi.lib().sf_matvec_f64(m, n, _dev_ptr(a, "A"), _dev_ptr(x, "x"),
                                            _dev_ptr(y, "y"), _stream(stream, a.device)), "sf_matvec_f64")
    return y


def device_info():
    cu, wave = ctypes.c_int(0), ctypes.c_int(0)
    name = ctypes.create_string_buffer(256)
    capi.check(capi.lib().sf_device_info(ctypes.byref(cu), ctypes.byref(wave), name, 256),
               "sf_device_info")
    return {"num_cu": cu.value, "wave_size": wave.value, "name": name.value.decode()}
