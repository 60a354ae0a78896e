"""ctypes binding of include/sumfact.h (the C ABI of lib/libsumfact.so).

This is the same binding a maintainer of the reference would write if the harness were driven from
Python; INTEGRATION.md shows the C++ call-site form.  Fails loudly when the library is missing --
there is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsumfact.so")

SF_OK, SF_EINVAL, SF_EALIGN, SF_ENOTBUILT, SF_ENOMEM, SF_ECOMPILE = 0, -1, -2, -3, -4, -5

# every symbol include/sumfact.h declares: name -> (restype, argtypes)
_vp, _sz, _u, _u64, _i = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint64,
                          ctypes.c_int)
SYMBOLS = {
    "sf_version": (_i, []),
    "sf_error_string": (ctypes.c_char_p, [_i]),
    "sf_variant_name": (ctypes.c_char_p, [_i]),
    "sf_sumsq_f64": (_i, [_vp, _sz, ctypes.POINTER(ctypes.c_double), _vp]),
    "sf_sumsq_f64_async": (_i, [_vp, _sz, _vp, _vp]),
    "sf_fill_sincos_f64": (_i, [_vp, _sz, _sz, _vp]),
    "sf_fill_basis_f64": (_i, [_vp, _sz, _sz, _vp]),
    "sf_fill_random_f64": (_i, [_vp, _sz, _u64, _u64, _vp]),
    "sf_fill_l2norm_f64": (_i, [_vp, _sz, _vp]),
    "sf_stream_copy_f64": (_i, [_vp, _vp, _sz, _vp]),
    "sf_bwdtrans_hex_f64_interleaved": (_i, [_u, _u, _u, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sf_interleave64_f64": (_i, [_vp, _vp, _sz, _sz, _i, _vp]),
    "sf_bwdtrans_hex_f64_mfma4": (_i, [_i, _u, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sf_sumsq_f32": (_i, [_vp, _sz, ctypes.POINTER(ctypes.c_double), _vp]),
    "sf_fill_sincos_f32": (_i, [_vp, _sz, _sz, _vp]),
    "sf_fill_basis_f32": (_i, [_vp, _sz, _sz, _vp]),
    "sf_fill_random_f32": (_i, [_vp, _sz, _u64, _u64, _vp]),
    "sf_vector_add_f64": (_i, [_vp, _vp, _sz, _vp]),
    "sf_fill_vecadd_f64": (_i, [_vp, _vp, _sz, _vp]),
    "sf_matvec_f64": (_i, [_u, _u, _vp, _vp, _vp, _vp]),
    "sf_fill_matvec_f64": (_i, [_vp, _vp, _u, _u, _vp]),
    "sf_set_launch_hint": (_i, [_u, _u]),
    "sf_device_info": (_i, [ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.c_char_p, _sz]),
    "sf_specialise": (_i, [_i, _u, _u, _u, _i]),
    "sf_specialisation_state": (_i, [_i, _u, _u, _u, _i, ctypes.POINTER(_u64)]),
    "sf_bwdtrans_specialised": (_i, [_i, _u, _u, _u, _i, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sf_last_specialise_log": (ctypes.c_char_p, []),
    "sf_shutdown": (_i, []),
    "sf_diag_tables_f64": (_i, [_u, _vp, _vp, _vp, _vp]),
    "sf_diag_tables_f32": (_i, [_u, _vp, _vp, _vp, _vp]),
    "sf_gs_setup": (_i, [_sz, _sz, _vp, _vp, _vp, _vp]),
}
for _sfx in ("f64", "f32"):     # the gather-scatter apply calls: count, index arrays, sign, values, stream
    SYMBOLS[f"sf_global_to_local_{_sfx}"] = (_i, [_sz, _vp, _vp, _vp, _vp, _vp])
    SYMBOLS[f"sf_assemble_{_sfx}"] = (_i, [_sz, _vp, _vp, _vp, _vp, _vp, _vp])
    SYMBOLS[f"sf_gs_{_sfx}"] = (_i, [_sz, _vp, _vp, _vp, _vp, _vp])


def _operator_symbols():
    """sf_<stem>_{hex,quad}_{f64,f64_variant,f32} of the ten operator families: [variant,] the extents, nelmt, the pointer
    operands in front of `in` (so many per direction, so many per call), [lambda,] in (or one input per direction, or none:
    diag_helmholtz reads only its operands), [BwdTrans _variant: wsp,] out (or one output per direction), stream."""
    rows = {"bwdtrans": (1, 0, False, False, 1), "iproduct": (1, 0, False, False, 1),
            "mass": (1, 1, False, False, 1), "helmholtz": (2, 2, True, False, 1),
            "affine_helmholtz": (3, 2, True, False, 1), "physderiv": (2, 1, False, True, 1),
            "iprodderiv": (2, 2, False, False, "per direction"), "diag_helmholtz": (1, 2, True, False, 0),
            "aff_physderiv": (2, 1, False, True, 1), "aff_iprodderiv": (3, 2, False, False, "per direction")}
    for stem, (per_direction, per_call, has_lambda, out_per_direction, inputs) in rows.items():
        for shape, dim in (("hex", 3), ("quad", 2)):
            ins = [_vp] * (dim if inputs == "per direction" else inputs)
            outs = [_vp] * (dim if out_per_direction else 1)
            tail = [_vp] * (per_direction * dim + per_call) + ([ctypes.c_double] if has_lambda else []) + ins + outs + [_vp]
            for sfx in ("f64", "f64_variant", "f32"):
                head = [_i] if sfx == "f64_variant" else []
                wsp = [_vp] if (stem, sfx) == ("bwdtrans", "f64_variant") else []
                yield f"sf_{stem}_{shape}_{sfx}", (_i, head + [_u] * dim + [_sz] + tail + wsp)


SYMBOLS.update(_operator_symbols())


def _geom_symbols():
    """sf_geom_{hex,quad}_{f64,f64_variant,f32}: [variant,] the extents, nelmt, basis / deriv / qw per direction, x_a per
    direction, df, w, g, detj, stream; sf_geom_affine_{hex,quad}_{f64,f32}: the same without variant and qw, with dfe, ge,
    je."""
    for shape, dim in (("hex", 3), ("quad", 2)):
        for sfx in ("f64", "f64_variant", "f32"):
            head = [_i] if sfx == "f64_variant" else []
            yield f"sf_geom_{shape}_{sfx}", (_i, head + [_u] * dim + [_sz] + [_vp] * (4 * dim + 4) + [_vp])
        for sfx in ("f64", "f32"):
            yield f"sf_geom_affine_{shape}_{sfx}", (_i, [_u] * dim + [_sz] + [_vp] * (3 * dim + 3) + [_vp])


SYMBOLS.update(_geom_symbols())


def _advect_symbols():
    """sf_advect_{hex,quad}_{f64,f64_variant,f32}: [variant,] the extents, nelmt, nf, basis / deriv per direction, df, w,
    c_j per direction, in_a and out_a per direction, stream."""
    for shape, dim in (("hex", 3), ("quad", 2)):
        for sfx in ("f64", "f64_variant", "f32"):
            head = [_i] if sfx == "f64_variant" else []
            yield f"sf_advect_{shape}_{sfx}", (_i, head + [_u] * dim + [_sz, _u] + [_vp] * (5 * dim + 2) + [_vp])


SYMBOLS.update(_advect_symbols())


def _affine_advect_symbols():
    """sf_aff_advect_{hex,quad}_{f64,f64_variant,f32}: [variant,] the extents, nelmt, nf, basis / deriv / qw per direction,
    dfe, je, c_j per direction, in_a and out_a per direction, stream."""
    for shape, dim in (("hex", 3), ("quad", 2)):
        for sfx in ("f64", "f64_variant", "f32"):
            head = [_i] if sfx == "f64_variant" else []
            yield f"sf_aff_advect_{shape}_{sfx}", (_i, head + [_u] * dim + [_sz, _u] + [_vp] * (6 * dim + 2) + [_vp])


SYMBOLS.update(_affine_advect_symbols())


def _vecgrad_symbols():
    """sf_vecgrad_{hex,quad}_{f64,f64_variant,f32}: [variant,] the extents, nelmt, basis / deriv per direction, df, in_a per
    direction, grad, div, the d(d-1)/2 planes of the curl, stream."""
    for shape, dim in (("hex", 3), ("quad", 2)):
        for sfx in ("f64", "f64_variant", "f32"):
            head = [_i] if sfx == "f64_variant" else []
            ptrs = 3 * dim + 1 + 2 + dim * (dim - 1) // 2
            yield f"sf_vecgrad_{shape}_{sfx}", (_i, head + [_u] * dim + [_sz] + [_vp] * ptrs + [_vp])


SYMBOLS.update(_vecgrad_symbols())


def _tensor_symbols():
    """sf_tensor_{hex,quad}_{f64,f64_variant,f32,f32_variant}: [variant,] the input extents, the output extents, trans,
    nelmt, one matrix per direction, in, out, stream; sf_specialise_tensor / sf_tensor_specialisation_state: dim, three
    input and three output extents, trans, scalar_bytes[, launches]."""
    for shape, dim in (("hex", 3), ("quad", 2)):
        for sfx in ("f64", "f64_variant", "f32", "f32_variant"):
            head = [_i] if sfx.endswith("_variant") else []
            yield f"sf_tensor_{shape}_{sfx}", (_i, head + [_u] * (2 * dim) + [_i, _sz] + [_vp] * (dim + 2) + [_vp])
    yield "sf_specialise_tensor", (_i, [_i] + [_u] * 6 + [_i, _i])
    yield "sf_tensor_specialisation_state", (_i, [_i] + [_u] * 6 + [_i, _i, ctypes.POINTER(_u64)])


SYMBOLS.update(_tensor_symbols())

_lib = None


class SumfactError(RuntimeError):
    def __init__(self, rc, what):
        self.rc = rc
        msg = lib().sf_error_string(rc).decode() if _lib is not None else str(rc)
        super().__init__(f"{what}: rc={rc} ({msg})")


def lib():
    """Load libsumfact.so (once).  Raises if it has not been built: no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(make -C gpu-benchmarking_amd).  There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the export is missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != SF_OK:
        raise SumfactError(rc, what)
