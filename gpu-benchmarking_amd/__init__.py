"""gpu_benchmarking_amd -- MI355X-native BwdTrans sum-factorisation hot path.

The directory is named ``gpu-benchmarking_amd`` (not importable by name); load it with
``__graft_entry__.load_package()`` which registers it as ``gpu_benchmarking_amd``.

Layout
  csrc/   HIP kernels (gfx950) + the C ABI of lib/libsumfact.so (include/sumfact.h)
  host/   C++ drivers benchmark01/04/05 with the reference's run_test<T> signature, CLI and log grammar
  tools/  sf_tune (variant sweep), run.sh-style sweeps
  capi.py / bwdtrans.py / logfmt.py / shard.py : Python plumbing over the C ABI (tests, bench.py)

There is NO CPU fallback here: every compute entry point goes through libsumfact.so and raises if
it is missing.
"""
from . import capi, logfmt, shard  # noqa: F401
from .bwdtrans import (  # noqa: F401
    bwdtrans_hex, bwdtrans_hex_mfma4, bwdtrans_quad, sumsq, fill_sincos, fill_basis, fill_random, fill_l2norm,
    stream_copy, device_info, interleave64, bwdtrans_hex_interleaved, fill_vecadd, vector_add, fill_matvec, matvec, hex_wsp_doubles, quad_wsp_doubles, VARIANTS,
    specialise, specialisation_state, specialise_log, bwdtrans_specialised,
    iproduct_hex, iproduct_quad, bwdtrans_autograd, mass_hex, mass_quad,
    helmholtz_hex, helmholtz_quad, affine_helmholtz_hex, affine_helmholtz_quad,
    physderiv_hex, physderiv_quad,
    iprodderiv_hex, iprodderiv_quad, physderiv_autograd,
    affine_physderiv_hex, affine_physderiv_quad, affine_iprodderiv_hex, affine_iprodderiv_quad,
    affine_physderiv_autograd,
    diag_tables, diag_helmholtz_hex, diag_helmholtz_quad,
    GsMap, gs_setup, global_to_local, assemble, gs,
    geom_hex, geom_quad, geom_affine_hex, geom_affine_quad, GEOM_OUTPUTS,
    advect_hex, advect_quad, affine_advect_hex, affine_advect_quad,
    vecgrad_hex, vecgrad_quad, VECGRAD_OUTPUTS,
    tensor_hex, tensor_quad, specialise_tensor, tensor_specialisation_state, tensor_autograd,
)
