"""GPU tests of the plain entry points of the C ABI (include/sumfact.h): sf_<stem>_{hex,quad}_f64 of all 16 stems, the ones
a C or C++ caller is told to use (examples/consumer.c).  The Python layer sends float64 to _f64_variant
and float32 to _f32 (bwdtrans._entry), so no other GPU test passes data through them; tests/test_cabi_cpu.py pins their
return codes, which a swap of two operands of one type does not change.

What is asserted: the plain entry point gives, bit for bit and for every output array, what _f64_variant gives with
SF_VARIANT_AUTO -- which is what the Python API returns for variant="auto".  Both calls take the same route and the
kernels are deterministic: no tolerance is involved.  sf_tensor_* is covered in float32 as well (_f32 against
_f32_variant(AUTO)).

Operands: every operand is present, the optional ones too (w, df, je, qw_d, the curl planes; nf = d fields for the two
advection families), each filled by sf.fill_random with a seed of its own, so that no two pointer arguments hold equal
data and an operand in another's slot changes the result.  The values need no meaning (the Jacobians of sf_geom_* are
whatever random coordinates give): bits are compared, NaN included.

Extents, nelmt = 3, the smallest at which every slot still differs from its neighbours:
  aniso  (3, 4, 5) / (3, 4), sf_tensor_* ni = (2, 3, 4) -> no = (3, 4, 5) and their 2D prefixes: every per-direction
         operand has a size of its own (the any-extent route)
  iso    nq = 4 (sf_tensor_*: 3 -> 4) on freshly allocated, hence 16-byte aligned, tensors: the wave route

Mechanism: the public function is called once as it is and once with bwdtrans._entry replaced, so that float64 with
"auto" resolves to sf_<stem>_<shape>_f64 with no leading variant argument; the substitute records the symbol when it is
called, and the test asserts that it was.  Two stems do not fit and are called through capi.lib() directly:
  bwdtrans     the variant form alone takes `wsp`
  geom_affine  has no variant form.  It is compared with sf_geom_* on the same coordinates: dfe[e][c] and je[e] are
               df[e][c][0][0][0] and |detj[e][0][0][0]| bit for bit, which include/sumfact.h promises for any coordinates.
               For ge the header promises no such equality (g of sf_geom_* carries the quadrature weights), so the
               sf_geom_* call is given unit weights: then w = |det| * (1 * (1 * 1)) = je exactly, and step 7, one text
               for both kernels with every FMA named (csrc/geom_point.h), makes g[e][c][0][0][0] the bits of ge[e][c].
"""
import ctypes

import pytest

from fused_families import F32, F64, sf, torch_mod  # noqa: F401
from multifield_common import leaves, same_bits

pytestmark = pytest.mark.gpu

NELMT = 3
EXTENTS = {"aniso": ((2, 3, 4), (3, 4, 5)), "iso": ((3, 3, 3), (4, 4, 4))}     # (sf_tensor_* ni, nq = sf_tensor_* no)
SHAPES = {"hex": 3, "quad": 2}


class Fill:
    """Flat device tensors from sf.fill_random, every one freshly allocated and with a seed of its own."""

    def __init__(self, sf, torch_mod, dtype_name):
        self.sf, self.dtype, self.seed = sf, getattr(torch_mod, dtype_name), 0

    def __call__(self, n):
        self.seed += 1
        return self.sf.fill_random(n, 7000 + self.seed, dtype=self.dtype)

    def each(self, nq, numel):
        return [self(numel(q)) for q in nq]

    def matrices(self, nq):
        """basis_d, deriv_d, qw_d."""
        return self.each(nq, lambda q: (q - 1) * q), self.each(nq, lambda q: q * q), self.each(nq, lambda q: q)


def prod(v):
    n = 1
    for x in v:
        n *= x
    return n


# ---- one function per stem: (sf, mk, nq, ni) -> a function of no argument that calls the public API on fixed operands ----
def iproduct(sf, mk, nq, ni):
    b, _, _ = mk.matrices(nq)
    inp = mk(NELMT * prod(nq))
    return lambda: pick(sf, "iproduct", nq)(nq, *b, inp)


def mass(sf, mk, nq, ni):
    b, _, _ = mk.matrices(nq)
    w, inp = mk(NELMT * prod(nq)), mk(NELMT * prod(ni))
    return lambda: pick(sf, "mass", nq)(nq, *b, w, inp)


def helmholtz(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    ncomp = len(nq) * (len(nq) + 1) // 2
    g, w, inp = mk(NELMT * ncomp * prod(nq)), mk(NELMT * prod(nq)), mk(NELMT * prod(ni))
    return lambda: pick(sf, "helmholtz", nq)(nq, *b, *d, g, w, 0.75, inp)


def affine_helmholtz(sf, mk, nq, ni):
    b, d, q = mk.matrices(nq)
    ge, je, inp = mk(NELMT * len(nq) * (len(nq) + 1) // 2), mk(NELMT), mk(NELMT * prod(ni))
    return lambda: pick(sf, "affine_helmholtz", nq)(nq, *b, *d, *q, ge, je, 0.75, inp)


def physderiv(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    df, inp = mk(NELMT * len(nq) ** 2 * prod(nq)), mk(NELMT * prod(ni))
    return lambda: pick(sf, "physderiv", nq)(nq, *b, *d, df, inp)


def iprodderiv(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    df, w = mk(NELMT * len(nq) ** 2 * prod(nq)), mk(NELMT * prod(nq))
    ins = [mk(NELMT * prod(nq)) for _ in nq]
    return lambda: pick(sf, "iprodderiv", nq)(nq, *b, *d, df, w, ins)


def aff_physderiv(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    dfe, inp = mk(NELMT * len(nq) ** 2), mk(NELMT * prod(ni))
    return lambda: pick(sf, "affine_physderiv", nq)(nq, *b, *d, dfe, inp)


def aff_iprodderiv(sf, mk, nq, ni):
    b, d, q = mk.matrices(nq)
    dfe, je = mk(NELMT * len(nq) ** 2), mk(NELMT)
    ins = [mk(NELMT * prod(nq)) for _ in nq]
    return lambda: pick(sf, "affine_iprodderiv", nq)(nq, *b, *d, *q, dfe, je, ins)


def diag_helmholtz(sf, mk, nq, ni):
    """The tables are the per-direction operands of the C call; with them given the API looks at no basis or deriv."""
    tabs = mk.each(nq, lambda q: 3 * (q - 1) * q)
    ncomp = len(nq) * (len(nq) + 1) // 2
    g, w = mk(NELMT * ncomp * prod(nq)), mk(NELMT * prod(nq))
    none = (None,) * (2 * len(nq))
    return lambda: pick(sf, "diag_helmholtz", nq)(nq, *none, g, w, 0.75, tabs=tabs)


def geom(sf, mk, nq, ni):
    b, d, q = mk.matrices(nq)
    xs = [mk(NELMT * prod(ni)) for _ in nq]
    return lambda: pick(sf, "geom", nq)(nq, *b, *d, *q, xs)


def advect(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    df, w = mk(NELMT * len(nq) ** 2 * prod(nq)), mk(NELMT * prod(nq))
    cs, ins = [mk(NELMT * prod(nq)) for _ in nq], [mk(NELMT * prod(ni)) for _ in nq]
    return lambda: pick(sf, "advect", nq)(nq, *b, *d, df, w, cs, ins)


def aff_advect(sf, mk, nq, ni):
    b, d, q = mk.matrices(nq)
    dfe, je = mk(NELMT * len(nq) ** 2), mk(NELMT)
    cs, ins = [mk(NELMT * prod(nq)) for _ in nq], [mk(NELMT * prod(ni)) for _ in nq]
    return lambda: pick(sf, "affine_advect", nq)(nq, *b, *d, *q, dfe, je, cs, ins)


def vecgrad(sf, mk, nq, ni):
    b, d, _ = mk.matrices(nq)
    df, ins = mk(NELMT * len(nq) ** 2 * prod(nq)), [mk(NELMT * prod(ni)) for _ in nq]
    return lambda: pick(sf, "vecgrad", nq)(nq, *b, *d, df, ins)


def tensor(sf, mk, no, ni):
    ms = [mk(a * b) for a, b in zip(ni, no)]
    x = mk(NELMT * prod(ni))
    return lambda: pick(sf, "tensor", no)(ni, no, *ms, x)


PATCHED = (iproduct, mass, helmholtz, affine_helmholtz, physderiv, iprodderiv, aff_physderiv, aff_iprodderiv, diag_helmholtz,
           geom, advect, aff_advect, vecgrad, tensor)


def pick(sf, name, nq):
    return getattr(sf, f"{name}_{'hex' if len(nq) == 3 else 'quad'}")


def extents(shape, which):
    """(nq, the modes per direction: nq - 1, which is also sf_tensor_*'s ni)."""
    ni, nq = EXTENTS[which]
    return nq[:SHAPES[shape]], ni[:SHAPES[shape]]


def plain_entry(sf, called):
    """bwdtrans._entry with the AUTO call of a dtype that has a variant form sent to the plain symbol instead, which takes
    no leading variant; `called` gets the symbol's name whenever it is called."""
    real = sf.bwdtrans._entry

    def entry(what, stem, f32, variant, f32_takes="auto"):
        has_variant_form = not f32 or f32_takes == "all"
        if variant is None or not has_variant_form or sf.bwdtrans._variant(variant) != sf.VARIANTS["auto"]:
            return real(what, stem, f32, variant, f32_takes)
        name = f"sf_{stem}_{'f32' if f32 else 'f64'}"
        fn = getattr(sf.capi.lib(), name)

        def recorded(*args):
            called.append(name)
            return fn(*args)

        return recorded, ()

    return entry


def written(torch_mod, got):
    """Every output array holds something: two calls that wrote nothing would agree as well."""
    return all(bool((t != 0).any()) for t in leaves(got))


def through_both(sf, torch_mod, monkeypatch, make, shape, which, dtype_name):
    nq, ni = extents(shape, which)
    call = make(sf, Fill(sf, torch_mod, dtype_name), nq, ni)
    want = call()                       # _f64_variant (sf_tensor_* in float32: _f32_variant) with SF_VARIANT_AUTO
    called = []
    with monkeypatch.context() as m:
        m.setattr(sf.bwdtrans, "_entry", plain_entry(sf, called))
        got = call()
    torch_mod.cuda.synchronize()
    sfx = "f32" if dtype_name == F32 else "f64"
    assert called == [f"sf_{make.__name__}_{shape}_{sfx}"]
    assert written(torch_mod, want) and same_bits(torch_mod, got, want), (make.__name__, shape, which)


@pytest.mark.parametrize("which", list(EXTENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("make", PATCHED, ids=lambda f: f.__name__)
def test_plain_f64_equals_the_auto_variant(sf, torch_mod, monkeypatch, make, shape, which):
    through_both(sf, torch_mod, monkeypatch, make, shape, which, F64)


@pytest.mark.parametrize("which", list(EXTENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tensor_plain_f32_equals_the_auto_variant(sf, torch_mod, monkeypatch, shape, which):
    through_both(sf, torch_mod, monkeypatch, tensor, shape, which, F32)


def direct(sf, torch_mod, name, *args):
    """capi.lib().<name>(*args, the current stream), tensors as their device addresses; the return code is checked."""
    args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch_mod.Tensor) else a for a in args]
    rc = getattr(sf.capi.lib(), name)(*args, ctypes.c_void_p(torch_mod.cuda.current_stream().cuda_stream))
    sf.capi.check(rc, name)


@pytest.mark.parametrize("which", list(EXTENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bwdtrans_plain_f64_equals_the_auto_variant(sf, torch_mod, shape, which):
    nq, ni = extents(shape, which)
    mk = Fill(sf, torch_mod, F64)
    b, _, _ = mk.matrices(nq)
    inp = mk(NELMT * prod(ni))
    want = pick(sf, "bwdtrans", nq)(nq, *b, inp)                    # sf_bwdtrans_*_f64_variant(AUTO, ..., wsp = NULL, ...)
    got = torch_mod.zeros_like(want)
    direct(sf, torch_mod, f"sf_bwdtrans_{shape}_f64", *nq, NELMT, *b, inp, got)
    torch_mod.cuda.synchronize()
    assert written(torch_mod, want) and same_bits(torch_mod, got, want), (shape, which)


@pytest.mark.parametrize("which", list(EXTENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_geom_affine_f64_is_point_zero_of_geom(sf, torch_mod, shape, which):
    """dfe, je and (with unit weights in the sf_geom_* call) ge against point (0, 0, 0) of sf_geom_*: see the module's
    docstring.  Each output buffer has room for the largest of the three."""
    nq, ni = extents(shape, which)
    d, nqt = len(nq), prod(nq)
    ncomp = d * (d + 1) // 2
    mk = Fill(sf, torch_mod, F64)
    b, ds, _ = mk.matrices(nq)
    xs = [mk(NELMT * prod(ni)) for _ in nq]
    ones = [torch_mod.ones(q, dtype=torch_mod.float64, device="cuda") for q in nq]
    full = pick(sf, "geom", nq)(nq, *b, *ds, *ones, xs)
    dfe, ge, je = (torch_mod.zeros(NELMT * d * d, dtype=torch_mod.float64, device="cuda")[:NELMT * per]
                   for per in (d * d, ncomp, 1))
    direct(sf, torch_mod, f"sf_geom_affine_{shape}_f64", *nq, NELMT, *b, *ds, *xs, dfe, ge, je)
    torch_mod.cuda.synchronize()
    point0 = lambda t, planes: t.view(NELMT, planes, nqt)[:, :, 0].reshape(-1)      # noqa: E731
    assert written(torch_mod, [dfe, ge, je])
    assert same_bits(torch_mod, dfe, point0(full["df"], d * d)), (shape, which)
    assert same_bits(torch_mod, je, point0(full["detj"], 1).abs()), (shape, which)
    assert same_bits(torch_mod, ge, point0(full["g"], ncomp)), (shape, which)
