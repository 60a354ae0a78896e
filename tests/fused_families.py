"""One adapter per fused operator family (sf_iproduct_*, sf_mass_*, sf_helmholtz_*, sf_affine_helmholtz_*, sf_physderiv_*,
sf_iprodderiv_*), so that tests/test_gpu_fused_offsets.py, test_gpu_fused_scale.py, test_gpu_fused_extents.py and
test_fused_refs_cpu.py are written once and parametrised over the six.  An adapter gives

  * the per-element operands of the call: name, scalars per element, the alignment variant "wave" asks of it, whether
    the call may leave it out (None), and the seed of its data;
  * the call itself, with out= and variant=;
  * the long-double reference and the fp64 numpy reference with the family's own bound, straight from tests/*_ref.py
    (ref_*, *_f64 / affine_eval, *_excess, *_n): no tolerance is introduced here;
  * the wave orders of its table.

Alignment (csrc/capi.hip: validate() asks sizeof(T) of every pointer; route() asks 16 bytes of the two pointers each
family hands it; the families' test_scalar_aligned_* tests show the same from outside):

    family      16-byte aligned (VEC)          scalar aligned (SCALAR)
    iproduct    in, out                        -
    mass        in, out                        w
    helmholtz   in, out                        g, w
    affine      in, out                        ge, je
    physderiv   in, out0 .. out{d-1}           df
    iprodderiv  out                            in0 .. in{d-1}, df, w

Data: sf.fill_random, seeded, per-value distinct, uniform in [-1, 1): every coefficient (w, g, df, ge, je, qw) takes both
signs -- none of the operators needs a definite one, and the bounds are stated on absolute values.  The Helmholtz
families run with lambda = 0.75 when the mass coefficient (w / je) is present and with lambda = 0 when it is None.

HEX64 / QUAD64 and the *_PINNED tables mirror the (EC, WPB) columns of csrc/wave_table.h and the EC overrides of
csrc/helmholtz_launch.h, which the affine, physderiv and iprodderiv launchers share: a workgroup of a wave kernel takes
EC * WPB elements (wave_launch.h launch_chunked, KMAP = 1 on every row).  SMALL_CAP and the extent bounds mirror the
constants of the any-extent kernels.  tests/test_fused_refs_cpu.py compares every mirror with the sources.
"""
import collections
import concurrent.futures

import numpy as np

from affine_ref import affine_eval, affine_excess, affine_n, ref_affine
from helm_ref import COMPONENTS, helm_excess, helm_n, helmholtz_f64, ref_helmholtz
from iprod_ref import U64, elementwise_excess, f64_factor, gamma, iprod_f64, ref_iprod, unit_roundoff  # noqa: F401
from iprodderiv_ref import iprodderiv_excess, iprodderiv_f64, iprodderiv_n, ref_iprodderiv
from mass_ref import mass_excess, mass_f64, mass_n, ref_mass
from physderiv_ref import physderiv_excess, physderiv_f64, physderiv_n, ref_physderiv

LAM = 0.75
VEC, SCALAR = "vec", "scalar"

# name, scalars per element, VEC / SCALAR, may be None, seed of its data
Operand = collections.namedtuple("Operand", "name per align optional seed")


def sizes(nq):
    """(modes, points) per element."""
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def _abs(a):
    return None if a is None else np.abs(a)


class Family:
    """What the tests need of one family.  `consts` names the small per-call arrays (bs: bases, ds: derivative matrices,
    qs: one-dimensional quadrature weights); `modes` lists which optional operands are present, the full set first."""
    name = ""
    hex_orders = range(2, 9)
    quad_orders = range(2, 17)
    consts = ("bs",)
    modes = ((),)
    helm_rows = True                      # the EC overrides of helmholtz_launch.h apply

    @property
    def wave_orders(self):
        return [(3, n) for n in self.hex_orders] + [(2, n) for n in self.quad_orders]

    def operands(self, nq):
        raise NotImplementedError

    def out_parts(self, nq):
        return 1

    def out_per(self, nq):
        return sizes(nq)[0]

    def largest_stream(self, nq):
        """(name, scalars per element) of the longest array of a call; an input wins a tie."""
        best = max(self.operands(nq), key=lambda o: o.per)
        return (best.name, best.per) if best.per >= self.out_per(nq) else ("out", self.out_per(nq))

    def lam(self, d):
        return 0.0

    def _fn(self, sf, nq):
        return getattr(sf, f"{self.stem}_{'hex' if len(nq) == 3 else 'quad'}")

    def __repr__(self):
        return self.name


class IProduct(Family):
    name, stem, hex_orders, helm_rows = "iproduct", "iproduct", range(2, 12), False

    def operands(self, nq):
        return [Operand("in", sizes(nq)[1], VEC, False, 10)]

    def call(self, sf, nq, c, d, out, variant):
        return [self._fn(sf, nq)(nq, *c["bs"], d["in"], out=out and out[0], variant=variant)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_iprod if ld else iprod_f64)(nq, n, c["bs"], d["in"])

    excess = staticmethod(elementwise_excess)

    def n(self, nq):
        return sum(int(q) for q in nq)


class Mass(Family):
    name, stem, hex_orders, helm_rows = "mass", "mass", range(2, 12), False

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("w", nqt, SCALAR, False, 7000)]

    def call(self, sf, nq, c, d, out, variant):
        return [self._fn(sf, nq)(nq, *c["bs"], d["w"], d["in"], out=out and out[0], variant=variant)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_mass if ld else mass_f64)(nq, n, c["bs"], d["w"], d["in"])

    excess = staticmethod(mass_excess)
    n = staticmethod(mass_n)


class Helmholtz(Family):
    name, stem, consts, modes = "helmholtz", "helmholtz", ("bs", "ds"), (("w",), ())

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("g", len(COMPONENTS[len(nq)]) * nqt, SCALAR, False, 8000),
                Operand("w", nqt, SCALAR, True, 7000)]

    def lam(self, d):
        return LAM if d["w"] is not None else 0.0

    def call(self, sf, nq, c, d, out, variant):
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["g"], d["w"], self.lam(d), d["in"], out=out and out[0],
                                 variant=variant)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_helmholtz if ld else helmholtz_f64)(nq, n, c["bs"], c["ds"], d["g"], d["w"], self.lam(d), d["in"])

    excess = staticmethod(helm_excess)
    n = staticmethod(helm_n)


class Affine(Family):
    name, stem, consts, modes = "affine", "affine_helmholtz", ("bs", "ds", "qs"), (("je",), ())

    def operands(self, nq):
        return [Operand("in", sizes(nq)[0], VEC, False, 10), Operand("ge", len(COMPONENTS[len(nq)]), SCALAR, False, 8000),
                Operand("je", 1, SCALAR, True, 7000)]

    def lam(self, d):
        return LAM if d["je"] is not None else 0.0

    def call(self, sf, nq, c, d, out, variant):
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], *c["qs"], d["ge"], d["je"], self.lam(d), d["in"],
                                 out=out and out[0], variant=variant)]

    def ref(self, nq, n, c, d, ld=True):
        lam = self.lam(d)
        if ld:
            return ref_affine(nq, n, c["bs"], c["ds"], c["qs"], d["ge"], d["je"], lam, d["in"])
        f = np.float64                   # affine_ref.py has no *_f64 pair: the documented order of operations in fp64
        return (affine_eval(nq, n, c["bs"], c["ds"], c["qs"], d["ge"], d["je"], lam, d["in"], f),
                affine_eval(nq, n, [np.abs(b) for b in c["bs"]], [np.abs(m) for m in c["ds"]],
                            [np.abs(q) for q in c["qs"]], np.abs(d["ge"]), _abs(d["je"]), abs(lam), np.abs(d["in"]), f))

    excess = staticmethod(affine_excess)
    n = staticmethod(affine_n)


class PhysDeriv(Family):
    name, stem, consts, modes = "physderiv", "physderiv", ("bs", "ds"), (("df",), ())

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("df", len(nq) ** 2 * nqt, SCALAR, True, 8000)]

    def out_parts(self, nq):
        return len(nq)

    def out_per(self, nq):
        return sizes(nq)[1]

    def call(self, sf, nq, c, d, out, variant):
        got = self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["df"], d["in"], out=out, variant=variant)
        return [got[a] for a in range(len(nq))]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_physderiv if ld else physderiv_f64)(nq, n, c["bs"], c["ds"], d["df"], d["in"])

    excess = staticmethod(physderiv_excess)
    n = staticmethod(physderiv_n)


class IProdDeriv(Family):
    name, stem, consts = "iprodderiv", "iprodderiv", ("bs", "ds")
    modes = (("df", "w"), ("df",), ("w",), ())

    def operands(self, nq):
        nqt = sizes(nq)[1]
        return ([Operand(f"in{a}", nqt, SCALAR, False, 10 + 2000 * a) for a in range(len(nq))]
                + [Operand("df", len(nq) ** 2 * nqt, SCALAR, True, 8000), Operand("w", nqt, SCALAR, True, 9000)])

    def call(self, sf, nq, c, d, out, variant):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["df"], d["w"], ins, out=out and out[0], variant=variant)]

    def ref(self, nq, n, c, d, ld=True):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return (ref_iprodderiv if ld else iprodderiv_f64)(nq, n, c["bs"], c["ds"], d["df"], d["w"], ins)

    excess = staticmethod(iprodderiv_excess)
    n = staticmethod(iprodderiv_n)


FAMILIES = [IProduct(), Mass(), Helmholtz(), Affine(), PhysDeriv(), IProdDeriv()]
BY_NAME = {f.name: f for f in FAMILIES}
WAVE_CASES = [(f, dim, nq) for f in FAMILIES for dim, nq in f.wave_orders]


def case_id(v):
    if isinstance(v, Family):
        return v.name
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def wave_ids():
    return [f"{f.name}-{d}d-nq{n}" for f, d, n in WAVE_CASES]


# ---- the (EC, WPB) of every wave row -----------------------------------------------------------------------------------
# csrc/wave_table.h: SF_HEX_CFG / SF_QUAD_CFG (fp64); HexCfgF32 / QuadCfgF32 (fp32: twice the fp64 EC unless pinned)
HEX64 = {2: (128, 4), 3: (14, 2), 4: (4, 8), 5: (2, 4), 6: (2, 8), 7: (1, 4), 8: (1, 8), 9: (1, 4), 10: (1, 4), 11: (1, 4)}
HEX32_PINNED = {3: (28, 4), 6: (4, 4), 7: (4, 4), 9: (4, 2)}
QUAD64 = {2: (128, 4), 3: (42, 4), 4: (16, 4), 5: (8, 4), 6: (8, 4), 7: (6, 4), 8: (4, 4), 9: (4, 4), 10: (4, 8), 11: (4, 4),
          12: (3, 4), 13: (4, 4), 14: (4, 4), 15: (4, 8), 16: (4, 4)}
QUAD32_PINNED = {4: (32, 4), 5: (16, 4), 6: (16, 4), 7: (16, 4), 8: (8, 4), 9: (8, 4), 10: (8, 4), 11: (8, 4), 12: (4, 4),
                 13: (16, 4), 14: (4, 4), 15: (4, 4), 16: (4, 4)}


def table_row(dim, nq, dtype_name):
    """(EC, WPB) of the BwdTrans row: what sf_iproduct_* and sf_mass_* run."""
    f64, pinned = (HEX64, HEX32_PINNED) if dim == 3 else (QUAD64, QUAD32_PINNED)
    if dtype_name == "float64":
        return f64[nq]
    return pinned.get(nq, (2 * f64[nq][0], f64[nq][1]))


def helm_ec(dim, nq, row_ec, dtype_name):
    """helm_hex_ec() / helm_quad_ec() of csrc/helmholtz_launch.h."""
    if dim == 3:
        if nq == 6 and dtype_name == "float64":
            return 1
        return min(row_ec, max(1, 128 // (nq * nq)))
    return min(row_ec, 128 // nq) if nq >= 9 else row_ec


def wave_row(fam, dim, nq, dtype_name):
    """(EC, WPB) of the family's wave kernel at this order."""
    ec, wpb = table_row(dim, nq, dtype_name)
    return (helm_ec(dim, nq, ec, dtype_name) if fam.helm_rows else ec), wpb


# ---- seeded data of one case on the device -----------------------------------------------------------------------------
def to_host(t):
    return None if t is None else t.detach().cpu().numpy()


class Problem:
    """Seeded data of one case, on the device.  Every operand is element-major, so the first n elements of a problem are
    a problem of n elements: a reference computed once at the largest count serves its prefixes."""

    def __init__(self, fam, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.fam, self.nq, self.nelmt, self.dtype_name = fam, tuple(nq), nelmt, dtype_name
        self.ops = fam.operands(self.nq)
        sets = {"bs": (500, lambda q: (q - 1) * q), "ds": (600, lambda q: q * q), "qs": (700, lambda q: q)}
        self.consts = {k: [sf.fill_random(sets[k][1](q), sets[k][0] + 7 * seed + d, dtype=dtype)
                           for d, q in enumerate(self.nq)] for k in fam.consts}
        self.data = {o.name: sf.fill_random(nelmt * o.per, o.seed + seed, dtype=dtype) for o in self.ops}
        self.seeds = {o.name: o.seed + seed for o in self.ops}
        self._host_consts = None

    def window(self, lo=0, n=None, present=None):
        """The operands of elements lo .. lo + n as views; an optional operand that is not in `present` is None."""
        n = self.nelmt - lo if n is None else n
        present = self.fam.modes[0] if present is None else present
        return {o.name: None if o.optional and o.name not in present else self.data[o.name][lo * o.per:(lo + n) * o.per]
                for o in self.ops}

    def run(self, sf, lo=0, n=None, present=None, data=None, out=None, variant="auto"):
        """The operator on elements lo .. lo + n (or on `data`, a dict like window()'s); returns the list of outputs."""
        d = self.window(lo, n, present) if data is None else data
        return self.fam.call(sf, self.nq, self.consts, d, out, variant)

    def reference(self, lo=0, n=None, present=None, ld=True):
        """(ref, absref), each of shape (out_parts, n * out_per): long double, or fp64 sweeps with ld=False."""
        n = self.nelmt - lo if n is None else n
        if self._host_consts is None:
            self._host_consts = {k: [to_host(t) for t in v] for k, v in self.consts.items()}
        d = {k: to_host(v) for k, v in self.window(lo, n, present).items()}
        ref, absref = self.fam.ref(self.nq, n, self._host_consts, d, ld)
        parts = self.fam.out_parts(self.nq)
        return np.asarray(ref).reshape(parts, -1), np.asarray(absref).reshape(parts, -1)

    def excess(self, got, ref, absref, factor=1.0):
        """max |err| / (factor gamma_N absref) of a list of output tensors (or one host array) against a reference."""
        if isinstance(got, (list, tuple)):
            got = np.stack([to_host(t) for t in got])
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return self.fam.excess(got, ref, absref, self.nq, unit_roundoff(self.dtype_name), factor=factor)

    def f64_factor(self):
        """The factor on gamma_N(u) absref64 for a result of unit roundoff u against the fp64 reference: iprod_ref.f64_factor
        at the family's N."""
        return f64_factor(self.fam.n(self.nq), unit_roundoff(self.dtype_name))


def excess_over_slices(p, outs, present, step, lo=0):
    """max |err| / (f64_factor gamma_N absref64) of elements lo .. nelmt against the fp64 reference, `step` elements
    at a time; the slices are independent, so four host threads share them."""
    per, factor = p.fam.out_per(p.nq), p.f64_factor()

    def one(a):
        n = min(step, p.nelmt - a)
        ref, absref = p.reference(a, n, present, ld=False)
        return p.excess([t[a * per:(a + n) * per] for t in outs], ref, absref, factor=factor)

    p.reference(lo, 1, present, ld=False)                     # the host copies of the small arrays, made once
    with concurrent.futures.ThreadPoolExecutor(4) as pool:
        return max(pool.map(one, range(lo, p.nelmt, step)))


def host_case(fam, nq, nelmt, present, seed):
    """(consts, data) of a small case as fp64 numpy arrays, for the tests that run no GPU."""
    rng = np.random.default_rng(seed)
    per = {"bs": lambda q: (q - 1) * q, "ds": lambda q: q * q, "qs": lambda q: q}
    consts = {k: [rng.uniform(-1, 1, per[k](q)) for q in nq] for k in fam.consts}
    data = {o.name: None if o.optional and o.name not in present else rng.uniform(-1, 1, nelmt * o.per)
            for o in fam.operands(tuple(nq))}
    return consts, data


# ---- the any-extent kernels: LDS classes and extent bounds ------------------------------------------------------------
# Each any-extent kernel is built twice, over a static lds[CAP] of a small class (2048 scalars, 64 threads) and of a large
# one (256 threads); the launcher picks by a formula per family, at this commit:
#   helm class (helmholtz, affine, physderiv, iprodderiv; helm_need() of csrc/helmholtz_generic.h):
#       small iff 4 nq0 nq1 nq2 <= 2048 (3D), 3 nq0 nq1 <= 2048 (2D); extents up to 12 (3D) and 32 (2D)
#   mass (mass_regions() of csrc/mass_generic.hip): small iff nq0 nq1 nq2 + nq0 nq1 (nq2 - 1) <= 2048 (3D),
#       nq0 nq1 + nq0 (nq1 - 1) <= 2048 (2D: at most 32 * 63 = 2016, always small); extents up to 16 (3D) and 32 (2D)
#   iproduct (`need` of csrc/iproduct_generic.hip): small iff (2 nq0 - 1) nq1 nq2 <= 2048 (3D), (2 nq0 - 1) nq1 <= 2048
#       (2D: at most 63 * 32 = 2016, always small -- the 2D kernel of the large class is never launched); same extents
def lds_need(fam, nq):
    """The left-hand side of the family's class formula, in scalars."""
    nq = [int(q) for q in nq]
    if fam.helm_rows:
        return (4 if len(nq) == 3 else 3) * int(np.prod(nq))
    nz = nq[2] if len(nq) == 3 else 1
    if fam.name == "mass":
        return nq[0] * nq[1] * nz + (nq[0] * nq[1] * (nz - 1) if len(nq) == 3 else nq[0] * (nq[1] - 1))
    return (2 * nq[0] - 1) * nq[1] * nz


SMALL_CAP = 2048                      # kHelmSmallCap, kMassSmallCap, kIprodSmallCap
MAX_EXTENT = {"helm": (12, 32), "wide": (16, 32)}    # (3D, 2D): kHelmMax*, kMassMax* / kIprodMax*

# (shape, "small" / "large"), the need beside each
HELM_BOUNDARY = [((8, 8, 8), "small"),      # 4 * 512 = 2048: the last small 3D shape
                 ((22, 31), "small"),       # 3 * 682 = 2046
                 ((31, 22), "small"),       # 3 * 682 = 2046
                 ((26, 26), "small"),       # 3 * 676 = 2028
                 ((8, 8, 9), "large"),      # 4 * 576 = 2304
                 ((9, 8, 8), "large"),      # 4 * 576 = 2304
                 ((23, 30), "large"),       # 3 * 690 = 2070
                 ((30, 23), "large"),       # 3 * 690 = 2070
                 ((32, 22), "large"),       # 3 * 704 = 2112
                 ((12, 12, 12), "large")]   # 4 * 1728 = 6912 = the large class itself
MASS_BOUNDARY = [((10, 10, 10), "small"),   # 100 * 19 = 1900
                 ((16, 16, 4), "small"),    # 256 * 7 = 1792
                 ((12, 12, 7), "small"),    # 144 * 13 = 1872
                 ((8, 8, 16), "small"),     # 64 * 31 = 1984
                 ((11, 11, 9), "large"),    # 121 * 17 = 2057
                 ((16, 16, 5), "large"),    # 256 * 9 = 2304
                 ((12, 12, 8), "large"),    # 144 * 15 = 2160
                 ((16, 16, 16), "large")]   # 256 * 31 = 7936 = the large class itself
IPROD_BOUNDARY = [((10, 10, 10), "small"),  # 19 * 100 = 1900
                  ((9, 11, 11), "large"),   # 17 * 121 = 2057
                  ((16, 16, 16), "large"),  # 31 * 256 = 7936 = the large class itself
                  # 2D: (2 nq0 - 1) nq1 <= 63 * 32 = 2016 < 2048 for every extent the kernel takes, so the formula puts no 2D
                  # shape on the large side; the two shapes nearest the switch stand in for the pair
                  ((32, 32), "small"),      # 63 * 32 = 2016
                  ((32, 31), "small")]      # 63 * 31 = 1953
# a one-mode direction (extent 2) beside the largest extent
HELM_ONE_MODE = [(2, 32), (32, 2), (2, 2, 12), (12, 2, 2), (2, 12, 2), (12, 12, 4), (4, 12, 12)]
WIDE_ONE_MODE = [(2, 32), (32, 2), (2, 2, 16), (16, 2, 2), (2, 16, 2), (16, 16, 4), (4, 16, 16)]
HELM_PAST = [(33, 2), (2, 33), (13, 2, 2)]
WIDE_PAST = [(33, 2), (2, 33), (17, 2, 2)]


def boundary_shapes(fam):
    return HELM_BOUNDARY if fam.helm_rows else (MASS_BOUNDARY if fam.name == "mass" else IPROD_BOUNDARY)


def one_mode_shapes(fam):
    return HELM_ONE_MODE if fam.helm_rows else WIDE_ONE_MODE


def past_the_bounds(fam):
    return HELM_PAST if fam.helm_rows else WIDE_PAST


def on_wave_table(fam, nq):
    return len(set(nq)) == 1 and nq[0] in (fam.hex_orders if len(nq) == 3 else fam.quad_orders)
