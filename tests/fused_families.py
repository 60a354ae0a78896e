"""One adapter per fused operator family (sf_iproduct_*, sf_mass_*, sf_helmholtz_*, sf_affine_helmholtz_*, sf_physderiv_*,
sf_iprodderiv_* -- FAMILIES -- and sf_diag_helmholtz_*, which joins them in COMMON), so that what the families' GPU tests
have in common is written once: tests/fused_common.py and tests/test_gpu_fused_common.py over COMMON; test_gpu_fused_offsets.py,
test_gpu_fused_scale.py, test_gpu_fused_extents.py and test_fused_refs_cpu.py over FAMILIES.  An adapter gives

  * the per-element operands of the call: name, scalars per element, the alignment variant "wave" asks of it, whether
    the call may leave it out (None), and the seed of its data;
  * the call itself, with out=, variant= and stream=;
  * the long-double reference and the fp64 numpy reference with the family's own bound, straight from tests/*_ref.py
    (ref_*, *_f64 / affine_eval, *_excess, *_n): no tolerance is introduced here;
  * the wave orders of its table;
  * the literals of the common tests (shapes, element counts, seeds, refused variants), each family with the values its
    own test file had, and prepare(): what the family's own tests ask of the data beyond the uniform arrays.

Beside the adapters: Problem (the seeded data of one case, its runs, references and checks), check_bound() (the one
assertion of the common tests, on host arrays: tests/test_fused_helpers_cpu.py), Banded (guard bands), and the `sf` and
`torch_mod` fixtures that the GPU test files import.

Alignment (csrc/capi.hip: validate() asks sizeof(T) of every pointer; route() asks 16 bytes of the two pointers each
family hands it; the families' test_scalar_aligned_* tests show the same from outside):

    family      16-byte aligned (VEC)          scalar aligned (SCALAR)
    iproduct    in, out                        -
    mass        in, out                        w
    helmholtz   in, out                        g, w
    affine      in, out                        ge, je
    physderiv   in, out0 .. out{d-1}           df
    iprodderiv  out                            in0 .. in{d-1}, df, w
    diag        out                            g, w, the tables

Data: sf.fill_random, seeded, per-value distinct, uniform in [-1, 1): every coefficient (w, g, df, ge, je, qw) takes both
signs -- none of the operators needs a definite one, and the bounds are stated on absolute values.  The Helmholtz
families run with lambda = 0.75 when the mass coefficient (w / je) is present and with lambda = 0 when it is None.
own_problem() is a Problem after the family's prepare(): the data of the family's own test file where that asks more
(mass: w = 0.25 + |w|, a definite matrix; iprodderiv: the d inputs are the rows of one array of one seed; diag: the tables).

HEX64 / QUAD64 and the *_PINNED tables mirror the (EC, WPB) columns of csrc/wave_table.h and the EC overrides of
csrc/helmholtz_launch.h, which the affine, physderiv and iprodderiv launchers share: a workgroup of a wave kernel takes
EC * WPB elements (wave_launch.h launch_chunked, KMAP = 1 on every row).  SMALL_CAP and the extent bounds mirror the
constants of the any-extent kernels.  tests/test_fused_refs_cpu.py compares every mirror with the sources.
"""
import collections
import concurrent.futures

import numpy as np
import pytest

from affine_ref import affine_eval, affine_excess, affine_n, ref_affine
from diag_ref import diag_excess, diag_f64, diag_n, ref_diag
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


RAGGED = (1, 2, 3, 5, 13, 15, 63, 65, 127, 257, 1001)
WIDE_RAGGED = (1, 2, 3, 5, 13, 14, 15, 63, 64, 65, 127, 257, 1000, 4099)          # tests/test_gpu_specialise.py
F64, F32 = "float64", "float32"


def _cases(f64, f32):
    return tuple((s, F64) for s in f64) + tuple((s, F32) for s in f32)


HELM_RAGGED_SHAPES = _cases([(2, 2, 2), (3, 3, 3), (4, 4, 4), (6, 6, 6), (7, 7, 7), (8, 8, 8), (3, 3), (7, 7), (8, 8),
                             (12, 12), (16, 16)], [(3, 3, 3), (6, 6, 6), (8, 8, 8), (7, 7), (13, 13)])
HELM_FALLBACK = ((6, 6, 12), (3, 5, 4), (12, 10, 11), (2, 3, 2), (9, 9, 9), (11, 11, 11), (12, 12, 12), (4, 9), (16, 3),
                 (32, 32), (23, 5))
WIDE_FALLBACK = ((6, 6, 12), (3, 5, 4), (16, 12, 14), (2, 3, 2), (13, 13, 13), (4, 9), (16, 3), (32, 32), (23, 5))
HELM_GUARD = {(3, 3, 3): 1001, (6, 6, 6): 129, (7, 7, 7): 257, (8, 8, 8): 65, (2, 2, 2): 33, (5, 5): 4099, (13, 13): 1000,
              (16, 16): 127, (6, 6, 12): 13, (23, 5): 14, (9, 9, 9): 15}
WIDE_GUARD = {(3, 3, 3): 1001, (7, 7, 7): 257, (8, 8, 8): 65, (9, 9, 9): 63, (11, 11, 11): 15, (5, 5): 4099, (13, 13): 1000,
              (16, 16): 127, (6, 6, 12): 13, (23, 5): 14}
NO_KERNEL = ("wave", "mfma", "mfma4", "thread", "block-lds", "block-glb", "wave-rt")      # at a shape off the wave table


def _refused(*groups):
    """((shapes, elements, variants), ...) -> the (shape, elements, dtype, variant) of Family.refused, fp64."""
    return tuple((nq, n, F64, v) for shapes, n, variants in groups for nq in shapes for v in variants)


class Family:
    """What the tests need of one family.  `consts` names the small per-call arrays (bs: bases, ds: derivative matrices,
    qs: one-dimensional quadrature weights); `modes` lists which optional operands are present, the full set first."""
    name = ""
    hex_orders = range(2, 9)
    quad_orders = range(2, 17)
    consts = ("bs",)
    modes = ((),)
    helm_rows = True                      # the EC overrides of helmholtz_launch.h apply

    # ---- the literals of the common tests (tests/fused_common.py), each with the value the family's own file had ----------------
    auto_count = 403                      # elements per wave order
    ragged, ragged_seed = RAGGED, staticmethod(lambda n: n % 101)            # counts, and the seed of each one's problem
    ragged_shapes = HELM_RAGGED_SHAPES
    fallback = HELM_FALLBACK              # shapes off the wave table
    fallback_counts, fallback_seed = (1, 37, 150), staticmethod(lambda n: 70 + n)
    explicit_count = 777
    refused = ()                          # (shape, elements, dtype, variant) that answer SF_ENOTBUILT
    guard = {}                            # shape -> elements
    guard_test = "test_guard_values_around_out_and_nan_around_the_inputs"      # the name the family's file gave the test
    guarded_consts = ()                   # the small arrays that also sit between NaN bands
    graph = (((8, 8, 8), 20011), ((9, 9), 5003))
    graph_bound = False                   # the replayed result is also held to the long-double bound
    first_call = (((8, 8, 8), 5001), ((6, 6, 12), 301), ((9, 9), 2001), ((23, 5), 301))
    streams = (((7, 7, 7), 30011), ((12, 12), 100003))
    stream_sample, stream_ld = None, False      # every element against the fp64 sweeps

    def auto_counts(self, dim, nq):
        return (self.auto_count,)

    def plan(self, counts, seed):
        """(elements, seed, counts to run) of the problems that serve `counts`: one problem per count."""
        return [(n, seed(n), (n,)) for n in counts]

    def guard_counts(self, nq, dtype_name):
        return (self.guard[nq],)

    def prepare(self, p, sf):
        """What own_problem() adds to the uniform data of a Problem."""

    def f64_factor(self, nq, u):
        """The factor on gamma_N(u) absref64 against the family's fp64 reference."""
        return f64_factor(self.n(nq), u)

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


class Wide(Family):
    """sf_iproduct_* and sf_mass_*: the rows of the BwdTrans table, hex orders up to 11, the wider any-extent kernels."""
    hex_orders, helm_rows = range(2, 12), False
    auto_count, ragged, fallback, fallback_counts, guard = 1003, WIDE_RAGGED, WIDE_FALLBACK, (1, 37, 300), WIDE_GUARD
    graph, graph_bound = Family.graph + (((6, 6, 12), 1001),), True
    streams = (((7, 7, 7), 100003), ((12, 12), 200009))


class IProduct(Wide):
    name = stem = "iproduct"
    guard_test = "test_guard_values_around_out"
    ragged_shapes = _cases([(2, 2, 2), (3, 3, 3), (8, 8, 8), (11, 11, 11), (3, 3), (7, 7), (16, 16)],
                           [(3, 3, 3), (9, 9, 9), (7, 7), (13, 13)])

    def operands(self, nq):
        return [Operand("in", sizes(nq)[1], VEC, False, 10)]

    def call(self, sf, nq, c, d, out, variant, **kw):
        return [self._fn(sf, nq)(nq, *c["bs"], d["in"], out=out and out[0], variant=variant, **kw)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_iprod if ld else iprod_f64)(nq, n, c["bs"], d["in"])

    excess = staticmethod(elementwise_excess)

    def n(self, nq):
        return sum(int(q) for q in nq)


class Mass(Wide):
    name = stem = "mass"
    guard_test = "test_guard_values_around_out_and_nan_around_w"
    # EC > 1 rows (3D nq 2..6, every 2D row), EC = 1 rows (3D nq 7..11), word-grid input rows (one element with an odd
    # number of modes: 3D nq 8 / 10 in fp64) and fp32
    ragged_shapes = _cases([(2, 2, 2), (3, 3, 3), (4, 4, 4), (6, 6, 6), (7, 7, 7), (8, 8, 8), (10, 10, 10), (11, 11, 11),
                            (3, 3), (7, 7), (8, 8), (12, 12), (16, 16)],
                           [(3, 3, 3), (8, 8, 8), (9, 9, 9), (7, 7), (13, 13)])

    def prepare(self, p, sf):
        p.data["w"] = 0.25 + p.data["w"].abs()          # the mass matrix of the family's own tests is definite

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("w", nqt, SCALAR, False, 7000)]

    def call(self, sf, nq, c, d, out, variant, **kw):
        return [self._fn(sf, nq)(nq, *c["bs"], d["w"], d["in"], out=out and out[0], variant=variant, **kw)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_mass if ld else mass_f64)(nq, n, c["bs"], d["w"], d["in"])

    excess = staticmethod(mass_excess)
    n = staticmethod(mass_n)


class Helmholtz(Family):
    name, stem, consts, modes = "helmholtz", "helmholtz", ("bs", "ds"), (("w",), ())
    guard, graph = HELM_GUARD, Family.graph + (((6, 6, 12), 1001),)
    guard_test = "test_guard_values_around_out_and_nan_around_g_and_w"
    refused = _refused((((9, 9, 9),), 5, ("wave", "mfma")), (((13, 4, 4),), 2, ("auto",)))

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("g", len(COMPONENTS[len(nq)]) * nqt, SCALAR, False, 8000),
                Operand("w", nqt, SCALAR, True, 7000)]

    def lam(self, d):
        return LAM if d["w"] is not None else 0.0

    def call(self, sf, nq, c, d, out, variant, **kw):
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["g"], d["w"], self.lam(d), d["in"], out=out and out[0],
                                 variant=variant, **kw)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_helmholtz if ld else helmholtz_f64)(nq, n, c["bs"], c["ds"], d["g"], d["w"], self.lam(d), d["in"])

    excess = staticmethod(helm_excess)
    n = staticmethod(helm_n)


class Affine(Family):
    name, stem, consts, modes = "affine", "affine_helmholtz", ("bs", "ds", "qs"), (("je",), ())
    # where the lane -> element map can go wrong: many elements per wave in two passes (3D nq 2, 3), two elements (nq 5),
    # one element and uniform constants (nq 6, 7, 8), the 2D chunk sizes, and the shrunk fp32 rows
    ragged_shapes = _cases([(2, 2, 2), (3, 3, 3), (5, 5, 5), (6, 6, 6), (7, 7, 7), (8, 8, 8), (3, 3), (8, 8), (12, 12),
                            (16, 16)], [(6, 6, 6), (13, 13)])
    fallback = ((6, 6, 12), (3, 5, 4), (2, 3, 2), (9, 9, 9), (12, 12, 12), (4, 9), (16, 3), (32, 32), (23, 5))
    ragged_seed, fallback_seed = staticmethod(lambda n: 3), staticmethod(lambda n: 70)
    explicit_count, guarded_consts = 333, ("qs",)
    refused = (_refused((((13, 4, 4),), 3, ("auto",)), (((4, 4, 13),), 3, ("generic",)), (((33, 5), (5, 33)), 3, ("auto",)),
                        (((9, 9, 9), (6, 6, 12), (17, 17)), 3, ("wave",)), (((8, 8, 8),), 3, ("mfma",)))
               + (((13, 4, 4), 3, F32, "auto"),))
    guard = {(2, 2, 2): 33, (3, 3, 3): 1001, (6, 6, 6): 129, (8, 8, 8): 65, (5, 5): 4099, (16, 16): 127, (6, 6, 12): 13,
             (9, 9, 9): 15}
    graph = (((8, 8, 8), 2003), ((9, 9), 5003), ((6, 6, 12), 301), ((3, 3, 3), 1001))
    first_call = (((8, 8, 8), 1001),) + Family.first_call[1:]
    streams, stream_ld = (((7, 7, 7), 1501), ((12, 12), 4001)), True

    def plan(self, counts, seed):
        """One problem: a run on fewer elements takes a prefix of its arrays and is compared with the prefix of its
        reference (per-element data: the family's arrays are too short for a count to change what is exercised)."""
        return [(max(counts), seed(max(counts)), tuple(counts))]

    def operands(self, nq):
        return [Operand("in", sizes(nq)[0], VEC, False, 10), Operand("ge", len(COMPONENTS[len(nq)]), SCALAR, False, 8000),
                Operand("je", 1, SCALAR, True, 7000)]

    def lam(self, d):
        return LAM if d["je"] is not None else 0.0

    def call(self, sf, nq, c, d, out, variant, **kw):
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], *c["qs"], d["ge"], d["je"], self.lam(d), d["in"],
                                 out=out and out[0], variant=variant, **kw)]

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
    fallback = HELM_FALLBACK[:9] + ((23, 5), (17, 17), (32, 32))
    refused = _refused((((9, 9, 9),), 5, NO_KERNEL), (((6, 6, 12), (17, 17), (4, 9)), 5, ("wave",)),
                       (((8, 8),), 5, ("mfma", "thread")), (((13, 4, 4),), 2, ("auto",)))
    guard = {(3, 3, 3): 1001, (6, 6, 6): 129, (7, 7, 7): 257, (8, 8, 8): 65, (2, 2, 2): 33, (5, 5): 4099, (16, 16): 131}
    guard_test = "test_guard_words_around_every_output_and_nan_around_df"
    first_call = Family.first_call[:2] + (((9, 9), 2002),) + Family.first_call[3:]
    stream_sample, stream_ld = 1024, True               # a seeded sample of elements against long double

    def operands(self, nq):
        nmt, nqt = sizes(nq)
        return [Operand("in", nmt, VEC, False, 10), Operand("df", len(nq) ** 2 * nqt, SCALAR, True, 8000)]

    def out_parts(self, nq):
        return len(nq)

    def out_per(self, nq):
        return sizes(nq)[1]

    def call(self, sf, nq, c, d, out, variant, **kw):
        got = self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["df"], d["in"], out=out, variant=variant, **kw)
        return [got[a] for a in range(len(nq))]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_physderiv if ld else physderiv_f64)(nq, n, c["bs"], c["ds"], d["df"], d["in"])

    excess = staticmethod(physderiv_excess)
    n = staticmethod(physderiv_n)


class IProdDeriv(Family):
    name, stem, consts = "iprodderiv", "iprodderiv", ("bs", "ds")
    modes = (("df", "w"), ("df",), ("w",), ())
    ragged_shapes = ()
    fallback = ((9, 9, 9), (11, 11, 11), (6, 6, 12), (3, 5, 4), (12, 10, 8), (20, 20), (4, 9), (23, 5), (32, 32))
    fallback_counts, explicit_count = (5, 33), 67
    refused = _refused((((9, 9, 9),), 5, NO_KERNEL), (((6, 6, 12), (17, 17), (4, 9)), 5, ("wave",)),
                       (((13, 4, 4),), 2, ("auto",)))
    # shape -> (EC of the fp64 row, EC of the fp32 row): the chunk lengths of csrc/iprodderiv_launch.h
    guard = {(8, 8, 8): (1, 2), (7, 7, 7): (1, 2), (6, 6, 6): (1, 3), (3, 3, 3): (14, 14), (16, 16): (4, 4), (9, 9): (4, 8),
             (2, 2): (128, 256)}
    guard_test = "test_guard_words_around_out_and_nan_around_every_input"
    first_call = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
    streams, stream_sample, stream_ld = (((7, 7, 7), 3011), ((12, 12), 10003)), 256, True

    def auto_counts(self, dim, nq):
        """One element, 97 elements (3 EC + 1 for every row with EC <= 32: ragged last chunks, the two-pass rows, the
        partly filled waves of 3D nq 5 / 6 / 7, the 2D EC override from nq 9) and, for the 2D rows with longer chunks (EC
        up to 256 at nq 2 in fp32), 769."""
        return (1, 97) + ((769,) if dim == 2 and nq <= 4 else ())

    def guard_counts(self, nq, dtype_name):
        ec = self.guard[nq][dtype_name == F32]
        return sorted({1, ec + 1, max(1, 2 * ec - 1)})

    def prepare(self, p, sf):
        """The d inputs as the rows of one (d, n) array of one seed, as sf_physderiv_* returns them."""
        n = p.nelmt * sizes(p.nq)[1]
        rows = sf.fill_random(len(p.nq) * n, 10 + p.seed, dtype=p.dtype).view(len(p.nq), n)
        p.data.update({f"in{a}": rows[a] for a in range(len(p.nq))})

    def operands(self, nq):
        nqt = sizes(nq)[1]
        return ([Operand(f"in{a}", nqt, SCALAR, False, 10 + 2000 * a) for a in range(len(nq))]
                + [Operand("df", len(nq) ** 2 * nqt, SCALAR, True, 8000), Operand("w", nqt, SCALAR, True, 9000)])

    def call(self, sf, nq, c, d, out, variant, **kw):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["df"], d["w"], ins, out=out and out[0], variant=variant, **kw)]

    def ref(self, nq, n, c, d, ld=True):
        ins = [d[f"in{a}"] for a in range(len(nq))]
        return (ref_iprodderiv if ld else iprodderiv_f64)(nq, n, c["bs"], c["ds"], d["df"], d["w"], ins)

    excess = staticmethod(iprodderiv_excess)
    n = staticmethod(iprodderiv_n)


class Diag(Family):
    """sf_diag_helmholtz_*: no `in`; the three tables per direction ride with the small arrays once prepare() has built
    them (None: the call builds them on the way)."""
    name, stem, consts, modes = "diag", "diag_helmholtz", ("bs", "ds"), (("w",), ())
    ragged_shapes = HELM_RAGGED_SHAPES[:11] + _cases([], [(3, 3, 3), (8, 8, 8), (13, 13)])
    refused = _refused((((13, 4, 4),), 2, ("auto", "generic", "wave")), (((8, 8, 8),), 5, ("mfma",)))
    guard, guarded_consts, graph = HELM_GUARD, ("tabs",), ()

    def operands(self, nq):
        nqt = sizes(nq)[1]
        return [Operand("g", len(COMPONENTS[len(nq)]) * nqt, SCALAR, False, 8000), Operand("w", nqt, SCALAR, True, 7000)]

    def lam(self, d):
        return LAM if d["w"] is not None else 0.0

    def prepare(self, p, sf):
        p.consts["tabs"] = [sf.diag_tables(q, b, d) for q, b, d in zip(p.nq, p.consts["bs"], p.consts["ds"])]

    def call(self, sf, nq, c, d, out, variant, **kw):
        return [self._fn(sf, nq)(nq, *c["bs"], *c["ds"], d["g"], d["w"], self.lam(d), out=out and out[0], variant=variant,
                                 tabs=c.get("tabs"), **kw)]

    def ref(self, nq, n, c, d, ld=True):
        return (ref_diag if ld else diag_f64)(nq, n, c["bs"], c["ds"], d["g"], d["w"], self.lam(d))

    excess = staticmethod(diag_excess)
    n = staticmethod(diag_n)

    def f64_factor(self, nq, u):
        """Each side within its own gamma_N of the truth: (gamma_N(u) + gamma_N(u64)) (1 + gamma_N(u64)) absref64."""
        gu, g64 = gamma(diag_n(nq), u), gamma(diag_n(nq), U64)
        return (gu + g64) * (1 + g64) / gu


FAMILIES = [IProduct(), Mass(), Helmholtz(), Affine(), PhysDeriv(), IProdDeriv()]
COMMON = FAMILIES + [Diag()]                                   # tests/fused_common.py, tests/test_gpu_fused_common.py
BY_NAME = {f.name: f for f in COMMON}
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
        self.dtype, self.seed = dtype, seed
        self.ops = fam.operands(self.nq)
        sets = {"bs": (500, lambda q: (q - 1) * q), "ds": (600, lambda q: q * q), "qs": (700, lambda q: q)}
        self.consts = {k: [sf.fill_random(sets[k][1](q), sets[k][0] + 7 * seed + d, dtype=dtype)
                           for d, q in enumerate(self.nq)] for k in fam.consts}
        self.data = {o.name: sf.fill_random(nelmt * o.per, o.seed + seed, dtype=dtype) for o in self.ops}
        self.seeds = {o.name: o.seed + seed for o in self.ops}
        self._host_consts, self._refs = None, {}

    def window(self, lo=0, n=None, present=None):
        """The operands of elements lo .. lo + n as views; an optional operand that is not in `present` is None."""
        n = self.nelmt - lo if n is None else n
        present = self.fam.modes[0] if present is None else present
        return {o.name: None if o.optional and o.name not in present else self.data[o.name][lo * o.per:(lo + n) * o.per]
                for o in self.ops}

    def run(self, sf, lo=0, n=None, present=None, data=None, out=None, variant="auto", consts=None, **kw):
        """The operator on elements lo .. lo + n (or on `data`, a dict like window()'s; on copies `consts` of the small
        arrays); returns the list of outputs.  kw: stream=."""
        d = self.window(lo, n, present) if data is None else data
        return self.fam.call(sf, self.nq, self.consts if consts is None else consts, d, out, variant, **kw)

    def reference(self, lo=0, n=None, present=None, ld=True, sample=None):
        """(ref, absref), each of shape (out_parts, n * out_per): long double, or fp64 sweeps with ld=False; of elements
        lo .. lo + n, or of the elements `sample` (an index tensor on the device)."""
        n = self.nelmt - lo if n is None else n
        if self._host_consts is None:
            self._host_consts = {k: [to_host(t) for t in v] for k, v in self.consts.items()}
        d = self.window(lo, n, present)
        if sample is not None:
            n, d = len(sample), {k: v if v is None else v.reshape(self.nelmt, -1)[sample].reshape(-1) for k, v in d.items()}
        d = {k: to_host(v) for k, v in d.items()}
        ref, absref = self.fam.ref(self.nq, n, self._host_consts, d, ld)
        parts = self.fam.out_parts(self.nq)
        return np.asarray(ref).reshape(parts, -1), np.asarray(absref).reshape(parts, -1)

    def excess(self, got, ref, absref, factor=1.0):
        """max |err| / (factor gamma_N absref) of a list of output tensors (or one host array) against a reference."""
        if isinstance(got, (list, tuple)):
            got = np.stack([to_host(t) for t in got])
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return self.fam.excess(got, ref, absref, self.nq, unit_roundoff(self.dtype_name), factor=factor)

    def check(self, got, what, n=None, present=None):
        """check_bound() of the outputs of a run on the first n elements against the long-double reference, which is
        computed once per combination of optional operands, at every element: a smaller n takes its prefix."""
        n = self.nelmt if n is None else n
        present = self.fam.modes[0] if present is None else present
        if present not in self._refs:
            self._refs[present] = self.reference(present=present)
        ref, absref = (r[:, :n * self.fam.out_per(self.nq)] for r in self._refs[present])
        got = np.stack([to_host(t) for t in got])
        return check_bound(self.fam, self.nq, self.dtype_name, got, ref, absref, f"{what} nelmt={n} present={present}")

    def check_elements(self, outs, what, sample=None, ld=True):
        """check_bound() of the elements `sample` (all of them: None) against a reference of just those: long double, or
        the fp64 sweeps with the family's f64_factor."""
        if sample is None:
            q = excess_over_slices(self, outs, self.fam.modes[0], 8192, ld=ld)
        else:
            ref, absref = self.reference(ld=ld, sample=sample)
            q = self.excess([t.reshape(self.nelmt, -1)[sample].reshape(-1) for t in outs], ref, absref,
                            1.0 if ld else self.f64_factor())
        print(f"{what}: {self.fam.name} {self.nq} {self.dtype_name} nelmt={self.nelmt}: max |err| / "
              f"({'gamma_N absref' if ld else 'f64_factor gamma_N absref64'}) = {q:.3g}")
        assert q <= 1.0, (what, self.fam.name, self.nq, q)

    def f64_factor(self):
        """The factor on gamma_N(u) absref64 for a result of unit roundoff u against the family's fp64 reference."""
        return self.fam.f64_factor(self.nq, unit_roundoff(self.dtype_name))


def excess_over_slices(p, outs, present, step, lo=0, ld=False):
    """max |err| / (f64_factor gamma_N absref64) of elements lo .. nelmt against the fp64 reference (ld: / (gamma_N absref)
    against long double), `step` elements at a time; the slices are independent, so four host threads share them."""
    per, factor = p.fam.out_per(p.nq), 1.0 if ld else p.f64_factor()

    def one(a):
        n = min(step, p.nelmt - a)
        ref, absref = p.reference(a, n, present, ld=ld)
        return p.excess([t[a * per:(a + n) * per] for t in outs], ref, absref, factor=factor)

    p.reference(lo, 1, present, ld=False)                     # the host copies of the small arrays, made once
    with concurrent.futures.ThreadPoolExecutor(4) as pool:
        return max(pool.map(one, range(lo, p.nelmt, step)))


def own_problem(fam, sf, torch_mod, nq, nelmt, dtype_name, seed):
    """A Problem with the data of the family's own test file: Family.prepare() on the uniform arrays (a definite mass
    matrix; the inputs of sf_iprodderiv_* as rows of one array; the tables of sf_diag_helmholtz_*, built once)."""
    p = Problem(fam, sf, torch_mod, nq, nelmt, dtype_name, seed)
    fam.prepare(p, sf)
    return p


def check_bound(fam, nq, dtype_name, got, ref, absref, what, factor=1.0):
    """The assertion of the common tests, on host arrays: max |got - ref| / (factor gamma_N absref) <= 1 with the family's
    N at the precision's unit roundoff, and a reference that is not all zero.  Prints and returns the ratio."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    q = fam.excess(got, ref, absref, nq, unit_roundoff(dtype_name), factor=factor)
    print(f"{what}: {fam.name} {nq} {dtype_name}: max |err| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0, (what, fam.name, nq, dtype_name, q)
    assert float(np.max(np.abs(ref))) > 0, (what, fam.name, nq)
    return q


class Banded:
    """A view of `n` scalars at `off` scalars into a line of a line-aligned buffer, `lines` 128-byte lines of `fill` on
    either side."""

    def __init__(self, torch_mod, dtype, n, off, fill, lines=2, device="cuda"):
        line = 128 // torch_mod.empty(0, dtype=dtype).element_size()
        self.fill, self.lo, self.hi = fill, lines * line + off, lines * line + off + n
        self.buf = torch_mod.empty(self.hi + lines * line, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 128 == 0 or not self.buf.is_cuda
        self.reset()
        self.view = self.buf[self.lo:self.hi]

    @classmethod
    def of(cls, torch_mod, t, fill=float("nan"), lines=4):
        """A copy of the tensor `t` between bands, on its device."""
        b = cls(torch_mod, t.dtype, t.numel(), 0, fill, lines, t.device)
        b.view.copy_(t.reshape(-1))
        return b

    def reset(self):
        self.buf.fill_(self.fill)

    def bands_intact(self, torch_mod):
        bands = torch_mod.cat([self.buf[:self.lo], self.buf[self.hi:]])
        return bool(torch_mod.isnan(bands).all()) if self.fill != self.fill else bool((bands == self.fill).all())


@pytest.fixture(scope="module")
def sf():
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a GPU"
    return torch


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
