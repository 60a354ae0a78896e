"""The geometric-factor family (sf_geom_*, sf_geom_affine_*) for tests/test_gpu_geom.py, in the pattern of
tests/fused_families.py and tests/affine_deriv_families.py: the literals of the cases, GeomProblem (the data of one case on
the device, its runs, its reference and its checks) and FAMILY, the family's adapter for the tests written once in
tests/test_gpu_multifield_common.py (refusals, stream capture, the first call of a process inside a capture, two streams
in flight).  The helpers it shares with the other multi-field families are tests/multifield_common.py.

The Family adapter itself does not fit: this family has d inputs and up to four outputs of different lengths, each with
a bound of its own that is a running error bound (tests/geom_ref.py GeomRef), not gamma_N absref.  What fits is kept:
prepare() gives the coordinates -- deformed elements of geom_ref.deformed(), never raw random fills, whose Jacobians
would be singular somewhere -- the seeds and the guard bands (fused_families.Banded).

Operands.  bases / derivs / qws: the Legendre modal basis at the Gauss-Lobatto points, its differentiation matrix and
weights (geom_ref.gll_operands), rounded to the working precision; the reference is computed on the rounded values the
device holds.
"""
import numpy as np

from fused_families import F32, NO_KERNEL, _refused, to_host
from geom_ref import AFFINE_OUTPUTS, OUTPUTS, deformed, gll_operands, ref_geom, sizes, unit_roundoff
from multifield_common import MultiField, bits, same_bits  # noqa: F401

WAVE_3D = (((2, 2, 2), 33), ((3, 3, 3), 1001), ((5, 5, 5), 67), ((6, 6, 6), 129), ((8, 8, 8), 65))
WAVE_2D = (((5, 5), 4099), ((16, 16), 127))
FALLBACK = (((6, 6, 12), 13), ((9, 9, 9), 15), ((23, 5), 14))
SUBSETS = (((3, 3, 3), 1001), ((5, 5), 4099))
REFUSED = _refused((((9, 9, 9),), 5, NO_KERNEL), (((6, 6, 12), (17, 17), (4, 9)), 5, ("wave",)),
                   (((8, 8),), 5, ("mfma", "thread")), (((13, 4, 4),), 2, ("auto",)), (((4, 4, 13),), 3, ("generic",)),
                   (((33, 5), (5, 33)), 3, ("auto",))) + (((13, 4, 4), 3, F32, "auto"),)
GRAPH = (((8, 8, 8), 2003), ((9, 9), 5003), ((6, 6, 12), 301), ((3, 3, 3), 1001))
FIRST_CALL = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
STREAMS, STREAM_SAMPLE = (((7, 7, 7), 3011), ((12, 12), 10003)), 64


def condition_limit(nq, dtype_name):
    """The limit on e(det) / |det| that the reference asserts: 2^-10 (geom_ref.py), with TWO exceptions, both float32.
    At (8, 8, 8) and (16, 16) the prescribed inputs cannot meet it in float32: e(J) = gamma_N(2^-24) absJ with the GLL
    differentiation matrix (entries up to 60 at 16 points) gives e(det) / |det| = 1.03e-3 and 2.55e-3 on these elements
    against 2^-10 = 0.98e-3; the figures that led to 2^-10 were taken in fp64.  The condition exists so that the
    second-order terms stay inside the factor 2 of the assertion: they are at most the sum of the relative errors of the
    factors of a value (fewer than ten of them, each at most a few times e(det) / |det|) times the first-order bound, so
    2^-8 = 3.9e-3 leaves them below a tenth of it.  The assertion on the outputs, |got - ref| <= 2 e, is the same
    everywhere."""
    return 2.0 ** -8 if (tuple(nq), dtype_name) in (((8, 8, 8), F32), ((16, 16), F32)) else 2.0 ** -10


def per_element(nq):
    """Scalars per element of every output."""
    d, nqt = len(nq), sizes(nq)[1]
    return {"df": d * d * nqt, "w": nqt, "g": d * (d + 1) // 2 * nqt, "detj": nqt, "dfe": d * d, "ge": d * (d + 1) // 2,
            "je": 1}


class GeomProblem:
    """One case on the device.  prepare() is the hook of the family: it fills .xs, the (d, n) coordinates."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed, affine=False):
        self.sf, self.torch, self.nq, self.nelmt, self.dtype_name = sf, torch_mod, tuple(nq), nelmt, dtype_name
        self.dtype, self.seed, self.affine = getattr(torch_mod, dtype_name), seed, affine
        self.d, self.per = len(nq), per_element(self.nq)
        dev = lambda a: torch_mod.tensor(np.asarray(a), dtype=self.dtype, device="cuda")      # noqa: E731
        self.bs, self.ds, self.qs = ([dev(v) for v in vs] for vs in gll_operands(self.nq))
        self.prepare()
        self._refs = {}

    def prepare(self):
        xs, self.A = deformed(self.nq, self.nelmt, 1000 + self.seed, affine=self.affine)
        n = xs[0].size
        pad = -n % 64                                               # rows 256-byte aligned, as physderiv_* returns them
        buf = self.torch.zeros((self.d, n + pad), dtype=self.dtype, device="cuda")
        for a in range(self.d):
            buf[a, :n] = self.torch.tensor(xs[a], dtype=self.dtype, device="cuda")
        self.xs = buf[:, :n]

    def prefix(self, n):
        """The problem of the first n elements: views of the same arrays."""
        import copy
        q = copy.copy(self)
        q.nelmt, q.xs, q._refs = n, self.xs[:, :n * sizes(self.nq)[0]], {}
        return q

    def run(self, outputs=OUTPUTS, out=None, variant="auto", xs=None, stream=None):
        """geom_hex / geom_quad: the dict of the outputs asked for."""
        fn = self.sf.geom_hex if self.d == 3 else self.sf.geom_quad
        return fn(self.nq, *self.bs, *self.ds, *self.qs, self.xs if xs is None else xs, outputs=outputs, out=out,
                  variant=variant, stream=stream)

    def run_affine(self, xs=None, stream=None):
        fn = self.sf.geom_affine_hex if self.d == 3 else self.sf.geom_affine_quad
        return dict(zip(AFFINE_OUTPUTS, fn(self.nq, *self.bs, *self.ds, self.xs if xs is None else xs, stream=stream)))

    def host_operands(self):
        return [[to_host(t).astype(np.float64) for t in v] for v in (self.bs, self.ds, self.qs)]

    def reference(self, elements=None, affine=False, xs=None):
        """GeomRef on what the device holds (of the elements `elements` only); the condition is asserted inside."""
        key = (None if elements is None else tuple(int(e) for e in elements), affine, xs is None)
        if key not in self._refs or xs is not None:
            B, D, Q = self.host_operands()
            src = self.xs if xs is None else xs
            rows = [to_host(src[a]).astype(np.float64).reshape(self.nelmt, -1) for a in range(self.d)]
            n = self.nelmt
            if elements is not None:
                rows, n = [r[np.asarray(elements)] for r in rows], len(elements)
            ref = ref_geom(self.nq, n, B, D, Q, [r.reshape(-1) for r in rows], unit_roundoff(self.dtype_name), affine=affine,
                           limit=condition_limit(self.nq, self.dtype_name))
            if xs is not None:
                return ref
            self._refs[key] = ref
        return self._refs[key]

    def check(self, got, what, elements=None, affine=False, ref=None):
        """Every output in `got` within 2 e of the long-double reference, elementwise; prints each figure first."""
        ref = self.reference(elements, affine) if ref is None else ref
        for name, t in got.items():
            host = to_host(t).reshape(self.nelmt, -1)
            if elements is not None:
                host = host[np.asarray(elements)]
            q = ref.excess(name, host)
            print(f"{what}: geom {self.nq} {self.dtype_name} nelmt={self.nelmt} {name}: max |err| / (2 e) = {q:.3g}")
            assert q <= 1.0, (what, self.nq, self.dtype_name, name, q)
            assert float(np.max(np.abs(ref.val[name]))) > 0, (what, name)


def zeros(p, outputs=OUTPUTS):
    """A zeroed `out` of p.run(outputs)."""
    return {k: p.torch.zeros(p.nelmt * p.per[k], dtype=p.dtype, device="cuda") for k in outputs}


def refused_calls(p, variant):
    """The deformed call; under AUTO the affine form too, which has the fallback's bounds."""
    return [lambda: p.run(variant=variant)] + ([p.run_affine] if variant == "auto" else [])


def first_affine(torch_mod, problems):
    """The affine kernel allocates its own outputs: its first call is captured through the C call's wrapper on a private
    memory pool."""
    p = problems[0]
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    graph = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(graph, stream=side):
            got = p.run_affine(stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch_mod.cuda.synchronize()
    eager = p.run_affine()
    torch_mod.cuda.synchronize()
    assert same_bits(torch_mod, got, eager) and float(got["je"].min()) > 0


FAMILY = MultiField(
    name="geom", problem=GeomProblem, graph=GRAPH, graph_modes=tuple({"outputs": o} for o in (OUTPUTS, ("df",), ("g", "w"))),
    graph_check={}, zeros=zeros, first_call=FIRST_CALL, first_modes=({"outputs": OUTPUTS},), first_also=None,
    first_tail=first_affine, first_eager=False, streams=STREAMS, stream_sample=STREAM_SAMPLE,
    stream_seed=lambda k, nelmt: nelmt % 97, streams_differ=False, refused=REFUSED, refused_calls=refused_calls)
