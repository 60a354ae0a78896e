"""The vector-gradient family (sf_vecgrad_*) for tests/test_gpu_vecgrad.py, in the pattern of tests/advect_families.py: the
literals of the cases, VecgradProblem (the data of one case on the device, its runs, its reference and its checks) and
FAMILY, the family's adapter for the tests written once in tests/test_gpu_multifield_common.py.  Outputs are compared
with multifield_common.same_bits: dicts with the same keys and the same bits, a curl as a (3, n) tensor or as three rows.

The Family adapter of tests/fused_families.py does not fit: this family has d inputs and up to three outputs of
different lengths, each with a count of its own in its bound.  What fits is kept: the seeded per-value-distinct data of
sf.fill_random (U[-1, 1): every coefficient with both signs), the element-major layout (the first n elements of a
problem are a problem of n elements: a reference computed once serves its prefixes), the guard bands
(fused_families.Banded), the fixtures and RAGGED.
"""
import itertools

import numpy as np

from fused_families import F32, F64, RAGGED, Banded, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from multifield_common import NOT_BUILT, MultiField, ids, planes, rows, same_bits  # noqa: F401
from vecgrad_ref import OUTPUTS, output_excess, ref_vecgrad, unit_roundoff

WAVE_ORDERS = [(q,) * 3 for q in range(2, 9)] + [(q,) * 2 for q in range(2, 17)]
WAVE_COUNT = 403
RAGGED_BOUND = 257
PHYSDERIV = (((3, 3, 3), 1001), ((7, 7, 7), 257), ((8, 8, 8), 65), ((5, 5), 4099), ((16, 16), 127))
SUBSET_SHAPES = (((8, 8, 8), 65), ((13, 13), 1000))
SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(OUTPUTS, r)]
FALLBACK = (((6, 6, 12), 13), ((9, 9, 9), 15), ((12, 12, 12), 5), ((23, 5), 14), ((32, 32), 3))
GUARD = (((3, 3, 3), 1001), ((8, 8, 8), 65), ((2, 2, 2), 33), ((13, 13), 1000), ((6, 6, 12), 13))
POISON = (((2, 2, 2), 33), ((5, 5, 5), 130), ((8, 8), 259))
GRAPH = (((8, 8, 8), 2003), ((9, 9), 5003))
FIRST_CALL = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
STREAMS, STREAM_SAMPLE = (((7, 7, 7), 3001), ((7, 7, 7), 3001)), 64
END_TO_END = (((5, 5, 5), 101), ((9, 9), 101))
MISALIGNED = (((4, 4, 4), 130), ((8, 8, 8), 65), ((9, 9), 259))


def banded_outputs(torch_mod, p, names, n, guard):
    """(out, bands): the `out` dict of vecgrad_* over the outputs `names` of n elements, every flat piece between guard
    words."""
    per, ncurl = per_element(p.nq)
    out, bands = {}, []
    for name in names:
        pieces = [Banded(torch_mod, p.dtype, n * per[name], 0, guard, lines=4) for _ in range(ncurl if name == "curl" else 1)]
        bands += pieces
        out[name] = [b.view for b in pieces] if len(pieces) > 1 else pieces[0].view
    return out, bands


def per_element(nq):
    """Scalars per element of "grad", "div" and of one plane of "curl"; the planes of the curl."""
    d, nqt = len(nq), sizes(nq)[1]
    return {"grad": d * d * nqt, "div": nqt, "curl": nqt}, d * (d - 1) // 2


def host_outputs(got, nelmt, elements=None):
    """The outputs as host arrays in the shapes of vecgrad_ref; of the elements `elements` only."""
    out = {}
    for name, t in got.items():
        if isinstance(t, (tuple, list)) or t.dim() == 2:
            h = np.stack([to_host(r).reshape(nelmt, -1) for r in t])
            out[name] = (h if elements is None else h[:, np.asarray(elements)]).reshape(h.shape[0], -1)
        else:
            h = to_host(t).reshape(nelmt, -1)
            out[name] = (h if elements is None else h[np.asarray(elements)]).reshape(-1)
    return out


class VecgradProblem:
    """One case on the device: bases, derivative matrices, df and d fields of modes, every array seeded and
    element-major."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        self.sf, self.torch, self.nq, self.nelmt, self.dtype_name = sf, torch_mod, tuple(nq), nelmt, dtype_name
        self.dtype, self.seed, self.d = getattr(torch_mod, dtype_name), seed, len(nq)
        self.nmt, self.nqt = sizes(self.nq)[:2]
        d, fill = self.d, lambda n, s: sf.fill_random(n, s + 13 * seed, dtype=self.dtype)
        self.bs = [fill((q - 1) * q, 500 + a) for a, q in enumerate(self.nq)]
        self.ds = [fill(q * q, 600 + a) for a, q in enumerate(self.nq)]
        self.df = fill(nelmt * d * d * self.nqt, 11)
        self.x = rows(torch_mod, d, nelmt * self.nmt, self.dtype)
        for a in range(d):
            self.x[a].copy_(fill(nelmt * self.nmt, 30 + a))
        self._ref = None

    def fn(self):
        return self.sf.vecgrad_hex if self.d == 3 else self.sf.vecgrad_quad

    def run(self, n=None, outputs=OUTPUTS, variant="auto", out=None, stream=None, **over):
        """vecgrad_* on the first n elements.  over: bs, ds, df, x in the place of the problem's (already cut to n)."""
        n = self.nelmt if n is None else n
        return self.fn()(self.nq, *over.get("bs", self.bs), *over.get("ds", self.ds),
                         over.get("df", self.df[:n * self.d * self.d * self.nqt]), over.get("x", self.x[:, :n * self.nmt]),
                         outputs=outputs, out=out, variant=variant, stream=stream)

    def physderiv(self, a, n=None, variant="auto"):
        """sf_physderiv_* on field a: the (d, n nq^d) tensor of its outputs."""
        n = self.nelmt if n is None else n
        fn = self.sf.physderiv_hex if self.d == 3 else self.sf.physderiv_quad
        return fn(self.nq, *self.bs, *self.ds, self.df[:n * self.d * self.d * self.nqt], self.x[a, :n * self.nmt],
                  variant=variant)

    def reference(self, elements=None, **over):
        """(ref, absref) in long double on what the device holds: of every element (cached), or of `elements`."""
        if elements is None and not over and self._ref is not None:
            return self._ref
        d, nqt, nmt = self.d, self.nqt, self.nmt
        pick = (lambda t, per: to_host(t).reshape(self.nelmt, per)) if elements is None else \
               (lambda t, per: to_host(t).reshape(self.nelmt, per)[np.asarray(elements)])
        n = self.nelmt if elements is None else len(elements)
        x = over.get("x", self.x)
        ref = ref_vecgrad(self.nq, n, [to_host(b) for b in self.bs], [to_host(t) for t in self.ds],
                          pick(over.get("df", self.df), d * d * nqt).reshape(-1), [pick(x[a], nmt).reshape(-1) for a in range(d)])
        if elements is None and not over:
            self._ref = ref
        return ref

    def check(self, got, what, n=None, elements=None, ref=None):
        """Every output of `got` within gamma_N absref of the long-double reference, elementwise, each with its own N;
        prints each figure first."""
        n = self.nelmt if n is None else n
        ref, absref = self.reference(elements) if ref is None else ref
        host = host_outputs(got, n, elements)
        per, _ = per_element(self.nq)
        worst = 0.0
        for name, h in host.items():
            r, a = ref[name], absref[name]
            if elements is None:
                r, a = r[..., :n * per[name]], a[..., :n * per[name]]
            assert h.shape == r.shape, (name, h.shape, r.shape)
            q = output_excess(h, r, a, self.nq, unit_roundoff(self.dtype_name), name)
            print(f"{what}: vecgrad {self.nq} {self.dtype_name} nelmt={n} {name}: max |err| / (gamma_N absref) = {q:.3g}")
            assert q <= 1.0, (what, self.nq, self.dtype_name, name, q)
            assert float(np.max(np.abs(r))) > 0, (what, self.nq, name)
            worst = max(worst, q)
        return worst


def zeros(p, outputs=OUTPUTS, **_):
    """A zeroed `out` of p.run(outputs=outputs)."""
    return banded_outputs(p.torch, p, outputs, p.nelmt, 0.0)[0]


def refused_calls(p, variant):
    """With every output and with one in float64; the float32 case with every output."""
    return [lambda o=o: p.run(outputs=o, variant=variant) for o in ((OUTPUTS, ("div",)) if p.dtype_name == F64 else (OUTPUTS,))]


FAMILY = MultiField(
    name="vecgrad", problem=VecgradProblem, graph=GRAPH, graph_modes=({"outputs": OUTPUTS}, {"outputs": ("div", "curl")}),
    graph_check={}, zeros=zeros, first_call=FIRST_CALL, first_modes=({"outputs": OUTPUTS},), first_also=None, first_tail=None,
    first_eager=False, streams=STREAMS, stream_sample=STREAM_SAMPLE, stream_seed=lambda k, nelmt: 40 + k, streams_differ=True,
    refused=NOT_BUILT, refused_calls=refused_calls)
