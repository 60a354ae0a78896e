"""The advection family (sf_advect_*) for tests/test_gpu_advect.py, in the pattern of tests/fused_families.py and
tests/geom_families.py: the literals of the cases, AdvectProblem (the data of one case on the device, its runs, its
reference and its checks) and FAMILY, the family's adapter for the tests written once in
tests/test_gpu_multifield_common.py (stream capture, the first call inside a capture, two streams in flight, the
SF_ENOTBUILT refusals).  The helpers it shares with the other multi-field families are tests/multifield_common.py.

The Family adapter of tests/fused_families.py does not fit: this family has nf = 1 or d inputs AND outputs and d + 2
point operands.  What fits is kept: the seeded per-value-distinct data of sf.fill_random (U[-1, 1): every coefficient
with both signs), the element-major layout (the first n elements of a problem are a problem of n elements: a reference
computed once serves its prefixes), the guard bands (fused_families.Banded), the fixtures and RAGGED.
"""
import numpy as np

from advect_ref import advect_excess, ref_advect, unit_roundoff
from fused_families import F32, F64, RAGGED, Banded, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from multifield_common import NOT_BUILT, MultiField, ids, rows, same_bits  # noqa: F401

WAVE_ORDERS = [(q,) * 3 for q in range(2, 9)] + [(q,) * 2 for q in range(2, 17)]
WAVE_COUNT = 403
RAGGED_BOUND = 257
SCALAR = (((3, 3, 3), 1001), ((7, 7, 7), 257), ((8, 8, 8), 65), ((5, 5), 4099), ((16, 16), 127))
FALLBACK = (((6, 6, 12), 13), ((9, 9, 9), 15), ((12, 12, 12), 5), ((23, 5), 14), ((32, 32), 3))
CHAIN = (((4, 4, 4), 257), ((8, 8, 8), 257), ((12, 12), 257))
GUARD = (((3, 3, 3), 1001), ((8, 8, 8), 65), ((2, 2, 2), 33), ((13, 13), 1000), ((6, 6, 12), 13))
POISON = (((2, 2, 2), 33), ((5, 5, 5), 130), ((8, 8), 259))
GRAPH = (((8, 8, 8), 2003), ((9, 9), 5003))
FIRST_CALL = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
STREAMS, STREAM_SAMPLE = (((7, 7, 7), 3001), ((7, 7, 7), 3001)), 64
END_TO_END = (((5, 5, 5), 101), ((9, 9), 101))
MISALIGNED = (((4, 4, 4), 130), ((8, 8, 8), 65), ((9, 9), 259))


class AdvectProblem:
    """One case on the device: bases, derivative matrices, df, w, c and d fields of modes, every array seeded and
    element-major."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        self.sf, self.torch, self.nq, self.nelmt, self.dtype_name = sf, torch_mod, tuple(nq), nelmt, dtype_name
        self.dtype, self.seed, self.d = getattr(torch_mod, dtype_name), seed, len(nq)
        self.nmt, self.nqt = sizes(self.nq)[:2]
        d, fill = self.d, lambda n, s: sf.fill_random(n, s + 13 * seed, dtype=self.dtype)
        self.bs = [fill((q - 1) * q, 500 + a) for a, q in enumerate(self.nq)]
        self.ds = [fill(q * q, 600 + a) for a, q in enumerate(self.nq)]
        self.fill_geometry(fill)
        self.c = rows(torch_mod, d, nelmt * self.nqt, self.dtype)
        self.x = rows(torch_mod, d, nelmt * self.nmt, self.dtype)
        for a in range(d):
            self.c[a].copy_(fill(nelmt * self.nqt, 20 + a))
            self.x[a].copy_(fill(nelmt * self.nmt, 30 + a))
        self._ref = None

    def fill_geometry(self, fill):
        """df and w, between the matrices and the fields in the order of the fills."""
        self.df = fill(self.nelmt * self.d * self.d * self.nqt, 11)
        self.w = fill(self.nelmt * self.nqt, 12)

    def fn(self):
        return self.sf.advect_hex if self.d == 3 else self.sf.advect_quad

    def run(self, n=None, nf=None, field=None, variant="auto", out=None, stream=None, **over):
        """advect_* on the first n elements: all d fields (nf = d), or the one field `field` (nf = 1).  over: bs, ds, df,
        w, c, x in the place of the problem's (already cut to n elements)."""
        n = self.nelmt if n is None else n
        nf = self.d if nf is None and field is None else (1 if nf is None else nf)
        d, nqt, nmt = self.d, self.nqt, self.nmt
        x = over.get("x")
        if x is None:
            x = self.x[:, :n * nmt] if nf == d else self.x[field if field is not None else 0, :n * nmt]
        return self.fn()(self.nq, *over.get("bs", self.bs), *over.get("ds", self.ds),
                         over.get("df", self.df[:n * d * d * nqt]), over.get("w", self.w[:n * nqt]),
                         over.get("c", self.c[:, :n * nqt]), x, out=out, variant=variant, stream=stream)

    def reference(self, elements=None, fields=None, **over):
        """(ref, absref) in long double on what the device holds: of every element (cached), or of `elements`."""
        if elements is None and fields is None and not over and self._ref is not None:
            return self._ref
        d, nqt, nmt = self.d, self.nqt, self.nmt
        pick = (lambda t, per: to_host(t).reshape(self.nelmt, per)) if elements is None else \
               (lambda t, per: to_host(t).reshape(self.nelmt, per)[np.asarray(elements)])
        n = self.nelmt if elements is None else len(elements)
        fields = range(d) if fields is None else fields
        x = over.get("x", self.x)
        ref = ref_advect(self.nq, n, [to_host(b) for b in self.bs], [to_host(t) for t in self.ds],
                         pick(over.get("df", self.df), d * d * nqt).reshape(-1), pick(over.get("w", self.w), nqt).reshape(-1),
                         [pick(self.c[j], nqt).reshape(-1) for j in range(d)], [pick(x[a], nmt).reshape(-1) for a in fields])
        if elements is None and not over and list(fields) == list(range(d)):
            self._ref = ref
        return ref

    def check(self, got, what, n=None, elements=None, fields=None, ref=None, excess=advect_excess, label="advect", **how):
        """Every out_a of `got` (a (nf, n nm^d) tensor or a tuple of rows) within gamma_N absref of the long-double
        reference (reference(elements, fields, **how)), elementwise; prints the figure first."""
        n = self.nelmt if n is None else n
        ref, absref = self.reference(elements, fields, **how) if ref is None else ref
        host = np.stack([to_host(t).reshape(-1) for t in got])
        if elements is not None:
            host = np.stack([h.reshape(-1, self.nmt)[np.asarray(elements)].reshape(-1) for h in host])
        else:
            ref, absref = ref[:, :n * self.nmt], absref[:, :n * self.nmt]
        assert host.shape == ref.shape, (host.shape, ref.shape)
        q = excess(host, ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {label} {self.nq} {self.dtype_name} nelmt={n}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, q)
        assert float(np.max(np.abs(ref))) > 0, (what, self.nq)
        return q


def zeros(p, field=None, **_):
    """A zeroed `out` of p.run(field=field): d rows, or one."""
    return rows(p.torch, p.d if field is None else 1, p.nelmt * p.nmt, p.dtype, fill=0.0)


def refused_calls(p, variant):
    """With d fields and with one in float64; the float32 case with d."""
    return [lambda f=f: p.run(field=f, variant=variant) for f in ((None, 0) if p.dtype_name == F64 else (None,))]


FAMILY = MultiField(
    name="advect", problem=AdvectProblem, graph=GRAPH, graph_modes=({"field": None}, {"field": 1}),
    graph_check={"fields": [1]}, zeros=zeros, first_call=FIRST_CALL, first_modes=({"field": None}, {"field": 0}),
    first_also=None, first_tail=None, first_eager=False, streams=STREAMS, stream_sample=STREAM_SAMPLE,
    stream_seed=lambda k, nelmt: 40 + k, streams_differ=True, refused=NOT_BUILT, refused_calls=refused_calls)
