"""The affine advection family (sf_aff_advect_*) for tests/test_gpu_affine_advect.py, in the pattern of
tests/advect_families.py, whose literals, helpers and AdvectProblem it takes over: AffineAdvectProblem is an AdvectProblem
(the same seeded operands, the same check) whose df and w are the planes EXPANDED on the device from dfe, je and the
quadrature weights (df[e][c][pt] = dfe[e][c]; w = je * (qw2 * (qw1 * qw0)) in the working precision, each product rounded
once, in exactly that association), so that the inherited run() is the deformed call that the affine one must equal bit
for bit.  FAMILY is the family's adapter for the tests written once in tests/test_gpu_multifield_common.py.
"""
import ctypes
import functools

import numpy as np

from advect_families import (FALLBACK, GRAPH, GUARD, MISALIGNED, POISON, RAGGED_BOUND, SCALAR, STREAM_SAMPLE,  # noqa: F401
                             STREAMS, WAVE_COUNT, WAVE_ORDERS, AdvectProblem, refused_calls, zeros)
from affine_advect_ref import affine_advect_excess, ref_affine_advect
from fused_families import to_host
from multifield_common import NOT_BUILT, MultiField, ids, rows, same_bits  # noqa: F401

NO_JE = (((3, 3, 3), 257), ((7, 7, 7), 257), ((8, 8, 8), 257), ((5, 5), 257), ((16, 16), 257))
FIRST_CALL = (((8, 8, 8), 1001), ((6, 6, 12), 101), ((9, 9), 1002), ((23, 5), 101))
END_TO_END = (((5, 5, 5), 101), ((9, 9), 101))
OWN = object()                                     # "the problem's own je": None means the call without a weight


class AffineAdvectProblem(AdvectProblem):
    """One case on the device: what AdvectProblem holds (the same seeds for the bases, derivative matrices, c and the
    fields), the quadrature weights, dfe and je, and df, w expanded from them."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        super().__init__(sf, torch_mod, nq, nelmt, dtype_name, seed)
        self._aref = {}

    def fill_geometry(self, fill):
        self.qs = [fill(q, 700 + a) for a, q in enumerate(self.nq)]
        self.dfe, self.je = fill(self.nelmt * self.d * self.d, 11), fill(self.nelmt, 12)
        self.df, self.w = self.expand(self.dfe, self.je)

    def expand(self, dfe, je):
        """(df, w) of sf_advect_* on the device; w a plane of ones when je is None."""
        n, d, nqt = dfe.numel() // (self.d * self.d), self.d, self.nqt
        df = dfe.reshape(n, d * d, 1).expand(n, d * d, nqt).contiguous().reshape(-1)
        if je is None:
            return df, self.torch.ones(n * nqt, dtype=self.dtype, device="cuda")
        q = self.qs[0]
        for t in self.qs[1:]:
            q = t.reshape(-1, *([1] * q.dim())) * q.unsqueeze(0)                      # qw2 * (qw1 * qw0)
        return df, (je.reshape(n, 1) * q.reshape(1, nqt)).reshape(-1)

    def fn_affine(self):
        return self.sf.affine_advect_hex if self.d == 3 else self.sf.affine_advect_quad

    def deformed(self, n=None, field=None, variant="auto", je=OWN):
        """sf_advect_* on the expanded planes of the first n elements (je=None: w a plane of ones)."""
        n = self.nelmt if n is None else n
        over = {} if je is OWN else {"w": self.expand(self.dfe[:n * self.d * self.d], je)[1]}
        return AdvectProblem.run(self, n, field=field, variant=variant, **over)

    def run(self, n=None, nf=None, field=None, variant="auto", out=None, stream=None, je=OWN, **over):
        """affine_advect_* on the first n elements: all d fields (nf = d), or the one field `field` (nf = 1).  over: bs, ds,
        qs, dfe, c, x in the place of the problem's (already cut to n elements); je: OWN, a tensor or None."""
        n = self.nelmt if n is None else n
        nf = self.d if nf is None and field is None else (1 if nf is None else nf)
        d, nqt, nmt = self.d, self.nqt, self.nmt
        x = over.get("x")
        if x is None:
            x = self.x[:, :n * nmt] if nf == d else self.x[field if field is not None else 0, :n * nmt]
        return self.fn_affine()(self.nq, *over.get("bs", self.bs), *over.get("ds", self.ds), *over.get("qs", self.qs),
                                over.get("dfe", self.dfe[:n * d * d]), self.je[:n] if je is OWN else je,
                                over.get("c", self.c[:, :n * nqt]), x, out=out, variant=variant, stream=stream)

    def raw(self, nf, qs, dfe, je, cs, ins, outs, variant="auto", n=None):
        """The C entry point with every slot as given (None: NULL); float32 has no variant argument."""
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        f32 = self.dtype_name == "float32"
        assert not f32 or variant == "auto"
        fn = getattr(self.sf.capi.lib(), f"sf_aff_advect_{'hex' if self.d == 3 else 'quad'}_{'f32' if f32 else 'f64_variant'}")
        head = () if f32 else (self.sf.VARIANTS[variant],)
        return fn(*head, *self.nq, self.nelmt if n is None else n, nf, *(ptr(t) for t in self.bs), *(ptr(t) for t in self.ds),
                  *(ptr(t) for t in qs), ptr(dfe), ptr(je), *(ptr(t) for t in cs), *(ptr(t) for t in ins),
                  *(ptr(t) for t in outs), ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream))

    def reference(self, elements=None, fields=None, je=OWN):
        """(ref, absref) of the affine operator in long double on what the device holds: of every element (cached per je
        given / None), or of `elements`."""
        with_je = je is not None
        whole = elements is None and fields is None
        if whole and with_je in self._aref:
            return self._aref[with_je]
        d, nqt, nmt = self.d, self.nqt, self.nmt
        pick = (lambda t, per: to_host(t).reshape(self.nelmt, per)) if elements is None else \
               (lambda t, per: to_host(t).reshape(self.nelmt, per)[np.asarray(elements)])
        n = self.nelmt if elements is None else len(elements)
        fields = range(d) if fields is None else fields
        ref = ref_affine_advect(self.nq, n, [to_host(b) for b in self.bs], [to_host(t) for t in self.ds],
                                [to_host(t) for t in self.qs], pick(self.dfe, d * d).reshape(-1),
                                pick(self.je, 1).reshape(-1) if with_je else None,
                                [pick(self.c[j], nqt).reshape(-1) for j in range(d)],
                                [pick(self.x[a], nmt).reshape(-1) for a in fields])
        if whole:
            self._aref[with_je] = ref
        return ref

    def check(self, got, what, n=None, elements=None, fields=None, je=OWN):
        """AdvectProblem.check against the affine reference and its bound (with or without je)."""
        return super().check(got, what, n, elements, fields, label="affine advect", je=je,
                             excess=functools.partial(affine_advect_excess, with_je=je is not None))


def first_also(p, out, field=None):
    """The first call's result equals the deformed call on the expanded planes, which runs after it."""
    return same_bits(p.torch, out, p.deformed(field=field))


FAMILY = MultiField(
    name="affine_advect", problem=AffineAdvectProblem, graph=GRAPH,
    graph_modes=({"field": None, "je": OWN}, {"field": None, "je": None}, {"field": 1, "je": OWN}), graph_check={"fields": [1]},
    zeros=zeros, first_call=FIRST_CALL, first_modes=({"field": None}, {"field": 0}), first_also=first_also, first_tail=None,
    first_eager=True, streams=STREAMS, stream_sample=STREAM_SAMPLE, stream_seed=lambda k, nelmt: 40 + k, streams_differ=True,
    refused=NOT_BUILT, refused_calls=refused_calls)
