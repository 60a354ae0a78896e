"""The parametrised GPU tests that the fused families have in common, written once: install(globals(), family) defines
a family's cases in its own tests/test_gpu_<family>.py under the names and IDs they have always had there, so that a
case's history goes on -- every wave order through AUTO, ragged counts, the any-extent fallback, the explicit variants,
guard values around every output with every input between NaN bands.  The tests with one case per family (refusals,
stream capture, two streams in flight) are tests/test_gpu_fused_common.py.

Each body runs every combination of optional operands the family has (Family.modes; lambda = 0.75 with the mass
coefficient, 0 without) and holds every result to the family's own bound: elementwise |gpu - ref| <= gamma_N absref
against the long-double reference of tests/<family>_ref.py (Problem.check), in fp64 also the bits of the explicit
variant.  The shapes, counts and seeds are the adapter's data (Family.ragged, .fallback, .guard, ...), each family with
the values its own file had; the data is own_problem()'s: the seed scheme of Problem, a definite w for mass, the inputs
of iprodderiv as rows of one array, the tables of diag built once.
"""
import pytest

from fused_families import F32, F64, Banded, case_id, own_problem
from multifield_common import same_bits  # noqa: F401

DTYPES = [F64, F32]


def run(torch_mod, p, sf, **kw):
    got = p.run(sf, **kw)
    torch_mod.cuda.synchronize()
    return got


def _counts_and_modes(fam, sf, torch_mod, nq, dtype_name, counts, seed):
    """(problem, count, optional operands present) of Family.plan(): every count with the full set of operands, and the
    other combinations on the last problem."""
    plan = fam.plan(counts, seed)
    for i, (nelmt, s, counts_of_p) in enumerate(plan):
        p = own_problem(fam, sf, torch_mod, nq, nelmt, dtype_name, s)
        for present in fam.modes if i == len(plan) - 1 else fam.modes[:1]:
            for n in counts_of_p:
                yield p, n, present


def install(ns, fam):
    """Define the family's cases of the common parametrised tests in the namespace `ns` of its test module."""

    @pytest.mark.parametrize("dtype_name", DTYPES)
    @pytest.mark.parametrize("dim,nq", fam.wave_orders, ids=[f"{d}d-nq{n}" for d, n in fam.wave_orders])
    def test_auto_every_wave_order(sf, torch_mod, dim, nq, dtype_name):
        for nelmt in fam.auto_counts(dim, nq):
            p = own_problem(fam, sf, torch_mod, (nq,) * dim, nelmt, dtype_name, nq)
            for present in fam.modes:
                got = run(torch_mod, p, sf, present=present)
                p.check(got, "auto", present=present)
                if dtype_name == F64:
                    # AUTO runs the wave kernel here: the same bits as the explicit variant
                    assert same_bits(torch_mod, got, run(torch_mod, p, sf, present=present, variant="wave"))

    @pytest.mark.parametrize("nq,dtype_name", fam.ragged_shapes, ids=[case_id(s) + "-" + d for s, d in fam.ragged_shapes])
    def test_ragged_counts(sf, torch_mod, nq, dtype_name):
        """The last chunk is partial, or the whole batch is smaller than one chunk or one workgroup; every per-element
        operand and every output ends where the batch ends."""
        for p, n, present in _counts_and_modes(fam, sf, torch_mod, nq, dtype_name, fam.ragged, fam.ragged_seed):
            p.check(run(torch_mod, p, sf, n=n, present=present), "ragged", n, present)

    @pytest.mark.parametrize("dtype_name", DTYPES)
    @pytest.mark.parametrize("nq", fam.fallback, ids=case_id)
    def test_fallback_shapes(sf, torch_mod, nq, dtype_name):
        for p, n, present in _counts_and_modes(fam, sf, torch_mod, nq, dtype_name, fam.fallback_counts, fam.fallback_seed):
            got = run(torch_mod, p, sf, n=n, present=present)
            p.check(got, "fallback", n, present)
            if dtype_name == F64:
                assert same_bits(torch_mod, got, run(torch_mod, p, sf, n=n, present=present, variant="generic"))
                with pytest.raises(sf.capi.SumfactError) as ei:
                    p.run(sf, n=n, present=present, variant="wave")
                assert ei.value.rc == sf.capi.SF_ENOTBUILT

    @pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (9, 9)], ids=case_id)
    def test_explicit_wave_and_generic(sf, torch_mod, nq):
        """Both routes of an order of the table inside the bound of the same reference."""
        p = own_problem(fam, sf, torch_mod, nq, fam.explicit_count, F64, 9)
        for present in fam.modes:
            for variant in ("wave", "generic"):
                p.check(run(torch_mod, p, sf, present=present, variant=variant), variant, present=present)

    @pytest.mark.parametrize("nq", list(fam.guard), ids=case_id)
    def test_guard_bands(sf, torch_mod, nq):
        """Every output sits between two guard bands of 512 bytes (16-byte aligned, so the wave kernels run): only its
        own values change.  Every per-element input, and the small arrays Family.guarded_consts names, are views inside
        buffers filled with NaN on both sides: a value read from outside that reached a result would show as a NaN in
        an output."""
        for dtype_name in DTYPES:
            for nelmt in fam.guard_counts(nq, dtype_name):
                p = own_problem(fam, sf, torch_mod, nq, nelmt, dtype_name, 5)
                ins = {k: Banded.of(torch_mod, v) for k, v in p.window().items()}
                small = {k: [Banded.of(torch_mod, t) for t in p.consts[k]] for k in fam.guarded_consts}
                consts = dict(p.consts, **{k: [b.view for b in v] for k, v in small.items()})
                outs = [Banded.of(torch_mod, t, -3.5) for t in p.run(sf)]
                for present in fam.modes:
                    data = {k: v if v is None else ins[k].view for k, v in p.window(present=present).items()}
                    for b in outs:
                        b.reset()
                    p.run(sf, data=data, consts=consts, out=[b.view for b in outs])
                    torch_mod.cuda.synchronize()
                    what = (fam.name, nq, dtype_name, nelmt, present)
                    assert all(b.bands_intact(torch_mod) for b in outs), ("written outside an output",) + what
                    assert all(b.bands_intact(torch_mod) for b in list(ins.values()) + sum(small.values(), [])), what
                    assert all(bool(torch_mod.isfinite(b.view).all()) for b in outs), ("not finite",) + what
                    p.check([b.view for b in outs], "guard", present=present)

    ns.update(test_auto_every_wave_order=test_auto_every_wave_order, test_fallback_shapes=test_fallback_shapes,
              test_explicit_wave_and_generic=test_explicit_wave_and_generic, **{fam.guard_test: test_guard_bands})
    if fam.ragged_shapes:
        ns.update(test_ragged_counts=test_ragged_counts)
