"""What the GPU tests of the multi-field families (sf_advect_*, sf_aff_advect_*, sf_vecgrad_*, sf_geom_*) share, written
once: bit comparison of tensors, sequences and dicts of outputs (bits, planes, leaves, same_bits), 256-byte aligned rows
(rows), case IDs (ids, _params), the 8-byte-only aligned copy (odd), the stream-capture idiom every capture test of tests/
uses (capture_replay), and MultiField, the adapter over which tests/test_gpu_multifield_common.py and its child process
tests/multifield_first_call.py are written.  Each family's adapter is FAMILY in its tests/<family>_families.py.
"""
from collections import namedtuple

import pytest

from fused_families import F32, F64, case_id


def ids(cases):
    return [case_id(s) + "-" + str(n) for s, n in cases]


def _params(names, cases, tail=lambda c: "-".join(case_id(v) for v in c[1:])):
    """parametrize over (family, values ...) tuples; the ID: the family, then the ID the values had in its own file."""
    cases = list(cases)
    labels = ["-".join(filter(None, (c[0].name, tail(c)))) for c in cases]
    return pytest.mark.parametrize(names, cases if "," in names else [c[0] for c in cases], ids=labels)


def bits(torch_mod, t):
    """The tensor as integers: equal bits, NaN included."""
    return t.view(torch_mod.int64 if t.dtype == torch_mod.float64 else torch_mod.int32)


def planes(v):
    """An output as a list of flat tensors: the rows of a (parts, n) tensor or of a tuple of rows, else the tensor itself."""
    if isinstance(v, (tuple, list)):
        return list(v)
    return [v[r] for r in range(v.shape[0])] if v.dim() == 2 else [v]


def leaves(v):
    """The tensors of a result: the values of a dict (a tuple of rows counts row by row), the items of a sequence, or the
    tensor itself."""
    if isinstance(v, dict):
        return [t for x in v.values() for t in (x if isinstance(x, (tuple, list)) else [x])]
    return list(v) if isinstance(v, (tuple, list)) else [v]


def same_bits(torch_mod, a, b):
    """The same bits, NaN included, in the same shapes: two tensors, two sequences of tensors of one length, or two dicts
    with the same keys whose values are tensors or row tuples (a tuple of rows equals the (parts, n) tensor of them)."""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and all(
            same_bits(torch_mod, planes(a[k]), planes(b[k])) for k in a)
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        a, b = planes(a), planes(b)
        return len(a) == len(b) and all(same_bits(torch_mod, x, y) for x, y in zip(a, b))
    return a.shape == b.shape and bool(torch_mod.equal(bits(torch_mod, a), bits(torch_mod, b)))


def rows(torch_mod, parts, n, dtype, fill=None):
    """A (parts, n) tensor whose rows each start 256-byte aligned, as the multi-field operators return theirs."""
    per = 256 // torch_mod.empty(0, dtype=dtype).element_size()
    buf = torch_mod.empty((parts, (n + per - 1) // per * per), dtype=dtype, device="cuda")
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :n]


def odd(torch_mod, t):
    """A copy of `t` at an odd scalar offset of a fresh buffer: 8-byte aligned only."""
    buf = torch_mod.empty(t.numel() + 3, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 8
    return v


def capture_replay(torch_mod, call):
    """call(side) captured into a graph on a side stream that waits for the current one, replayed once on the current
    stream and waited for."""
    torch_mod.cuda.synchronize()
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            call(side)
    torch_mod.cuda.current_stream().wait_stream(side)
    g.replay()
    torch_mod.cuda.synchronize()


MultiField = namedtuple("MultiField", [
    "name",             # the ID prefix of the family's cases, and the argument of tests/multifield_first_call.py
    "problem",          # the class: problem(sf, torch_mod, nq, nelmt, dtype_name, seed) with .run(**mode) and .check()
    "graph",            # (nq, nelmt) of test_captured_graph_replay_matches_eager
    "graph_modes",      # the keyword arguments of run() it iterates; the outputs of the last are held to the bound ...
    "graph_check",      # ... by check(out, "graph", elements=..., **graph_check)
    "zeros",            # zeros(p, **mode): a zeroed `out` of run(**mode), allocated without running anything
    "first_call",       # (nq, nelmt) of the child process, one per route
    "first_modes",      # the keyword arguments of run() it iterates on each
    "first_also",       # None, or first_also(p, out, **mode): what else the first call's result must satisfy
    "first_tail",       # None, or first_tail(torch_mod, problems): further first calls once every route has run
    "first_eager",      # whether the child also has the "eager" mode: the first calls made outside a capture
    "streams",          # the two (nq, nelmt) of test_two_streams_in_flight
    "stream_sample",    # the seeded sample's size
    "stream_seed",      # stream_seed(k, nelmt): the seed of job k
    "streams_differ",   # whether the two jobs' results must differ in bits
    "refused",          # (nq, nelmt, dtype_name, variant) that answer SF_ENOTBUILT ...
    "refused_calls",    # ... in every call of refused_calls(p, variant), a list of functions of no argument
])


# the refused table of sf_advect_*, sf_aff_advect_* and sf_vecgrad_*: "wave" off the table, extents beyond the fallback's
# bounds, variants without a kernel of the family
NOT_BUILT = tuple((nq, 3, F64, variant) for nq, variant in (
    ((9, 9, 9), "wave"), ((6, 6, 12), "wave"), ((13, 2, 2), "auto"), ((33, 2), "auto"), ((13, 2, 2), "generic"),
    ((8, 8, 8), "mfma"), ((8, 8), "thread"))) + (((13, 2, 2), 3, F32, "auto"),)


def families():
    """The adapters, in the order the families were added."""
    import advect_families
    import affine_advect_families
    import geom_families
    import vecgrad_families
    return [m.FAMILY for m in (geom_families, advect_families, affine_advect_families, vecgrad_families)]
