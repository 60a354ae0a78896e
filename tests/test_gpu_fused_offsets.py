"""GPU tests of the six fused families at base addresses that are not line-aligned.

The chunk I/O of the wave kernels (chunk_load, chunk_flush, flush_any of csrc/bwdtrans_wave.h; align_shift() and
line_offset(), MEMF bits 2 and 3) changes behaviour with the low address bits of every chunk.  Where a chunk is a whole
number of 128-byte lines, only the base address of the operand sets those bits, and the families' own test files give
the wave kernels line-aligned bases only.  Here every operand of every wave order sits at a chosen offset inside a
128-byte line of a line-aligned buffer:

  * an operand that variant "wave" needs 16-byte aligned (tests/fused_families.py) at 16, 48, 80, 112 and 0 bytes -- 2, 6,
    10, 14 and 0 doubles, 4, 12, 20, 28 and 0 floats -- chosen per operand, so that `in` and `out`, and the d outputs of
    sf_physderiv_*, differ within a case;
  * an operand that needs scalar alignment only at 1, 4, the last scalar of the line, 6 and 0 scalars: an odd scalar, a
    16-byte multiple and the line's end among them; the d inputs of sf_iprodderiv_*, its df and its w all differ.

Five (count, offsets) cases per order and precision, as test_line_alignment_offsets of test_gpu_parity.py has: 5 and 64
elements, and the smallest count from 257 on that fills more than one workgroup of the row and leaves its last chunk
ragged.  The combinations of optional coefficients alternate over the cases.  Every output lies between guard bands of a
sentinel, every input between NaN bands; afterwards the bands are intact, the output is finite and inside the family's
bound of the long-double reference (computed once per order at the largest count: the smaller cases are its prefixes),
and in fp64 the explicit "wave" call is not refused and gives the bits of AUTO.
"""
import pytest

from fused_families import SCALAR, VEC, WAVE_CASES, Banded, Problem, sf, torch_mod, wave_ids, wave_row  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -3.5
VEC_BYTES = (16, 48, 80, 112, 0)


def ragged_count(ec, wpb):
    """The smallest count >= 257 that is more than one workgroup (EC * WPB elements) and no whole number of chunks; with
    one element per chunk, one that is no whole number of workgroups.  At most 1025: the longest row has 1024."""
    n = max(257, ec * wpb + 1)
    while (n % ec == 0) if ec > 1 else (n % wpb == 0):
        n += 1
    assert 257 <= n <= 1031
    return n


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("fam,dim,nq", WAVE_CASES, ids=wave_ids())
def test_line_offsets_of_every_operand(sf, torch_mod, fam, dim, nq, dtype_name):
    ext = (nq,) * dim
    dtype = getattr(torch_mod, dtype_name)
    size = 8 if dtype_name == "float64" else 4
    line = 128 // size
    vec_offs = [b // size for b in VEC_BYTES]
    sca_offs = [1, 4, line - 1, 6, 0]
    big = ragged_count(*wave_row(fam, dim, nq, dtype_name))
    p = Problem(fam, sf, torch_mod, ext, big, dtype_name, nq)
    parts, out_per = fam.out_parts(ext), fam.out_per(ext)
    refs, worst = {}, 0.0
    for i, nelmt in enumerate((big, 64, 5, big, 64)):
        present = fam.modes[i % len(fam.modes)]
        if present not in refs:
            refs[present] = p.reference(present=present)
        ref, absref = (r[:, :nelmt * out_per] for r in refs[present])
        # the k-th 16-byte operand (inputs, then outputs) and the j-th scalar-aligned one take their own offsets
        k = j = 0
        ins, data, offsets = [], {}, []
        for o in p.ops:
            if o.align == VEC:
                off, k = vec_offs[(i + 2 * k) % 5], k + 1
            else:
                off, j = sca_offs[(i + j) % 5], j + 1
            if o.optional and o.name not in present:
                data[o.name] = None
                continue
            b = Banded(torch_mod, dtype, nelmt * o.per, off, float("nan"))
            b.view.copy_(p.data[o.name][:nelmt * o.per])
            assert b.view.data_ptr() % 128 == off * size and (o.align == SCALAR or b.view.data_ptr() % 16 == 0)
            ins.append(b)
            data[o.name] = b.view
            offsets.append((o.name, off))
        outs = []
        for a in range(parts):
            off, k = vec_offs[(i + 2 * k) % 5], k + 1
            outs.append(Banded(torch_mod, dtype, nelmt * out_per, off, SENTINEL))
            offsets.append((f"out{a}", off))
        assert parts == 1 or len({b.lo for b in outs}) == parts          # the d outputs do not share one offset
        what = (fam.name, ext, dtype_name, nelmt, present, offsets)

        def run(variant):
            for b in outs:
                b.reset()
            p.run(sf, data=data, out=[b.view for b in outs], variant=variant)
            torch_mod.cuda.synchronize()
            assert all(b.bands_intact(torch_mod) for b in outs), ("written outside an output", variant) + what
            assert all(b.bands_intact(torch_mod) for b in ins), ("an input's band changed", variant) + what
            assert all(bool(torch_mod.isfinite(b.view).all()) for b in outs), ("not finite", variant) + what
            return [b.view.clone() for b in outs]

        got = run("auto")
        q = p.excess(got, ref, absref)
        worst = max(worst, q)
        assert q <= 1.0, (q,) + what
        if dtype_name == "float64":
            wave = run("wave")                                             # must not be refused
            assert all(torch_mod.equal(g, w) for g, w in zip(got, wave)), what
    print(f"offsets {fam.name} {ext} {dtype_name}: max |err| / (gamma_N absref) = {worst:.3g}")
