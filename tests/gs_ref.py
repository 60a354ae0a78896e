"""Reference and map builders of the gather-scatter calls (include/sumfact.h sf_gs_setup, sf_global_to_local_*,
sf_assemble_*, sf_gs_*) for tests/test_gs_cpu.py, tests/test_gpu_gs.py and tools/gs_bench.py.  Imports nothing of the
product.

With Q the nlocal x nglobal matrix of a local-to-global map l2g (Q[i][l2g[i]] = sign[i], a negative l2g[i] an empty row):

    global_to_local = Q,     assemble = Q^T,     gs = Q Q^T  (in place, rows of Q with no or one partner left alone)

assemble adds the terms of a global degree of freedom in ascending local index, one rounding per addition: that is what
np.add.at does (ufunc.at is unbuffered and walks the indices in order), in the dtype of the values.  sign * x is exact, so
the references are exact restatements: the GPU results are compared with np.array_equal, no tolerance.
"""
import numpy as np


def ref_assemble(l2g, nglobal, local, sign=None):
    l2g, local = np.asarray(l2g), np.asarray(local)
    v = local if sign is None else np.asarray(sign) * local
    out = np.zeros(nglobal, dtype=local.dtype)
    valid = l2g >= 0
    np.add.at(out, l2g[valid], v[valid])
    return out


def ref_global_to_local(l2g, glob, sign=None):
    l2g, glob = np.asarray(l2g), np.asarray(glob)
    valid = l2g >= 0
    out = np.zeros(l2g.size, dtype=glob.dtype)
    out[valid] = glob[l2g[valid]]
    return out if sign is None else (np.asarray(sign) * out).astype(glob.dtype)


def multiplicity(l2g, nglobal):
    l2g = np.asarray(l2g)
    return np.bincount(l2g[l2g >= 0], minlength=nglobal)


def shared(l2g, nglobal):
    """Mask of the local coefficients that gs changes: mapped, and not alone on their global degree of freedom."""
    l2g = np.asarray(l2g)
    out = np.zeros(l2g.size, dtype=bool)
    valid = l2g >= 0
    out[valid] = multiplicity(l2g, nglobal)[l2g[valid]] >= 2
    return out


def ref_gs(l2g, nglobal, local, sign=None):
    local = np.asarray(local)
    both = ref_global_to_local(l2g, ref_assemble(l2g, nglobal, local, sign), sign)
    return np.where(shared(l2g, nglobal), both, local)


def structured_map(nel, nm):
    """(l2g int32, nglobal) of a structured mesh of nel = (nx, ny[, nz]) elements with nm modes per direction and element
    that share their end modes with the neighbours: local numbering element-major ([ez][ey][ex][k][j][i], i fastest),
    global numbering lexicographic over the nel_d (nm - 1) + 1 nodes per direction (x fastest).  An interior vertex
    belongs to 4 elements in 2D and 8 in 3D."""
    nel = tuple(int(n) for n in nel)
    dim = len(nel)
    assert dim in (2, 3) and nm >= 2
    npts = [n * (nm - 1) + 1 for n in nel]
    nglobal = int(np.prod(npts))
    assert nglobal < 2 ** 31
    node = [(np.arange(n, dtype=np.int32)[:, None] * np.int32(nm - 1) + np.arange(nm, dtype=np.int32)[None, :])
            for n in nel]
    stride = [np.int32(1), np.int32(npts[0]), np.int32(npts[0] * npts[1])]
    if dim == 2:
        g = (node[1] * stride[1])[:, None, :, None] + node[0][None, :, None, :]                     # [ey][ex][j][i]
    else:
        g = ((node[2] * stride[2])[:, None, None, :, None, None] + (node[1] * stride[1])[None, :, None, None, :, None]
             + node[0][None, None, :, None, None, :])                                               # [ez][ey][ex][k][j][i]
    return np.ascontiguousarray(g, dtype=np.int32).reshape(-1), nglobal


def random_map(nlocal, nglobal, seed, empty_share=0.0, negative_share=0.0, long_row=0):
    """l2g int32: every entry drawn from the global degrees of freedom that are not left empty (a share `empty_share` of
    them is), a share `negative_share` of the entries negative, and -- long_row > 0 -- long_row entries at random places
    moved to one row."""
    rng = np.random.default_rng(seed)
    used = np.flatnonzero(rng.random(nglobal) >= empty_share)
    if used.size == 0:
        used = np.array([nglobal // 2])
    l2g = rng.choice(used, size=nlocal).astype(np.int32)
    l2g[rng.random(nlocal) < negative_share] = -1 - rng.integers(0, 5)
    if long_row:
        assert long_row <= nlocal
        l2g[rng.choice(nlocal, size=long_row, replace=False)] = used[used.size // 2]
    return l2g


def random_sign(n, seed, dtype):
    return np.where(np.random.default_rng(seed).random(n) < 0.5, -1.0, 1.0).astype(dtype)
