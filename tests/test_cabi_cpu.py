"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/sumfact.h declares, with no compute call (no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    lib = os.path.join(ROOT, "gpu-benchmarking_amd", "lib", "libsumfact.so")
    if not os.path.exists(lib):
        ge.build()
    return ge.load_package()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(pkg):
    lib = pkg.capi.lib()
    declared = _declared_symbols()
    assert len(declared) >= 16
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/sumfact.h but not exported"
    # and the Python binding covers exactly the header
    assert sorted(pkg.capi.SYMBOLS) == declared


def test_version_and_strings(pkg):
    lib = pkg.capi.lib()
    assert lib.sf_version() == 100
    assert lib.sf_error_string(0) == b"success"
    assert b"invalid" in lib.sf_error_string(-1)
    names = [lib.sf_variant_name(i).decode() for i in range(9)]
    assert names == list(pkg.VARIANTS)


def test_argument_validation_without_gpu(pkg):
    """Validation happens before any HIP call, so it is testable on a CPU-only box."""
    lib = pkg.capi.lib()
    assert lib.sf_bwdtrans_hex_f64(1, 8, 8, 10, None, None, None, None, None, None) == -1
    assert lib.sf_bwdtrans_hex_f64(8, 8, 8, 0, None, None, None, None, None, None) == 0
    assert lib.sf_bwdtrans_hex_f64(8, 8, 8, 4, None, None, None, None, None, None) == -1
    assert lib.sf_bwdtrans_quad_f64(8, 1, 10, None, None, None, None, None) == -1
    assert lib.sf_bwdtrans_quad_f64(8, 8, 0, None, None, None, None, None) == 0
    assert lib.sf_bwdtrans_hex_f64_variant(99, 8, 8, 8, 4, None, None, None, None, None, None,
                                           None) == -1
    # misaligned (odd) addresses are rejected before launch
    assert lib.sf_bwdtrans_hex_f64(8, 8, 8, 4, 0x1000, 0x1000, 0x1000, 0x1001, 0x2000, None) == -2


def test_hex_mfma4_export_validates_as_the_variant_without_gpu(pkg):
    """sf_bwdtrans_hex_f64_mfma4 answers what sf_bwdtrans_hex_f64_variant(SF_VARIANT_MFMA4, nq, nq, nq, ...) answers,
    whichever output path is named -- and, off the kernel's table, before any HIP call."""
    lib = pkg.capi.lib()
    mfma4 = pkg.VARIANTS["mfma4"]
    A = 0x10000  # 16-byte-aligned dummies, never dereferenced
    cases = [  # nq, nelmt, (basis0, basis1, basis2, in, out), expected code
        (1, 10, (A, A, A, A, A), pkg.capi.SF_EINVAL),
        (12, 0, (None, None, None, None, None), pkg.capi.SF_OK),
        (12, 4, (A, A, None, A, A), pkg.capi.SF_EINVAL),            # a null among the pointers
        (12, 4, (A, A, A, A + 1, A), pkg.capi.SF_EALIGN),           # an odd address
        (11, 4, (A, A, A, A, A), pkg.capi.SF_ENOTBUILT),            # off the table
        (12, 4, (A, A, A, A + 8, A), pkg.capi.SF_EALIGN),           # `in` only 8-byte aligned
    ]
    for nq, nelmt, (b0, b1, b2, x, out), want in cases:
        assert lib.sf_bwdtrans_hex_f64_variant(mfma4, nq, nq, nq, nelmt, b0, b1, b2, x, None, out, None) == want, (nq, nelmt)
        for direct in (0, 1):
            assert lib.sf_bwdtrans_hex_f64_mfma4(direct, nq, nelmt, b0, b1, b2, x, out, None) == want, (direct, nq, nelmt)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="replays calls on dummy pointers, which must never meet a real device")
def test_recorded_return_codes(pkg):
    """Every operator entry point answers the cases of tests/golden/make_capi_codes.py -- nulls, misalignment, every
    ordered pair of pointers on one address, an empty batch, a bad extent or variant, two defects at once -- as the build
    that tests/golden/capi_return_codes.json was recorded from did: the validation order and the guarded pairs of every
    family, none of the calls reaching the HIP runtime.  No case is left out: the count per symbol is asserted."""
    import importlib.util
    import json
    golden = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_capi_codes", os.path.join(golden, "make_capi_codes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(golden, "capi_return_codes.json")) as fh:
        recorded = json.load(fh)["symbols"]
    symbols = pkg.capi.SYMBOLS
    names = gen.operator_symbols(symbols)
    assert sorted(recorded) == names and len(names) == 96
    got = gen.replay(pkg.capi.lib(), symbols)
    wrong, total = [], 0
    for name in names:
        want = recorded[name]
        assert len(got[name]) == len(want) == gen.case_count(name, symbols[name][1]), name
        total += len(want)
        wrong += [f"{name}, {label}: rc {rc}, recorded {-int(w)}" for (label, rc), w in zip(got[name], want) if rc != -int(w)]
    assert total == 22610
    assert not wrong, f"{len(wrong)} of {total} cases differ:\n" + "\n".join(wrong[:40])


def test_library_reads_no_environment_variable():
    """The kernels' configuration is what the source says: no file under csrc/ reads the environment."""
    csrc = os.path.join(ROOT, "gpu-benchmarking_amd", "csrc")
    for dirpath, _, files in os.walk(csrc):
        for f in files:
            assert "getenv" not in open(os.path.join(dirpath, f)).read(), f


def test_product_never_imports_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    pkg_dir = os.path.join(ROOT, "gpu-benchmarking_amd")
    for dirpath, _, files in os.walk(pkg_dir):
        if any(part in dirpath for part in ("_build", "__pycache__")):
            continue
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cc", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "liboracle" not in text and "oracle/" not in text.replace(
                    "oracle_fill_random", ""), f


def test_missing_library_fails_loudly(pkg, monkeypatch):
    monkeypatch.setattr(pkg.capi, "_lib", None)
    monkeypatch.setattr(pkg.capi, "LIB_PATH", "/nonexistent/libsumfact.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.capi.lib()
