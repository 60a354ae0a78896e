"""CPU checks of tools/opbench.py, the harness the operator timing tools (tools/*_bench.py) share: the table of algorithmic
scalars per element behind every published roofline fraction, pinned to values worked out by hand from the formulas each
tool used to carry and to the scalars recorded in profiles/r16 and profiles/r20; every tool's command line, defaults as
literals; and the rounding of the rates.  No device is needed: opbench imports without torch and without the library.
"""
import ast
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "gpu-benchmarking_amd", "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import opbench  # noqa: E402
from opbench import scalars  # noqa: E402

# 3D nq 8: nm^3 = 343, nq^3 = 512; 2D nq 16: nm^2 = 225, nq^2 = 256.  (op, options): (3D nq 8, 2D nq 16)
TABLE = [
    ("bwdtrans", {}, 855, 481),                                   # nm^d + nq^d
    ("iproduct", {}, 855, 481),
    ("mass", {}, 1198, 706),                                      # 2 nm^d + nq^d
    ("helmholtz", {}, 4270, 1474),                                # 2 nm^d + (1 + d(d+1)/2) nq^d
    ("helmholtz", {"w": False}, 3758, 1218),
    ("affine_helmholtz", {}, 693, 454),                           # 2 nm^d + d(d+1)/2 + 1
    ("affine_helmholtz", {"je": False}, 692, 453),
    ("affine_helmholtz_deformed", {}, 4270, 1474),
    ("affine_helmholtz_deformed", {"je": False}, 3758, 1218),
    ("diag_helmholtz", {}, 3927, 1249),                           # (1 + d(d+1)/2) nq^d + nm^d
    ("diag_helmholtz", {"w": False}, 3415, 993),
    ("physderiv", {}, 6487, 1761),                                # nm^d + (d^2 + d) nq^d
    ("physderiv", {"df": False}, 1879, 737),                      # nm^d + d nq^d
    ("iprodderiv", {}, 6999, 2017),                               # (d^2 + d + 1) nq^d + nm^d
    ("iprodderiv", {"w": False}, 6487, 1761),
    ("iprodderiv", {"df": False, "w": False}, 1879, 737),
    ("affine_physderiv", {}, 1888, 741),                          # nm^d + d nq^d + d^2
    ("affine_iprodderiv", {}, 1889, 742),                         # d nq^d + nm^d + d^2 + 1
    ("affine_iprodderiv", {"je": False}, 1888, 741),
    ("geom", {}, 9733, 2754),                                     # d nm^d + (d^2 + d(d+1)/2 + 2) nq^d
    ("advect", {}, 8714, 2692),                                   # (d^2 + d + 1) nq^d + 2 nf nm^d, nf = d
    ("advect", {"nf": 1}, 7342, 2242),
    ("affine_advect", {}, 3604, 1417),                            # d nq^d + 2 d nm^d + d^2 + 1
    ("vecgrad", {}, 12293, 3010),                                 # d nm^d + d^2 nq^d + (d^2 + 1 + d(d-1)/2) nq^d
    ("vecgrad", {"outputs": ("div", "curl")}, 7685, 1986),
]


@pytest.mark.parametrize("op,options,hex8,quad16", TABLE, ids=[f"{t[0]}-{'-'.join(map(str, t[1])) or 'all'}" for t in TABLE])
def test_scalars_per_element(op, options, hex8, quad16):
    assert scalars(op, 3, 8, **options) == hex8
    assert scalars(op, 2, 16, **options) == quad16


def test_scalars_tensor_and_the_table_is_covered():
    assert scalars("tensor", 3, ni=4, no=6) == 280 and scalars("tensor", 2, ni=10, no=15) == 325
    assert scalars("tensor", 3, ni=7, no=8) == scalars("bwdtrans", 3, 8)
    assert scalars("advect", 3, 8, nf=3) == 8714 and scalars("advect", 2, 16, nf=2) == 2692
    assert {t[0] for t in TABLE} | {"tensor"} == set(opbench._SCALARS)
    with pytest.raises(TypeError):
        scalars("mass", 3, 8, w=False)                            # an option the operator does not have
    with pytest.raises(KeyError):
        scalars("helmholz", 3, 8)


RECORDED = [("r16/affine_deriv_vs_deformed.log", {"gradient": ("affine_physderiv", "physderiv"),
                                                  "weak_divergence": ("affine_iprodderiv", "iprodderiv")}, 24),
            ("r20/affine_advect_vs_deformed.log", {"advect": ("affine_advect", "advect")}, 24)]


@pytest.mark.parametrize("log,ops,rows", RECORDED, ids=[r[0][:3] for r in RECORDED])
def test_scalars_match_the_recorded_logs(log, ops, rows):
    seen = 0
    with open(os.path.join(ROOT, "profiles", log)) as fh:
        for line in fh:
            m = re.match(r"repeat \d+ (\w+) (\d)D f\d\d nq +(\d+): (\{.*\})$", line.strip())
            if not m:
                continue
            affine, deformed = ops[m.group(1)]
            dim, nq, row = int(m.group(2)), int(m.group(3)), ast.literal_eval(m.group(4))
            assert scalars(affine, dim, nq) == row["scalars_per_element"], line
            assert scalars(deformed, dim, nq) == row["deformed_scalars_per_element"], line
            seen += 1
    assert seen == rows


SPLIT = {"nelmt3": 1 << 18, "nelmt2": 1 << 20, "reps": 40, "hex": [4, 6, 8], "quad": [8, 12, 16], "f32": False,
         "variant": "auto", "json": None}
SINGLE = {"nelmt": 1 << 20, "reps": 40, "hex": list(range(2, 12)), "quad": list(range(2, 17)), "no_f32": False,
          "json": None}
CHAIN = {"chain": False, "check": False}
DEFAULTS = {
    "advect": {**SPLIT, **CHAIN, "repeats": 2},
    "affine_advect": {**SPLIT, "check": False, "repeats": 1},
    "affine": {**SPLIT, "laplacian": False, "mass": False, "no_deformed": False},
    "affine_deriv": {**SPLIT, "check": False, "repeats": 1, "no_je": False},
    "diag": {**SPLIT, **CHAIN, "laplacian": False, "helmholtz": False},
    "geom": {**SPLIT, **CHAIN, "repeats": 2},
    "gs": {"hex": 64, "quad": 1024, "nq": 8, "reps": 20, "f32": False, "sign": False, "helmholtz": False, "check": False,
           "json": None},
    "helmholtz": {**SPLIT, **CHAIN, "laplacian": False, "mass": False},
    "iprod": {**SINGLE, "bwdtrans": False},
    "iprodderiv": {**SPLIT, **CHAIN},
    "mass": {**SINGLE, "chain": False, "variant": "auto"},
    "physderiv": {**SPLIT, **CHAIN},
    "tensor": {**SPLIT, **CHAIN, "repeats": 2, "bwdtrans": False,
               "hex": [(8, 8, 0), (4, 6, 0), (6, 9, 0), (9, 6, 1)], "quad": [(8, 8, 0), (16, 16, 0), (10, 15, 0)]},
    "vecgrad": {**SPLIT, **CHAIN, "repeats": 2},
}
VALUES = {"nelmt3": "512", "nelmt2": "1024", "nelmt": "1024", "reps": "2", "repeats": "3", "hex": "4,5", "quad": "5",
          "nq": "4", "variant": "wave", "json": "x.json"}


@pytest.mark.parametrize("tool", sorted(DEFAULTS))
def test_command_line(tool):
    options = importlib.import_module(f"{tool}_bench").options
    assert vars(options([])) == DEFAULTS[tool]
    argv = []
    for name, default in DEFAULTS[tool].items():
        argv += [f"--{name.replace('_', '-')}"] + ([] if default is False else [VALUES[name]])
    if tool in ("gs", "tensor"):
        argv[argv.index("--hex") + 1] = "4" if tool == "gs" else "4>6,6>4:t"
        argv[argv.index("--quad") + 1] = "5" if tool == "gs" else "5>7"
    got = vars(options(argv))
    assert set(got) == set(DEFAULTS[tool])
    assert all(v is True for k, v in got.items() if DEFAULTS[tool][k] is False)
    assert got["reps"] == 2 and got["json"] == "x.json"
    assert got["hex"] == {"gs": 4, "tensor": [(4, 6, 0), (6, 4, 1)]}.get(tool, [4, 5])
    assert got["quad"] == {"gs": 5, "tensor": [(5, 7, 0)]}.get(tool, [5])


def test_rates_round_as_the_recorded_logs():
    nb, t = 1234567890, 0.321                                     # 3846.0058... GB/s, 0.48075... of 8 TB/s
    assert opbench.frac(nb, t) == round(nb / t * 1e-6 / 8000.0, 4) == 0.4808
    assert opbench.gb_s(nb, t) == round(nb / t * 1e-6, 1) == 3846.0
    assert opbench.gdof_s(262144 * 343, 0.5) == 179.83            # 179.830784
    assert opbench.ms(0.123456789) == 0.12346
    assert opbench.frac(8e9, 1.0) == 1.0
    assert opbench.roofline(nb, t, 0.3) == {"gb_s": 3846.0, "frac_mean": 0.4808, "frac_min": 0.5144}
    assert opbench.fracs("mass", nb, t, 0.3) == {"mass_frac_mean": 0.4808, "mass_frac_min": 0.5144}
    assert opbench.chain_row(0.5, 1.0, 0.9) == {"t_chain": 1.0, "t_chain_min": 0.9, "speedup_vs_chain": 2.0,
                                                "not_slower_than_chain": True}
    assert opbench.chain_row(0.5, 0.4, 0.3, prefix="ms", bar=False) == {"ms_chain": 0.4, "ms_chain_min": 0.3,
                                                                       "speedup_vs_chain": 0.8}


def test_opbench_imports_without_torch_or_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import opbench, helmholtz_bench, gs_bench; "
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('gpu_benchmarking_amd')]; "
            "assert not bad, bad")
    subprocess.run([sys.executable, "-c", code, TOOLS], check=True, cwd=ROOT)
