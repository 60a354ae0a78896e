"""Every operator timing tool (tools/*_bench.py) runs: main([...]) in-process at the smallest sizes the tools take, with
--json into tmp_path.  Held to: exit status 0, a JSON document whose recursive key layout (names and order) is the literal
below -- the layout the tools had before they shared tools/opbench.py, on which the recorded logs and the tables of
DESIGN.md depend --, hip_graph_replay true, and every check value present and finite (or true).  No bound on any
chain_rel_diff: accuracy is the parity tests' subject.  aniso_bench.py is not here: it takes no options, compiles a
specialisation per shape and shares nothing with the harness.
"""
import importlib
import json
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "gpu-benchmarking_amd", "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

pytestmark = pytest.mark.gpu

COMMON = "--hex 4 --quad 5 --nelmt3 512 --nelmt2 1024 --reps 2 --f32".split()
SINGLE = "--hex 4 --quad 5 --nelmt 1024 --reps 2".split()
CHECKS = ("chain_rel_diff", "rel_diff", "bits_equal", "equal_values", "launched_specialisation", "global_to_local_equal",
          "assemble_rel_diff", "gs_rel_diff")


def keys(names):
    return dict.fromkeys(names.split())


def table(row, hex_=("4",), quad=("5",), ops=("",)):
    """{[op_]hex_f64: {order: row}, [op_]quad_f64: ..., [op_]hex_f32: ..., [op_]quad_f32: ...}: the order of the sweep."""
    return {f"{op}{shape}_{t}": {n: row for n in ns}
            for t in ("f64", "f32") for shape, ns in (("hex", hex_), ("quad", quad)) for op in ops}


def document(head, body, tail=""):
    return {**keys("protocol device " + head), **body, **keys("hip_graph_replay " + tail)}


ROOF = "gb_s frac_mean frac_min "
CHAIN = "t_chain t_chain_min speedup_vs_chain not_slower_than_chain "
VERSUS = keys("ms ms_min scalars_per_element " + ROOF + "ms_deformed ms_deformed_min deformed_scalars_per_element "
              "deformed_frac_mean ratio ratio_min ok bits_equal")
GEOM_REP = keys("t_geom t_geom_min " + ROOF + CHAIN)
TENSOR_REP = keys("t_tensor t_tensor_min " + ROOF + CHAIN)
TENSOR_ROW = {"repeats": [TENSOR_REP] * 2, **keys("not_slower_than_chain chain_rel_diff")}
ADVECT_ROW = keys("repeat t_advect t_advect_min gdof_s " + ROOF + CHAIN)
VECGRAD_ROW = keys("repeat outputs t_vecgrad t_vecgrad_min " + ROOF + CHAIN)
GS_ROW = keys("ms ms_min " + ROOF + "ms_torch ms_torch_min speedup_vs_torch at_least_as_fast")
GS_CALLS = {"global_to_local": GS_ROW, "assemble": GS_ROW, "gs": GS_ROW,
            "check": keys("global_to_local_equal assemble_rel_diff gs_rel_diff")}
GS_HELM = {"helmholtz": keys("ms_operator ms_operator_min ms_assembled ms_assembled_min assembled_over_operator")}


def gs_mesh(dim, f64):
    return {"nel": [None] * dim, **keys("nlocal nglobal shared setup_ms"), "f64": f64, "f32": GS_CALLS}


# tool: (arguments, layout, whether the document holds check values)
TOOLS_CASES = {
    "advect": (COMMON + ["--chain", "--check"],
               document("", {"advect": table([ADVECT_ROW] * 2 + [keys("chain_rel_diff")])}), True),
    "affine_advect": (COMMON + ["--check"],
                      document("", {"repeats": [table(VERSUS, ops=("advect_",))]}, "all_ok bits_equal"), True),
    "affine": (COMMON + ["--mass", "--laplacian"],
               document("lambda", {"affine": table(keys(
                   "ms ms_min gdof_s scalars_per_element " + ROOF + "ms_deformed ms_deformed_min "
                   "deformed_scalars_per_element deformed_frac_mean ratio ratio_min ok rel_diff ms_mass mass_frac_mean "
                   "mass_frac_min"))}, "all_ok"), True),
    "affine_deriv": (COMMON + ["--check"],
                     document("je", {"repeats": [table(VERSUS, ops=("gradient_", "weak_divergence_"))]},
                              "all_ok bits_equal"), True),
    "diag": (COMMON + ["--chain", "--check", "--helmholtz", "--laplacian"],
             document("lambda", {"diag": table(keys(
                 "ms ms_min gdof_s " + ROOF + "ms_chain ms_chain_min speedup_vs_chain chain_rel_diff ms_helmholtz "
                 "ms_helmholtz_min helmholtz_frac_mean helmholtz_frac_min diag_over_helmholtz"))}), True),
    "geom": (COMMON + ["--chain", "--check"],
             document("", {"geom": table({"repeats": [GEOM_REP] * 2, "not_slower_than_chain": None,
                                          "chain_rel_diff": keys("df w g detj")})}), True),
    "gs": ("--hex 4 --quad 8 --nq 4 --reps 2 --f32 --check --helmholtz".split(),
           document("nq sign", {"gs": {"hex": gs_mesh(3, {**GS_CALLS, **GS_HELM}), "quad": gs_mesh(2, GS_CALLS)}}), True),
    "helmholtz": (COMMON + ["--chain", "--check", "--mass", "--laplacian"],
                  document("lambda", {"helmholtz": table(keys(
                      "ms ms_min gdof_s " + ROOF + "ms_chain ms_chain_min speedup_vs_chain chain_rel_diff ms_mass "
                      "mass_frac_mean mass_frac_min ms_bwd bwd_frac_mean bwd_frac_min"))}), True),
    "iprod": (SINGLE + ["--bwdtrans"],
              document("", {what: table(keys("gdof_s gdof_s_min " + ROOF)) for what in ("iproduct", "bwdtrans")}), False),
    "iprodderiv": (COMMON + ["--chain", "--check"],
                   document("", {"iprodderiv": table(keys(
                       "t_iprodderiv t_iprodderiv_min gdof_s " + ROOF + "t_bothnull t_bothnull_min bothnull_frac_mean "
                       "bothnull_frac_min t_physderiv physderiv_frac_mean physderiv_frac_min t_iproduct iproduct_frac_mean "
                       "iproduct_frac_min " + CHAIN + "chain_excess chain_agrees chain_rel_diff"))}), True),
    "mass": (SINGLE + ["--chain"],
             document("", {"mass": table(keys("ms ms_min gdof_s " + ROOF + "ms_chain speedup_vs_chain ms_bwd ms_iprod "
                                              "ms_bwd_plus_iprod ratio_to_bwd_plus_iprod"))}), False),
    "physderiv": (COMMON + ["--chain", "--check"],
                  document("", {"physderiv": table(keys(
                      "t_physderiv t_physderiv_min gdof_s " + ROOF + "t_refspace t_refspace_min refspace_frac_mean "
                      "refspace_frac_min t_helmholtz helmholtz_frac_mean helmholtz_frac_min t_bwd bwd_frac_mean "
                      "bwd_frac_min " + CHAIN + "chain_rel_diff"))}), True),
    "tensor": ("--hex 4>6,6>4:t --quad 5>7 --nelmt3 512 --nelmt2 1024 --reps 2 --f32 --chain --check".split(),
               document("", {"tensor": table(TENSOR_ROW, hex_=("4>6", "6>4:t"), quad=("5>7",))}), True),
    "vecgrad": (COMMON + ["--chain", "--check"],
                document("", {"vecgrad": table([VECGRAD_ROW] * 4 + [{"chain_rel_diff": keys("grad div curl")}])}), True),
}


def layout(x):
    if isinstance(x, dict):
        return {k: layout(v) for k, v in x.items()}
    if isinstance(x, list):
        return [layout(v) for v in x]
    return None


def check_values(x, found):
    """Every value under a key of CHECKS, collected into `found`, must be true or a finite number (or a dict of them)."""
    if isinstance(x, dict):
        for k, v in x.items():
            if k in CHECKS:
                for leaf in (v.values() if isinstance(v, dict) else [v]):
                    assert leaf is True or (isinstance(leaf, float) and math.isfinite(leaf)), (k, v)
                    found.append(k)
            else:
                check_values(v, found)
    elif isinstance(x, list):
        for v in x:
            check_values(v, found)


@pytest.mark.parametrize("tool", sorted(TOOLS_CASES))
def test_tool_runs_and_keeps_its_layout(tool, tmp_path):
    argv, expected, has_checks = TOOLS_CASES[tool]
    path = tmp_path / f"{tool}.json"
    status = importlib.import_module(f"{tool}_bench").main(argv + ["--json", str(path)])
    assert status == 0
    doc = json.loads(path.read_text())
    got = layout(doc)
    assert got == expected
    assert json.dumps(got) == json.dumps(expected)                # and in the same order
    assert doc["hip_graph_replay"] is True
    found = []
    check_values(doc, found)
    assert bool(found) == has_checks, found
