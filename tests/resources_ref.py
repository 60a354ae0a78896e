"""The compiler's resource report of the kernels of a translation unit, for the CPU tests that hold every wave
instantiation of a family to no scratch, no spills and at most 256 VGPRs: tools/kernel_resources.py run on source units,
its lines parsed and checked once.  Which kernels there must be, and what a family holds them to beyond this, is in the
family's own tests/test_<family>_cpu.py.  RTC_ROW is the line of bin/sf_rtc_check, for the two files that read it.
"""
import collections
import os
import re
import subprocess

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-benchmarking_amd")

Resources = collections.namedtuple("Resources", "name vgpr agpr sgpr scratch spill_v spill_s occ")
ROW = re.compile(r"^(\S.*?)\s+vgpr\s+(-?\d+) agpr\s+(-?\d+) sgpr\s+(-?\d+) scratch\s+(-?\d+) "
                 r"spill v(-?\d+)/s(-?\d+) occ (-?\d+)\s*$")
RTC_ROW = re.compile(r"^(fp64|fp32) ([23])D (\S+)\s+vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) "
                     r"spill v(\d+)/s(\d+) occ (\d+) lds\s+(\d+) wpb (\d) ec\s+(\d+)\s+compile ([\d.]+) s\s+(ok|SPILLS)$")


def parse(line):
    """One line of tools/kernel_resources.py as Resources: it must parse, with no scratch, no spill and 1..256 VGPRs."""
    m = ROW.match(line)
    assert m, f"unparsed kernel_resources line: {line!r}"
    r = Resources(m.group(1), *(int(g) for g in m.groups()[1:]))
    assert r.scratch == 0 and r.spill_v == 0 and r.spill_s == 0, line
    assert 0 < r.vgpr <= 256, line
    return r


def kernel_resources(units, kernel, timeout=1800):
    """(unit, Resources) of every kernel of csrc/<unit> whose demangled name contains `kernel`, for every unit of `units`,
    each line through parse(); the units compile side by side, and each must list at least one kernel."""
    tool = os.path.join(PKG, "tools", "kernel_resources.py")
    procs = [subprocess.Popen(["python3", tool, os.path.join(PKG, "csrc", unit), kernel], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=PKG) for unit in units]
    found = []
    for unit, proc in zip(units, procs):
        out = proc.communicate(timeout=timeout)[0]
        lines = [ln for ln in out.splitlines() if ln.strip()]
        assert lines, (unit, kernel, out)
        found += [(unit, parse(ln)) for ln in lines]
    return found
