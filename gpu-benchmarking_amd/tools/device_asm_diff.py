#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel: the check of a refactor that must not change
what a kernel does.

    python3 tools/device_asm_diff.py PARENT_TREE NEW_TREE [--identical | --by-content] [-j N] [unit ...]

PARENT_TREE / NEW_TREE: two copies of gpu-benchmarking_amd/ (the directories that hold csrc/).  unit: file names under
csrc/ (default: every csrc/*.hip of NEW_TREE).  Each unit of each tree is compiled to device assembly with the flags of the
Makefile (+ --cuda-device-only -S -Rpass-analysis=kernel-resource-usage); kernels are matched by mangled name.

Must be equal per kernel (exit status 1 otherwise): the kernel set; the count of every mnemonic of floating-point
arithmetic (v_[pk_]{fma,fmac,mul,add,sub,mad,mac}*_f*), of LDS access (ds_*) and of vector memory access (global_*,
buffer_*, flat_*, scratch_*); the occupancy remark; the LDS size.  Scratch size and spill counts must be 0, or where
the parent's kernel already has some, not above the parent's.
Recorded (a table row for every kernel where one moved): VGPRs, SGPRs, s_waitcnt count, instruction count.
With --identical the sha256 of every kernel's text must be equal instead (units that the change does not touch).
With --by-content kernels are matched by text, not by name (a change that removes kernels, which renumbers the local
labels of every later kernel of the unit, or template parameters, which renames a kernel): the function index in local
labels (.LBB<f>_<n>, .LJTI<f>_<n>, ...) and the kernel's own name are normalised before hashing, and every kernel of the
new tree must then equal one kernel of the parent's unit, each parent kernel serving once.  Parent kernels left without
a partner are listed by demangled name; the exit status is 0 when every new kernel found one.
"""
import argparse
import collections
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-pass-failed",
         "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", "-"]
MUST = re.compile(r"^(v_(pk_)?(fma|fmac|mul|add|sub|mad|mac)\w*_f(16|32|64)(_|$)|ds_|global_|buffer_|flat_|scratch_)")
REMARK = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass")
EQUAL = ("Occupancy", "LDS Size")
ZERO = ("ScratchSize", "VGPRs Spill", "SGPRs Spill")
RECORD = ("VGPRs", "TotalSGPRs", "s_waitcnt", "insts")
LABEL = re.compile(r"(\.L[A-Za-z_]+|\bBB)\d+_(\d+)")  # .LBB12_3 and, in comments, BB12_3: drop the function index


def content_sha(name, text):
    """sha256 of a kernel's text with its own name, the function index of local labels and column padding normalised."""
    body = LABEL.sub(r"\1_\2", "\n".join(text).replace(name, "KERNEL"))
    return hashlib.sha256(re.sub(r"[ \t]+", " ", body).encode()).hexdigest()


def kernels_of(tree, unit):
    """{mangled name: {"sha", "must": Counter, remark fields, "s_waitcnt", "insts"}} of one unit of one tree."""
    run = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [os.path.join("csrc", unit)],
                         cwd=tree, capture_output=True, text=True)
    if run.returncode:
        sys.exit(f"{tree}: {unit} does not compile\n{run.stderr[-2000:]}")
    res, cur = {}, None
    for ln in run.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = REMARK.search(ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", run.stdout, re.M))
    out, cur, text = {}, None, []
    for ln in run.stdout.splitlines():
        if cur is None:
            if ln.split(":")[0] in names:  # "name:   ; @name"
                cur, text = ln.split(":")[0], []
            continue
        if ln.startswith(".Lfunc_end"):
            ops = [t.split()[0] for t in (x.split(";")[0].strip() for x in text)
                   if t and not t.startswith(".") and not t.endswith(":")]
            k = dict(res.get(cur, {}))
            k["sha"] = hashlib.sha256("\n".join(text).encode()).hexdigest()
            k["csha"] = content_sha(cur, text)
            k["must"] = collections.Counter(o for o in ops if MUST.match(o))
            k["s_waitcnt"] = sum(o.startswith("s_waitcnt") for o in ops)
            k["insts"] = len(ops)
            out[cur], cur = k, None
        else:
            text.append(ln)
    return out


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"^void sf::", "", d).split("(")[0] for d in out]


def by_content(unit, old, new):
    """Pair every kernel of `new` with one of `old` of equal normalised text; returns the number left without one."""
    free = collections.defaultdict(list)
    for n in sorted(old):
        free[old[n]["csha"]].append(n)
    lone = []
    for n in sorted(new, key=lambda n: (n not in old, n)):  # kernels that kept their name take their namesake first
        pool = free[new[n]["csha"]]
        if n in pool:
            pool.remove(n)
        elif pool:
            pool.pop(0)
        else:
            lone.append(n)
    for d in demangled(lone):
        print(f"FAIL {unit}: {d}: equals no kernel of the parent tree")
    rest = sorted(n for pool in free.values() for n in pool)
    for d in demangled(rest):
        print(f"parent only {unit}: {d}")
    print(f"== {unit}: parent {len(old)} kernels, new {len(new)}, {len(new) - len(lone)} equal a parent kernel by content, "
          f"{len(rest)} only in the parent, {len(lone)} FAILED")
    return len(lone)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("units", nargs="*")
    ap.add_argument("--identical", action="store_true")
    ap.add_argument("--by-content", action="store_true")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_intermixed_args()  # unit names may follow the flags
    units = a.units or sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.new, "csrc", "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        jobs = {(t, u): pool.submit(kernels_of, t, u) for u in units for t in (a.parent, a.new)}
    bad = 0
    for u in units:
        old, new = jobs[(a.parent, u)].result(), jobs[(a.new, u)].result()
        if a.by_content:
            bad += by_content(u, old, new)
            continue
        names = sorted(set(old) | set(new))
        same = moved = fail = 0
        for n, short in zip(names, demangled(names)):
            if n not in old or n not in new:
                print(f"FAIL {u}: {short}: only in the {'new' if n in new else 'parent'} tree")
                fail += 1
                continue
            o, w = old[n], new[n]
            if o["sha"] == w["sha"] and all(f in w for f in EQUAL + ZERO + RECORD):
                same += 1
                continue
            why = ["text differs"] if a.identical else []
            for m in sorted(set(o["must"]) | set(w["must"])):
                if o["must"][m] != w["must"][m]:
                    why.append(f"{m} {o['must'][m]} -> {w['must'][m]}")
            for f in EQUAL + ZERO + RECORD:  # a kernel without one of the figures has not been checked
                if f not in o or f not in w:
                    why.append(f"{f} missing")
            for f in EQUAL:
                if o.get(f, -1) != w.get(f, -1):
                    why.append(f"{f} {o.get(f, -1)} -> {w.get(f, -1)}")
            for f in ZERO:
                if w.get(f, -1) != 0 and not 0 <= w.get(f, -1) <= o.get(f, -1):
                    why.append(f"{f} {o.get(f, -1)} -> {w.get(f, -1)}")
            if why:
                print(f"FAIL {u}: {short}: " + "; ".join(why))
                fail += 1
            if any(o.get(f) != w.get(f) for f in RECORD):
                moved += 1
                print(f"moved {u}: {short}: " + "  ".join(
                    f"{f} {o.get(f, -1)} -> {w.get(f, -1)} ({w.get(f, -1) - o.get(f, -1):+d})" for f in RECORD))
        print(f"== {u}: {len(names)} kernels, {same} identical, {moved} with moved registers / waits / totals, "
              f"{fail} FAILED")
        bad += fail
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
