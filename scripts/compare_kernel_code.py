#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel: for a refactor that must not change what the GPU runs.

    python scripts/compare_kernel_code.py OLD_DIR NEW_DIR      # two directories of the Makefile's object files (*.o)

Every object's gfx950 code object is extracted (llvm-objdump --offloading) and disassembled; a function's instruction sequence is
its disassembly without addresses, encodings and branch targets.  Prints the functions whose sequences differ, with both
instruction counts and, for kernels, both vgpr_count / private_segment_fixed_size / group_segment_fixed_size of the code object's
notes, the functions only one build has, and the objects only one build has (a difference unless the object is host-only); a differing function whose two builds hold the same opcodes the same number of times
(another schedule or register assignment) is marked.  A plain text diff: it looks for no particular instruction.
Exit status: 0 = identical, 1 = differences, 2 = a kernel's registers, scratch or LDS grew.
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

BUDGETS = ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(llvm, obj, work):
    """-> (functions {symbol: [instruction, ...]}, kernels {symbol: {budget: value}}) of one object file"""
    shutil.copy(obj, work)                                   # the bundles are extracted next to the object: never into the tree
    name = os.path.basename(obj)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", name], cwd=work, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(work) if f.startswith(name) and "amdgcn" in f and "gfx950" in f]
    if not dev:
        return {}, {}                                        # host-only translation unit
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", dev[0]], cwd=work, check=True, capture_output=True, text=True).stdout
    funcs, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = line.split("//")[0].strip()
        if not ins:
            continue
        if re.match(r"s_(c?branch|call)", ins):              # the target is an address
            ins = ins.split()[0]
        elif pcrel and re.match(r"s_addc?_u32 ", ins):        # s_getpc_b64 + offset: the address of data or of another function
            ins = ins.rsplit(",", 1)[0] + ", <addr>"
            pcrel -= 1
        else:
            pcrel = 2 if ins.startswith("s_getpc_b64") else 0
        cur.append(re.sub(r"<[^>]*>", "<sym>", ins))
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev[0]], cwd=work, check=True, capture_output=True, text=True).stdout
    kernels, entry = {}, {}
    for line in notes.splitlines() + ["  - .end:"]:          # a kernel's entry: "  - .key: value" then "    .key: value" lines
        m = re.match(r"^  (- | {2})\.(\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            if "name" in entry:
                kernels[entry["name"]] = {b: int(entry.get(b, 0)) for b in BUDGETS}
            entry = {}
        entry[m.group(2)] = m.group(3)
    return funcs, kernels


def demangle(sym):
    try:
        return subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip() or sym
    except OSError:
        return sym


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--llvm", default=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"))
    ap.add_argument("--diff", action="store_true", help="also print a unified diff of each differing function")
    a = ap.parse_args()
    objs = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    old_objs, new_objs = objs(a.old_dir), objs(a.new_dir)
    status = 0
    for f in sorted(old_objs ^ new_objs):                    # a translation unit that came or went: a difference if it holds device code
        d = a.old_dir if f in old_objs else a.new_dir
        with tempfile.TemporaryDirectory() as w:
            funcs, _ = code_object(a.llvm, os.path.join(d, f), w)
        print(f"{f}: only in {d}" + (f", {len(funcs)} device functions" if funcs else ", host-only"))
        if funcs:
            status = 1
    n_funcs = n_kernels = 0
    for f in sorted(old_objs & new_objs):
        with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
            fa, ka = code_object(a.llvm, os.path.join(a.old_dir, f), wa)
            fb, kb = code_object(a.llvm, os.path.join(a.new_dir, f), wb)
        n_funcs += len(fb)
        n_kernels += len(kb)
        for s in sorted(set(fa) ^ set(fb)):
            print(f"{f}: {demangle(s)}: only in the {'old' if s in fa else 'new'} build{' (kernel)' if s in ka or s in kb else ''}")
            status = max(status, 1)
        for s in sorted(set(fa) & set(fb)):
            grew = [b for b in BUDGETS if s in ka and s in kb and kb[s].get(b, 0) > ka[s].get(b, 0)]
            if fa[s] == fb[s] and not grew:
                continue
            status = max(status, 2 if grew else 1)
            print(f"{f}: {demangle(s)}")
            ops = lambda body: sorted(i.split()[0] for i in body)
            print(f"    instructions {len(fa[s])} -> {len(fb[s])}" + (" (same sequence)" if fa[s] == fb[s] else
                                                                    " (the same opcodes, in another order or other registers)" if ops(fa[s]) == ops(fb[s]) else ""))
            if s in ka and s in kb:
                print("    " + ", ".join(f"{b} {ka[s].get(b)} -> {kb[s].get(b)}" for b in BUDGETS) + ("   GREW: " + ", ".join(grew) if grew else ""))
            if a.diff:
                for line in difflib.unified_diff(fa[s], fb[s], "old", "new", lineterm="", n=2):
                    print("      " + line)
    print(f"{len(old_objs & new_objs)} objects, {n_funcs} device functions ({n_kernels} kernels) compared: " +
          ("identical" if status == 0 else "DIFFERENCES above"))
    return status


if __name__ == "__main__":
    sys.exit(main())
