#!/usr/bin/env python3
"""Show what became of a kernel's software prefetch in the machine code.

Compiles one .hip file to gfx950 assembly (device side only, the Makefile's flags; no GPU needed) and prints, per kernel
and per loop (a backward branch and the label it targets), the vector-memory loads issued, the EXEC-mask branches, and
every wait on the vector-memory counter with the number of loads issued since the previous wait:

    python tools/prefetch_waits.py vision_mtl_amd/csrc/conv_pw.hip [-k pw_gemm_kernel] [-D NAME=VALUE ...] [--seq]

Reading it: a prefetch that is really in flight shows up as `vmcnt(N)` with N > 0 in front of the consumer (N = the
loads of the younger groups); `vmcnt(0)` directly after a group's loads, or `execz` branches between the loop header and
its back edge, mean that the pipeline in the source drains once per step.  --seq prints the loop bodies as one line of
events in program order (L = load, S = store, M<n> = n MFMAs, W<n> = vmcnt(n), B = barrier, X = execz branch).
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision_mtl_amd", "csrc")

LOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)_")
STORE = re.compile(r"^(global_store|buffer_store|flat_store|scratch_store|global_atomic|buffer_atomic|flat_atomic)_")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    sys.exit("prefetch_waits: no hipcc")


def compile_asm(src, defines, arch):
    cmd = [hipcc(), "-O3", "-std=c++17", f"--offload-arch={arch}", "-S", "--cuda-device-only", "-I", CSRC, "-o", "-", src]
    cmd += [f"-D{d}" for d in defines]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(asm):
    """[(mangled name, [instruction or label lines])] for every .amdhsa kernel"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, body = [], None, []
    for raw in asm.split("\n"):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur, body = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            out.append((cur, body))
            cur = None
            continue
        if line.startswith(".") and not LABEL.match(line):
            continue  # directives
        body.append(line)
    return out


def events(lines):
    """program-order events of a span: (kind, value)"""
    ev, mf = [], 0

    def flush():
        nonlocal mf
        if mf:
            ev.append(("M", mf))
            mf = 0

    for ln in lines:
        op = ln.split()[0]
        if op.startswith("v_mfma"):
            mf += 1
            continue
        if LOAD.match(op):
            flush(); ev.append(("L", 1))
        elif STORE.match(op):
            flush(); ev.append(("S", 1))
        elif op == "s_waitcnt":
            m = VMCNT.search(ln)
            if m:
                flush(); ev.append(("W", int(m.group(1))))
        elif op == "s_barrier":
            flush(); ev.append(("B", 1))
        elif op == "s_cbranch_execz" or op == "s_cbranch_execnz":
            flush(); ev.append(("X", 1))
        elif op.startswith("ds_write") or op.startswith("ds_store"):
            flush(); ev.append(("D", 1))
    flush()
    return ev


def merge(ev):
    """run-length merge of L / S / D / X events"""
    out = []
    for k, v in ev:
        if out and out[-1][0] == k and k in "LSDX":
            out[-1] = (k, out[-1][1] + v)
        else:
            out.append((k, v))
    return out


def describe(ev):
    loads = sum(v for k, v in ev if k == "L")
    stores = sum(v for k, v in ev if k == "S")
    mfma = sum(v for k, v in ev if k == "M")
    execz = sum(v for k, v in ev if k == "X")
    waits, since = [], 0
    for k, v in ev:
        if k == "L":
            since += v
        elif k == "W":
            waits.append(f"vmcnt({v})@+{since}")
            since = 0
    return loads, stores, mfma, execz, waits


def seq(ev):
    return " ".join({"L": f"L{v}", "S": f"S{v}", "D": f"D{v}", "M": f"M{v}", "W": f"W{v}", "B": "B", "X": f"X{v}"}[k]
                    for k, v in merge(ev))


def loops(body):
    pos = {}
    for i, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            pos[m.group(1)] = i
    found = {}
    for i, ln in enumerate(body):
        m = BRANCH.match(ln)
        if m and m.group(1) in pos and pos[m.group(1)] < i:
            head = pos[m.group(1)]
            found[head] = max(found.get(head, 0), i)  # several back edges to one header: the outermost
    return sorted(found.items())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("-k", "--kernel", default="", help="only kernels whose demangled name matches this regular expression")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--seq", action="store_true", help="print each loop body as a line of events")
    ap.add_argument("--loops", type=int, default=3, help="loops printed per kernel, in program order (0 = all); a "
                    "backward branch out of a block the compiler moved behind the kernel's end also counts as one")
    ap.add_argument("--seq-limit", type=int, default=400, help="longest wait list / event line printed (0 = whole)")
    ap.add_argument("--save-asm", default="", help="also write the assembly to this file")
    ap.add_argument("--min-loads", type=int, default=1, help="skip loops with fewer vector-memory loads")
    a = ap.parse_args()
    asm = compile_asm(a.src, a.defines, a.arch)
    if a.save_asm:
        with open(a.save_asm, "w") as f:
            f.write(asm)
    ks = kernels(asm)
    names = demangle([k for k, _ in ks])
    print(f"# {os.path.relpath(os.path.abspath(a.src), ROOT)}  ({a.arch}, -O3{''.join(' -D' + d for d in a.defines)})")
    for k, body in ks:
        name = names[k].replace("void ", "").split("(")[0]
        if not re.search(a.kernel, name):
            continue
        loads, stores, mfma, execz, waits = describe(events(body))
        zero = sum(1 for w in waits if w.startswith("vmcnt(0)"))
        print(f"\n{name}\n  whole kernel: {loads} loads, {stores} stores, {mfma} mfma, {execz} exec branches, "
              f"{len(waits)} vmcnt waits ({zero} of them vmcnt(0))")
        shown = 0
        for head, tail in loops(body):
            ev = events(body[head:tail + 1])
            loads, stores, mfma, execz, waits = describe(ev)
            if loads < a.min_loads:
                continue
            shown += 1
            if a.loops and shown > a.loops:
                continue
            wl = " ".join(waits) if waits else "none"
            if a.seq_limit and len(wl) > a.seq_limit:
                wl = wl[:a.seq_limit] + " ..."
            print(f"  loop {body[head][:-1]} ({tail - head} lines): {loads} loads, {stores} stores, {mfma} mfma, "
                  f"{execz} exec branches; waits: {wl}")
            if a.seq:
                line = seq(ev)
                print(f"    {line if not a.seq_limit or len(line) <= a.seq_limit else line[:a.seq_limit] + ' ...'}")
        if a.loops and shown > a.loops:
            print(f"  (+{shown - a.loops} more backward branches with loads)")


if __name__ == "__main__":
    main()
