#!/usr/bin/env python3
"""Compare two device code objects function by function (CPU only).

    hipcc <flags> -x hip --cuda-device-only -c trace.hip -o new.co     (and old.co at another commit)
    tools/kernel_diff.py old.co new.co [--rename-new PATTERN REPL]... [--rename-old PATTERN REPL]... [--drop-arg N]

Each input is a clang offload bundle (or a bare ELF).  Functions are matched by
demangled name.  For a commit that renames kernels, --rename-new / --rename-old
rewrite the demangled names of that side before matching: re.sub(PATTERN, REPL),
each rule applied to every name, in the order given.  Rules can be kept in a file,
one argument per line, and given as @FILE (kernel_diff_variants.args maps
k_trace<TraceVariant<...>> names back to the ten positional arguments k_trace had
before the descriptor).  --drop-arg N removes the N-th (0-based) template argument
of k_trace<a, b, ...> from the OLD names, for a commit that deleted that parameter.  The
disassembly is compared as text with addresses and encodings stripped.  Lines
that differ only in the literal of the s_add_u32 / s_addc_u32 pair that follows an
s_getpc_b64 are reported apart: those are pc-relative addresses of out-of-line
functions, which move when the code object changes size.  Exit status 1 when
anything else differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def elf_of(path, tmp):
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return path
    targets = [t for t in run(f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={path}").split()
               if "amdgcn" in t]
    out = os.path.join(tmp, os.path.basename(path) + f".{len(os.listdir(tmp))}.elf")
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={targets[0]}", f"--input={path}",
        f"--output={out}")
    return out


def functions(elf):
    """demangled name -> list of instruction lines"""
    text = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", elf)
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        ins = re.sub(r"\s+", " ", ins)
        if ins and ins != "...":   # (objdump's mark for a run of zero bytes: padding behind a function)
            cur.append(ins)
    names = list(funcs)
    dem = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    return {d: funcs[n] for n, d in zip(names, dem.splitlines())}


def pc_relative(ins, i):
    """ins[i] is the s_add_u32 / s_addc_u32 that adds a literal to the low / high half of the
    register pair an s_getpc_b64 wrote at most three instructions earlier"""
    m = re.match(r"(s_add_u32|s_addc_u32) s(\d+), s(\d+), \S+$", ins[i])
    if not m or m.group(2) != m.group(3):
        return False
    reg = int(m.group(2))
    for j in range(max(0, i - 3), i):
        g = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", ins[j])
        if g and reg == int(g.group(1 if m.group(1) == "s_add_u32" else 2)):
            return True
    return False


def drop_arg(name, k):
    m = re.search(r"k_trace<(.*)>\(", name)
    if not m:
        return name
    args = m.group(1).split(", ")
    del args[k]
    return name[:m.start(1)] + ", ".join(args) + name[m.end(1):]


def renamed(funcs, rules):
    out = {}
    for n, body in funcs.items():
        for pat, repl in rules:
            n = re.sub(pat, repl, n)
        if n in out:
            sys.exit(f"rename rules map two functions to {n}")
        out[n] = body
    return out


def main():
    ap = argparse.ArgumentParser(fromfile_prefix_chars="@")
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename-old", nargs=2, action="append", default=[], metavar=("PATTERN", "REPL"))
    ap.add_argument("--rename-new", nargs=2, action="append", default=[], metavar=("PATTERN", "REPL"))
    ap.add_argument("--drop-arg", type=int, default=None)
    ap.add_argument("--drop-value", default="false", help="old k_trace variants whose dropped argument differs are "
                    "expected to have no counterpart")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = functions(elf_of(a.old, tmp)), functions(elf_of(a.new, tmp))
    old, new = renamed(old, a.rename_old), renamed(new, a.rename_new)
    gone = []
    if a.drop_arg is not None:
        kept = {}
        for n, body in old.items():
            m = re.search(r"k_trace<(.*)>\(", n)
            if m and m.group(1).split(", ")[a.drop_arg] != a.drop_value:
                gone.append(n)
                continue
            kept[drop_arg(n, a.drop_arg)] = body
        old = kept
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    same = reloc_only = 0
    bad = []
    for n in sorted(set(old) & set(new)):
        x, y = old[n], new[n]
        if x == y:
            same += 1
            continue
        other = len(x) != len(y)
        if not other:
            for i, (p, q) in enumerate(zip(x, y)):
                if p == q:
                    continue
                if not (p.rsplit(" ", 1)[0] == q.rsplit(" ", 1)[0] and pc_relative(x, i) and pc_relative(y, i)):
                    other = True
                    break
        if other:
            bad.append(n)
        else:
            reloc_only += 1
    kt = lambda d: sum("k_trace<" in n for n in d)
    print(f"old: {len(old) + len(gone)} functions ({kt(old) + len(gone)} k_trace, {len(gone)} dropped with the argument)")
    print(f"new: {len(new)} functions ({kt(new)} k_trace)")
    print(f"identical: {same}; identical but for pc-relative literals: {reloc_only}; different: {len(bad)}")
    for n in bad:
        print("  DIFF", n, len(old[n]), "->", len(new[n]), "instructions")
    for n in only_old:
        print("  only in old:", n)
    for n in only_new:
        print("  only in new:", n)
    return 1 if (bad or only_old or only_new) else 0


if __name__ == "__main__":
    sys.exit(main())
