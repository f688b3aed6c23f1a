#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of sources instruction by instruction (a
refactor that must not change machine code):
  python tools/kasm_diff.py OLD.hip [...] -- NEW.hip [...] [--map REGEX=REPL ...] [-v]
A .hip argument is compiled to device assembly with the Makefile's flags, a .s one is
read as it is.  Kernels are matched by demangled name without the parameter list,
after every --map rewrite of the old names (for a removed template parameter, e.g.
--map 'conv2_wgrad_x9_kernel<(\\d+), 0>=conv2_wgrad_x9_kernel<\\1>').  A kernel's text
is its instruction stream and its .amdhsa_kernel block, with function-local labels
renumbered and its own mangled name (also inside its LDS symbols) replaced.  Prints
the kernels that differ (-v: a unified diff), those on one side only, and for every
matched kernel whose resources differ the kres.py numbers of both sides."""
import difflib
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-fvisibility=hidden", "--cuda-device-only", "-S", "-x", "hip"]
RES = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")


def asm_of(path):
    if path.endswith(".s"):
        return open(path).read()
    extra = ["-ffp-contract=off"] if re.search(r"(gae|obs)\.hip$", path) else []
    return subprocess.run([CLANG, *FLAGS, *extra, path, "-o", "-"], capture_output=True, text=True, check=True).stdout


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def strip_params(d):
    if not d.endswith(")"):
        return d
    depth = 0
    for i in range(len(d) - 1, -1, -1):
        depth += d[i] == ")"
        depth -= d[i] == "("
        if depth == 0:
            return d[:i]
    return d


def kernels(paths):
    """{mangled name: (normalised text, resources)} over all the files"""
    with ThreadPoolExecutor(8) as ex:
        asms = list(ex.map(asm_of, paths))
    out = {}
    for asm in asms:
        meta = asm[asm.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in asm else ""
        res = {}
        for blk in re.split(r"\n  - ", meta)[1:]:
            f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)", blk, re.M))
            res[f.get("name")] = tuple(f.get(k) for k in RES)
        for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel", asm, re.M | re.S):
            name = m.group(1)
            body = re.search(r"^%s:.*?^\t\.size\t%s," % (re.escape(name), re.escape(name)), asm, re.M | re.S)
            text = (body.group(0) if body else "") + "\n" + m.group(0)
            text = text.replace(name, "@SELF").replace(name[2:], "@SELF")
            text = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+", r".\1", text)
            text = re.sub(r"[ \t]*;.*$", "", text, flags=re.M)   # comments carry function numbers
            text = re.sub(r"\n{2,}", "\n", text)
            out[name] = (text, res.get(name))
    return out


def main():
    args = sys.argv[1:]
    verbose = "-v" in args
    args = [a for a in args if a != "-v"]
    maps = []
    while "--map" in args:
        i = args.index("--map")
        pat, repl = args[i + 1].split("=", 1)
        maps.append((re.compile(pat), repl))
        del args[i:i + 2]
    sep = args.index("--")
    old, new = kernels(args[:sep]), kernels(args[sep + 1:])
    dm = demangle(list(old) + list(new))

    def key(n, is_old):
        k = strip_params(dm[n])
        if is_old:
            for pat, repl in maps:
                k = pat.sub(repl, k)
        return k

    ok = {key(n, True): n for n in old}
    nk = {key(n, False): n for n in new}
    same = differ = 0
    for k in sorted(ok):
        if k not in nk:
            continue
        (ta, ra), (tb, rb) = old[ok[k]], new[nk[k]]
        if ta == tb:
            same += 1
        else:
            differ += 1
            print(f"DIFFERS  {k}")
            if verbose:
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(ta.split("\n"), tb.split("\n"), "old", "new",
                                                                             n=1, lineterm=""))
        if ra != rb:
            print(f"RESOURCES {k}\n  old {dict(zip(RES, ra or ()))}\n  new {dict(zip(RES, rb or ()))}")
    for k in sorted(set(ok) - set(nk)):
        print(f"ONLY OLD {k}")
    for k in sorted(set(nk) - set(ok)):
        print(f"ONLY NEW {k}")
    print(f"{same} kernels identical, {differ} differ, {len(set(ok) - set(nk))} only old, {len(set(nk) - set(ok))} only new")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
