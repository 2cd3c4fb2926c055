#!/usr/bin/env python
"""Is the gfx950 device code of two source trees the same?  For host-only
refactors: compiles the named sources of both trees device-only, takes the
gfx950 ELF out of the bundle and compares its disassembly (llvm-objdump -d,
without the file-name header) and its notes (llvm-readelf --notes: kernel
symbols, registers, LDS, kernarg layout).  Raw ELF bytes are not compared: two
builds of one source differ in the __hip_cuid_* symbol.  It only diffs.

    python scripts/device_code_equal.py PARENT_TREE . --builds product diag trace \\
        --sources mh_kernel.hip > profiles/dispatch/device_code_equal.txt

--per-kernel, for changes that add instantiations to a translation unit (the
whole code objects then differ: more kernels, other addresses, and a template
argument more in every symbol): for every kernel of tree a, tree b must have a
kernel with the same instruction stream (mnemonics, operands and encodings in
order; addresses and the symbol+offset comments of branches dropped) and the
same resource notes (every field of its amdhsa.kernels entry but .name and
.symbol).  --changed NAME... names kernels (substring of the symbol) that are
meant to change: they are listed, not counted.

    python scripts/device_code_equal.py PARENT_TREE . --per-kernel --builds product diag \\
        --sources mh_kernel.hip mala_kernel.hip model_kernels.hip \\
        --changed log_prior_kernel prior_sample_kernel
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
BUILDS = {"product": [], "diag": ["-DSMCDET_DIAG"], "trace": ["-DSMCDET_TRACE"]}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\n{r.stderr[-4000:]}")
    return r.stdout


def device_text(tree, source, defines, work):
    """(disassembly lines, notes lines) of the tree's source, file names removed."""
    obj, elf = os.path.join(work, "bundle.o"), os.path.join(work, "gfx950.elf")
    run([os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
         "--cuda-device-only", *defines, "-c",
         os.path.join(tree, "smcdet_amd", "csrc", source), "-o", obj])
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
         f"--targets={TARGET}", f"--input={obj}", f"--output={elf}"])
    dis = [l for l in run([os.path.join(LLVM, "llvm-objdump"), "-d", elf]).splitlines()
           if "file format" not in l]
    notes = [l for l in run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf]).splitlines()
             if elf not in l]
    return dis, notes


def kernel_streams(dis):
    """{symbol: tuple of instruction lines without addresses} of a disassembly."""
    out, cur = {}, None
    for l in dis:
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", l)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and l.strip():
            text, _, enc = l.partition("//")
            enc = enc.split(":", 1)[-1].split("<", 1)[0]  # the encoding words
            cur.append(text.strip() + " | " + " ".join(enc.split()))
    return {k: tuple(v) for k, v in out.items()}


def kernel_notes(notes):
    """{kernel name: tuple of its amdhsa.kernels entry's lines but .name / .symbol}."""
    out, entry, inside = {}, None, False

    def close():
        if entry:
            name = next(l.split()[-1] for l in entry if l.strip().startswith(".name:"))
            out[name] = tuple(l for l in entry
                              if not l.strip().startswith((".name:", ".symbol:")))
    for l in notes:
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and l.startswith("  - "):
            close()
            entry = [l.replace("  - ", "    ", 1)]
        elif inside and l.startswith("    "):
            entry.append(l)
        elif inside:
            close()
            entry, inside = None, False
    close()
    return out


def per_kernel(text_a, text_b, changed):
    """Lines of the report and the number of tree a's kernels without a twin."""
    (dis_a, notes_a), (dis_b, notes_b) = text_a, text_b
    sa, sb, na, nb = (kernel_streams(dis_a), kernel_streams(dis_b), kernel_notes(notes_a),
                      kernel_notes(notes_b))
    twins = {}
    for k, v in sb.items():
        if k in nb:
            twins.setdefault((v, nb[k]), []).append(k)
    lines, missing = [], 0
    for k in sorted(na):
        hit = twins.get((sa[k], na[k]))
        if hit:
            lines.append(f"    same  {len(sa[k]):6d} instr  {k}\n          -> {hit[0]}")
        elif any(c in k for c in changed):
            lines.append(f"    meant to change  {k}")
        else:
            missing += 1
            near = [j for j in sb if sb[j] == sa[k]]
            lines.append(f"    NO TWIN  {k}" + (f"  (stream of {near[0]}, notes differ)"
                                                if near else ""))
    new = sorted(set(nb) - {h for hs in twins.values() for h in hs
                            if any((sa[k], na[k]) == (sb[h], nb[h]) for k in na)})
    for k in new:
        lines.append(f"    new   {len(sb[k]):6d} instr  {k}")
    return lines, missing


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--builds", nargs="+", default=list(BUILDS), choices=list(BUILDS))
    ap.add_argument("--sources", nargs="+", default=["mh_kernel.hip"])
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--per-kernel", action="store_true",
                    help="every kernel of tree a has a twin in tree b (see above)")
    ap.add_argument("--changed", nargs="*", default=[],
                    help="--per-kernel: kernels meant to change (substrings of the symbol)")
    a = ap.parse_args()
    jobs = [(s, b, t) for s in a.sources for b in a.builds for t in (a.tree_a, a.tree_b)]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as pool:
        def one(i):
            s, b, t = jobs[i]
            work = os.path.join(tmp, str(i))
            os.mkdir(work)
            return device_text(t, s, BUILDS[b], work)
        texts = list(pool.map(one, range(len(jobs))))
    print("device code of tree a (the parent) and tree b, hipcc -O3 -std=c++17 -fPIC "
          "--offload-arch=gfx950 --cuda-device-only;\nllvm-objdump -d and llvm-readelf --notes "
          "of the unbundled gfx950 ELF\n")
    differ = 0
    if a.per_kernel:
        for i in range(0, len(jobs), 2):
            s, b, _ = jobs[i]
            lines, missing = per_kernel(texts[i], texts[i + 1], a.changed)
            differ += missing
            print(f"{s:<24} {b:<8} per kernel: "
                  f"{'every kernel of tree a has a twin' if not missing else f'{missing} WITHOUT A TWIN'}")
            print("\n".join(lines))
        print("\nevery kernel of tree a is in tree b with the same instruction stream and resource "
              "notes" if not differ else f"\n{differ} kernel(s) of tree a WITHOUT A TWIN in tree b")
        return 1 if differ else 0
    for i in range(0, len(jobs), 2):
        s, b, _ = jobs[i]
        (dis_a, notes_a), (dis_b, notes_b) = texts[i], texts[i + 1]
        kernels = sum(1 for l in notes_b if re.match(r"\s+\.symbol:\s+\S+\.kd", l))
        same_d, same_n = dis_a == dis_b, notes_a == notes_b
        print(f"{s:<24} {b:<8} {kernels:4d} kernels  {len(dis_b):8d} disassembly lines "
              f"{'identical' if same_d else 'DIFFER'}   {len(notes_b):6d} notes lines "
              f"{'identical' if same_n else 'DIFFER'}")
        for same, x, y in ((same_d, dis_a, dis_b), (same_n, notes_a, notes_b)):
            if not same:
                differ += 1
                for l in list(difflib.unified_diff(x, y, "a", "b", n=0, lineterm=""))[:40]:
                    print("    " + l)
    print("\nall identical" if not differ else f"\n{differ} comparison(s) DIFFER")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
