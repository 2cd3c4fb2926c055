#!/usr/bin/env python3
"""Same-box A/B runner: the procedure of the committed records
(profiles/geometry/ab.txt, profiles/headtail/ab.txt, profiles/dispatch/ab.txt).

    scripts/ab.py --arm parent,lib=smcdet_amd/libsmcdet_hip_parent.so --arm tree \\
        [--pairs 6] [--limit 240] [--metric ms_per_step] [--out profiles/x/ab.txt] \\
        [--cmd "python scripts/mh_microbench.py --no-extra"] [-- common arguments]

An arm is `LABEL[,item]...`; the first arm is the baseline.  Items:
    lib=PATH     the library (exported as SMCDET_HIP_LIB, absolute; with
                 SMCDET_ALLOW_STALE=1 when it was built from other sources than
                 this tree's); without it the arm runs smcdet_amd/libsmcdet_hip.so
    NAME=VALUE   an environment setting (NAME in capitals)
    anything else, in order: an extra command argument (`c4,--workload,c4`)

In every pair each arm runs once, in arm order, one child process at a time,
each under its own `timeout -k 10 <limit>`, from the repository root.  Pair r0
is run, printed and discarded.  The first child that exits non-zero ends the
run: nothing more is started, the tail of its output is printed and its status
is this tool's (no retry).  The metric is read from the child's last stdout
line, which must be JSON (bench.py's line); `--metric a.b.c` is a dotted path,
and of several the first is the one judged.

Before the first run the arms are checked to differ (library bytes, settings,
arguments) and to be able to differ: a setting or MH flag that only the
diagnostic build reads is refused on any other library.  The table states
medians, ranges and how they lie; it sets no threshold.

Only the standard library is imported here, and neither torch nor the package:
this process never loads the HIP runtime.
"""
import argparse
import hashlib
import json
import os
import re
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "smcdet_amd", "libsmcdet_hip.so")

# What only the diagnostic build (make diag, "(gfx950, diag)" in smcdet_version())
# reads.  The settings: the two `#ifdef SMCDET_DIAG` getenv sites,
# smcdet_amd/csrc/mh_kernel.hip (SMCDET_MH_BLOCK_SLOTS, in the launch plan's
# set-up) and smcdet_amd/csrc/smc_kernels.hip (SMCDET_TILE_THREADS,
# tile_threads()).  The flags: the gate at the head of mh_sweep_impl
# (ablations 256 / 512, scalar slots 1024, no 1/v cache 4096, PSF table 8192).
DIAG_ENV = ("SMCDET_MH_BLOCK_SLOTS", "SMCDET_TILE_THREADS")
DIAG_MH_FLAGS = 256 | 512 | 1024 | 4096 | 8192

_VERSION_CHILD = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); "
                  "L.smcdet_version.restype = ctypes.c_char_p; "
                  "print(L.smcdet_version().decode())")


class Refused(Exception):
    """The run is not started (exit status 2)."""


def tree_source_hash():
    """sha1 of the library's sources here, in the Makefile's SRCS + HDRS order
    (what `make` compiles into smcdet_version()); None without them."""
    try:
        mk = open(os.path.join(ROOT, "Makefile")).read()
        names = " ".join(re.search(rf"^{k} := (.*)$", mk, re.M).group(1) for k in ("SRCS", "HDRS"))
        h = hashlib.sha1()
        for n in names.replace("$(CSRC)", "smcdet_amd/csrc").split():
            with open(os.path.join(ROOT, n), "rb") as f:
                h.update(f.read())
        return h.hexdigest()
    except (OSError, AttributeError):
        return None


def library_version(path):
    """smcdet_version() of the library at `path`, asked of a short-lived child."""
    r = subprocess.run([sys.executable, "-c", _VERSION_CHILD, path], capture_output=True,
                       text=True, timeout=120)
    if r.returncode != 0:
        raise Refused(f"{path} does not load: {r.stderr.strip()[-400:]}")
    return r.stdout.strip()


class Arm:
    def __init__(self, spec):
        label, *items = spec.split(",")
        if not label or "=" in label:
            raise Refused(f"--arm {spec!r}: the first item is the arm's label")
        self.label, self.lib_given, self.env, self.args = label, None, {}, []
        for it in items:
            if it.startswith("lib="):
                self.lib_given = os.path.abspath(it[4:])
            elif re.match(r"[A-Z_][A-Z0-9_]*=", it):
                k, v = it.split("=", 1)
                self.env[k] = v
            else:
                self.args.append(it)
        # the library the children of this arm load (None: a --cmd that needs none)
        self.lib = self.lib_given or (DEFAULT_LIB if os.path.exists(DEFAULT_LIB) else None)
        self.sha1 = self.version = None
        if self.lib_given and not os.path.exists(self.lib_given):
            raise Refused(f"arm {label}: no library at {self.lib_given}")
        if self.lib:
            with open(self.lib, "rb") as f:
                self.sha1 = hashlib.sha1(f.read()).hexdigest()
            self.version = library_version(self.lib)

    @property
    def is_diag(self):
        return bool(self.version) and ", diag)" in self.version

    def child_env(self, tree_hash):
        e = dict(os.environ)
        e.pop("SMCDET_HIP_LIB", None)  # the arms decide, not the caller's shell
        e.pop("SMCDET_ALLOW_STALE", None)
        e.update(self.env)
        if self.lib_given:
            e["SMCDET_HIP_LIB"] = self.lib_given
            if "src " not in self.version or self.version.rsplit("src ", 1)[-1] != tree_hash:
                e["SMCDET_ALLOW_STALE"] = "1"
        return e

    def describe(self):
        lib = "none" if not self.lib else (
            f"{os.path.relpath(self.lib, ROOT)} sha1 {self.sha1} \"{self.version}\"")
        env = " ".join(f"{k}={v}" for k, v in self.env.items()) or "-"
        return f"library {lib}; environment {env}; arguments {shlex.join(self.args) or '-'}"


def mh_debug_flags(argv):
    """The value of --mh-debug-flags in an argument list (0 if absent)."""
    v = 0
    for i, a in enumerate(argv):
        if a == "--mh-debug-flags" and i + 1 < len(argv):
            v = int(argv[i + 1], 0)
        elif a.startswith("--mh-debug-flags="):
            v = int(a.split("=", 1)[1], 0)
    return v


def check_arms(arms, cmd_args, allow_identical):
    if len(arms) < 2:
        raise Refused("an A/B needs two or more --arm")
    if len({a.label for a in arms}) < len(arms):
        raise Refused("arm labels must be distinct")
    for a in arms:
        need = [k for k in DIAG_ENV if k in a.env]
        fl = mh_debug_flags(cmd_args + a.args) & DIAG_MH_FLAGS
        if fl:
            need.append(f"--mh-debug-flags bits {fl}")
        if need and not a.is_diag:
            raise Refused(
                f"arm {a.label}: {', '.join(need)} is read by the diagnostic build only, and "
                f"its library ({a.version or 'none'}) is not one: the arm would run the same "
                "kernels as without it.  Give it lib=smcdet_amd/libsmcdet_hip_diag.so (make diag)")
    if not allow_identical:
        seen = {}
        for a in arms:
            key = (a.sha1, tuple(sorted(a.env.items())), tuple(a.args))
            if key in seen:
                raise Refused(
                    f"arms {seen[key]} and {a.label} are identical (same library bytes, "
                    "environment and arguments): the comparison would be of a thing with itself; "
                    "--allow-identical runs it as an A/A")
            seen[key] = a.label


def lookup(doc, path):
    for k in path.split("."):
        doc = doc[int(k)] if isinstance(doc, list) else doc[k]
    if isinstance(doc, bool) or not isinstance(doc, (int, float)):
        raise TypeError(f"{path} is not a number")
    return float(doc)


def num(v):
    return f"{v:.4f}" if abs(v) < 1e4 else f"{v:.6g}"


def table(metric, labels, rows):
    """The block of one metric: rows[pair][arm] (complete pairs and, last,
    possibly a partial one), then the statistics over the kept pairs r1..."""
    w = max(12, *(len(x) + 2 for x in labels))
    out = ["pair  " + "".join(f"{x:>{w}}" for x in labels)]
    for i, row in enumerate(rows):
        out.append(f"r{i:<5d}" + "".join(f"{num(v):>{w}}" for v in row)
                   + ("   (discarded)" if i == 0 else ""))
    kept = [r for r in rows[1:] if len(r) == len(labels)]
    if not kept:
        return out
    lw = max(len(x) for x in labels)
    cols = [[r[j] for r in kept] for j in range(len(labels))]
    med = [statistics.median(c) for c in cols]
    for j, x in enumerate(labels):
        out.append(f"  {x:<{lw}}  median {num(med[j])}  range {num(min(cols[j]))}-"
                   f"{num(max(cols[j]))}  (n = {len(kept)})")
    b, base = labels[0], cols[0]
    span = max(base) - min(base)
    for j in range(1, len(labels)):
        c, x = cols[j], labels[j]
        lower = sum(1 for p, q in zip(base, c) if q < p)
        disjoint = max(c) < min(base) or min(c) > max(base)
        inside = med[0] - span <= med[j] <= med[0] + span
        pct = f"{100.0 * (med[j] / med[0] - 1.0):+.2f}%" if med[0] else "n/a"
        out.append(f"  {x}'s median vs {b}'s: {pct}; lower in {lower} of {len(kept)} pairs; "
                   f"ranges {'disjoint' if disjoint else 'overlap'}")
        out.append(f"  {b}'s median +- its own min-to-max range {num(span)} = "
                   f"{num(med[0] - span)}..{num(med[0] + span)}: {x}'s median is "
                   f"{'within' if inside else 'outside'}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arm", action="append", default=[], metavar="LABEL[,lib=PATH][,NAME=VALUE][,ARG]")
    ap.add_argument("--pairs", type=int, default=6, help="pairs run, r0 included (default 6)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child (timeout -k 10)")
    ap.add_argument("--metric", action="append", default=[], help="dotted path; the first is judged")
    ap.add_argument("--cmd", default=None, help="replaces `python bench.py`")
    ap.add_argument("--out", default=None, help="table file; the runs' lines go to <out>.runs.jsonl")
    ap.add_argument("--allow-identical", action="store_true", help="an A/A run")
    ap.add_argument("common", nargs="*", help="after --: arguments of every arm's command")
    a = ap.parse_args(argv)
    metrics = a.metric or ["ms_per_step"]
    cmd = shlex.split(a.cmd) if a.cmd else [sys.executable, "bench.py"]
    if a.pairs < 2:
        ap.error("--pairs counts the discarded r0: at least 2")
    try:
        arms = [Arm(s) for s in a.arm]
        check_arms(arms, cmd + a.common, a.allow_identical)
    except Refused as e:
        print(f"ab.py: refused: {e}", file=sys.stderr)
        return 2
    labels = [x.label for x in arms]
    tree_hash = tree_source_hash()
    shown = shlex.join((["python"] if not a.cmd else cmd[:1]) + cmd[1:] + a.common)
    head = [f"Same-box A/B (scripts/ab.py): `{shown}`, {a.pairs} pairs; in each pair every arm runs "
            f"once, in the order below, one process at a time under `timeout -k 10 {a.limit}`; "
            "pair r0 is run and discarded.",
            f"sources of this tree: sha1 {tree_hash}"]
    head += [f"arm {x.label}{' (baseline)' if i == 0 else ''}: {x.describe()}"
             for i, x in enumerate(arms)]
    print("\n".join(head), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    runs = open(os.path.splitext(a.out)[0] + ".runs.jsonl", "w") if a.out else None
    rows = {m: [] for m in metrics}  # metric -> [pair][arm]

    def report(status):
        txt = list(head)
        for i, m in enumerate(metrics):
            txt += ["", m + (" (the metric judged)" if i == 0 and len(metrics) > 1 else "")]
            txt += table(m, labels, rows[m])
        if status:
            txt += ["", f"INCOMPLETE: {status}; no statistics are to be read from this file"]
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(txt) + "\n")
        return txt

    def stop(status, rc, tail=""):
        if tail:
            print(tail, flush=True)
        print(f"ab.py: {status}; nothing more is started", file=sys.stderr)
        report(status)
        return rc

    for p in range(a.pairs):
        for m in metrics:
            rows[m].append([])
        for x in arms:
            who = f"pair r{p} arm {x.label}"
            r = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd + a.common + x.args,
                               cwd=ROOT, env=x.child_env(tree_hash), stdin=subprocess.DEVNULL,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               errors="replace")
            lines = r.stdout.strip().splitlines()
            if r.returncode != 0:
                rc = r.returncode if r.returncode > 0 else 128 - r.returncode
                tail = "\n".join(lines[-15:] + r.stderr.strip().splitlines()[-25:])
                return stop(f"{who} exited with status {rc}", rc, tail)
            try:
                doc = json.loads(lines[-1])
                vals = [lookup(doc, m) for m in metrics]
            except (IndexError, ValueError, KeyError, TypeError) as e:
                return stop(f"{who}: no metric in the last stdout line "
                            f"({type(e).__name__}: {e})", 2, "\n".join(lines[-5:]))
            if runs:
                runs.write(json.dumps({"pair": p, "arm": x.label, "discarded": p == 0,
                                       "line": doc}) + "\n")
                runs.flush()
            for m, v in zip(metrics, vals):
                rows[m][-1].append(v)
        print(f"r{p}: " + "  ".join(f"{x} {num(v)}" for x, v in zip(labels, rows[metrics[0]][-1]))
              + ("   (discarded)" if p == 0 else ""), flush=True)
    print("\n".join(report(None)[len(head):]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
