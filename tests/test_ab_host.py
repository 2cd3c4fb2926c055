"""scripts/ab.py, the same-box A/B runner, driven with a stub child (a few
lines of Python that print one JSON line chosen by a counter file): the
protocol, the statistics, the stopping rule and the checks that the arms
differ.  No GPU; the library is involved only in the last two tests."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = os.path.join(ROOT, "scripts", "ab.py")
LIB = os.path.join(ROOT, "smcdet_amd", "libsmcdet_hip.so")
DIAG = os.path.join(ROOT, "smcdet_amd", "libsmcdet_hip_diag.so")

# invocation i (counted in argv[1]) prints line i of argv[2] (JSON per line, or
# "exit N" / "sleep S" / any other text as it is) and logs "$ARM:<its further
# arguments>" to argv[1].arms
STUB = """
import os, sys, time
n = int(open(sys.argv[1]).read() or 0) if os.path.exists(sys.argv[1]) else 0
open(sys.argv[1], "w").write(str(n + 1))
open(sys.argv[1] + ".arms", "a").write(os.environ.get("ARM", "?") + ":" + ",".join(sys.argv[3:]) + "\\n")
line = open(sys.argv[2]).read().splitlines()[n]
print("some earlier output", flush=True)
if line.startswith("exit "):
    sys.exit(int(line[5:]))
if line.startswith("sleep "):
    time.sleep(float(line[6:]))
print(line)
"""


def run_ab(tmp_path, lines, *args, arms=("a,ARM=a", "b,ARM=b"), out=True):
    """ab.py over the stub with `lines` as its script; returns (CompletedProcess,
    invocations, the arms in invocation order, table text or None)."""
    (tmp_path / "stub.py").write_text(STUB)
    (tmp_path / "lines").write_text("\n".join(lines) + "\n")
    cnt = tmp_path / "count"
    for f in (cnt, tmp_path / "count.arms", tmp_path / "new" / "ab.txt"):
        f.unlink(missing_ok=True)
    cmd = [sys.executable, AB, "--cmd",
           f"{sys.executable} {tmp_path / 'stub.py'} {cnt} {tmp_path / 'lines'}"]
    for s in arms:
        cmd += ["--arm", s]
    if out:
        cmd += ["--out", str(tmp_path / "new" / "ab.txt")]
    r = subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=120)
    n = int(cnt.read_text()) if cnt.exists() else 0
    order = (tmp_path / "count.arms").read_text().split() if n else []
    tab = (tmp_path / "new" / "ab.txt").read_text() if (tmp_path / "new" / "ab.txt").exists() else None
    return r, n, order, tab


def ms(*pairs):
    return [json.dumps({"ms_per_step": v, "roofline": {"kernel_ms": v / 2}})
            for p in pairs for v in p]


def test_order_discard_and_statistics(tmp_path):
    """Arm order within pairs, r0 discarded, and the statistics on known
    numbers: b is lower in 3 of 4 kept pairs, the ranges overlap, and b's
    median lies within a's median +- a's own range."""
    pairs = [(9.0, 1.0), (1.00, 0.98), (1.04, 1.01), (1.02, 1.03), (1.06, 0.99)]
    r, n, order, tab = run_ab(tmp_path, ms(*pairs), "--pairs", "5")
    assert r.returncode == 0, r.stderr
    assert n == 10 and order == ["a:", "b:"] * 5
    assert all(ln in r.stdout for ln in tab.splitlines())  # the file is what was printed
    rows = [ln for ln in tab.splitlines() if ln.startswith("r")]
    assert len(rows) == 5 and rows[0].endswith("(discarded)") and "9.0000" in rows[0]
    assert not any("discarded" in x for x in rows[1:])
    # kept: a = 1.00 1.04 1.02 1.06, b = 0.98 1.01 1.03 0.99
    assert "a  median 1.0300  range 1.0000-1.0600  (n = 4)" in tab
    assert "b  median 1.0000  range 0.9800-1.0300  (n = 4)" in tab
    assert "b's median vs a's: -2.91%; lower in 3 of 4 pairs; ranges overlap" in tab
    assert "a's median +- its own min-to-max range 0.0600 = 0.9700..1.0900: b's median is within" in tab
    assert "INCOMPLETE" not in tab
    # every run's full line is kept beside the table
    runs = [json.loads(x) for x in (tmp_path / "new" / "ab.runs.jsonl").read_text().splitlines()]
    assert [(x["pair"], x["arm"]) for x in runs] == [(p, a) for p in range(5) for a in "ab"]
    assert runs[0]["discarded"] and not runs[2]["discarded"]
    assert runs[3]["line"] == {"ms_per_step": 0.98, "roofline": {"kernel_ms": 0.49}}
    # the header records the command, the arms and the discard rule
    assert "stub.py" in tab and "arm a (baseline): " in tab and "environment ARM=b" in tab
    assert "pair r0 is run and discarded" in tab


def test_disjoint_ranges_and_median_outside(tmp_path):
    """b above a in every kept pair: ranges disjoint, lower in 0 of 3, and its
    median outside a's median +- a's range; the default is 6 pairs."""
    pairs = [(1.0, 1.0), (1.00, 1.10), (1.02, 1.12), (1.01, 1.11)]
    r, n, order, tab = run_ab(tmp_path, ms(*pairs), "--pairs", "4")
    assert r.returncode == 0, r.stderr
    assert "b's median vs a's: +9.90%; lower in 0 of 3 pairs; ranges disjoint" in tab
    assert "range 0.0200 = 0.9900..1.0300: b's median is outside" in tab
    # three arms, default pair count: 6 pairs of 3 runs, the baseline first
    r, n, order, tab = run_ab(tmp_path, ms(*[(1.0, 2.0, 0.5)] * 6),
                              arms=("a,ARM=a", "b,ARM=b", "c,ARM=c"))
    assert r.returncode == 0 and n == 18 and order == ["a:", "b:", "c:"] * 6
    assert "b's median vs a's: +100.00%" in tab and "c's median vs a's: -50.00%" in tab


@pytest.mark.parametrize("line,args,status", [("exit 134", (), 134), ("sleep 30", ("--limit", "1"), 124)])
def test_stops_at_the_first_abnormal_exit(tmp_path, line, args, status):
    """The third child aborts (or outlives its limit): ab.py passes its status
    on, starts nothing more, and writes no table as complete."""
    lines = ms((1.0, 1.0)) + [line] + ms((1.0, 1.0), (1.0, 1.0))
    r, n, order, tab = run_ab(tmp_path, lines, "--pairs", "3", *args)
    assert r.returncode == status, (r.returncode, r.stderr)
    assert n == 3 and order == ["a:", "b:", "a:"]
    assert "some earlier output" in r.stdout  # the tail of the child's output
    assert "nothing more is started" in r.stderr
    assert "INCOMPLETE: pair r1 arm a exited with status %d" % status in tab
    assert "median" not in tab


def test_identical_arms_are_refused(tmp_path):
    r, n, _, tab = run_ab(tmp_path, ms((1.0, 1.0)), arms=("a", "b"))
    assert r.returncode == 2 and n == 0 and tab is None
    assert "identical" in r.stderr and "--allow-identical" in r.stderr
    # the same settings under two labels, and the same arguments, are identical too
    r, n, _, _ = run_ab(tmp_path, ms((1.0, 1.0)), arms=("a,ARM=x,--k,1", "b,ARM=x,--k,1"))
    assert r.returncode == 2 and n == 0
    r, n, order, tab = run_ab(tmp_path, ms((1.0, 1.0), (1.0, 1.0)), "--pairs", "2",
                              "--allow-identical", arms=("a", "b"))
    assert r.returncode == 0 and n == 4, r.stderr
    # arguments alone make arms differ, and reach the child after the common ones
    r, n, order, _ = run_ab(tmp_path, ms((1.0, 1.0), (1.0, 1.0)), "--pairs", "2", "--", "-c",
                            arms=("a", "b,--k,1"))
    assert r.returncode == 0 and order == ["?:-c", "?:-c,--k,1"] * 2, (r.stderr, order)


def test_dotted_metrics_and_a_last_line_that_is_not_json(tmp_path):
    pairs = [(1.0, 1.0), (2.0, 4.0), (2.0, 4.0)]
    r, n, _, tab = run_ab(tmp_path, ms(*pairs), "--pairs", "3", "--metric", "roofline.kernel_ms",
                          "--metric", "ms_per_step")
    assert r.returncode == 0, r.stderr
    judged, other = tab.split("\nms_per_step\n")
    assert "roofline.kernel_ms (the metric judged)" in judged
    assert "a  median 1.0000" in judged and "b  median 2.0000" in judged
    assert "a  median 2.0000" in other and "b  median 4.0000" in other
    # a run without the metric, or whose last line is no JSON, is an error, not a skipped run
    for bad in ("done.", json.dumps({"value": 3})):
        r, n, _, tab = run_ab(tmp_path, ms((1.0, 1.0)) + [bad] + ms((1.0, 1.0)), "--pairs", "3")
        assert r.returncode == 2 and n == 3, (bad, r.returncode, n)
        assert "no metric in the last stdout line" in r.stderr
        assert "INCOMPLETE" in tab and "median" not in tab


def test_diagnostic_only_settings_need_the_diagnostic_build(tmp_path):
    """SMCDET_MH_BLOCK_SLOTS (and the diagnostic MH flags) on the product
    library would time the same kernel twice: refused; the diagnostic build
    takes them."""
    if not (os.path.exists(LIB) and os.path.exists(DIAG)):
        pytest.skip("libraries not built")
    r, n, _, _ = run_ab(tmp_path, ms((1.0, 1.0)), arms=("a", f"b,lib={LIB},SMCDET_MH_BLOCK_SLOTS=4"))
    assert r.returncode == 2 and n == 0
    assert "SMCDET_MH_BLOCK_SLOTS" in r.stderr and "libsmcdet_hip_diag.so" in r.stderr
    r, n, _, _ = run_ab(tmp_path, ms((1.0, 1.0)), arms=("a", "b,--mh-debug-flags,1024"))
    assert r.returncode == 2 and n == 0 and "--mh-debug-flags bits 1024" in r.stderr
    r, n, _, tab = run_ab(tmp_path, ms((1.0, 1.0), (1.0, 1.0)), "--pairs", "2",
                          arms=(f"a,lib={DIAG}", f"b,lib={DIAG},SMCDET_MH_BLOCK_SLOTS=4"))
    assert r.returncode == 0 and n == 4, r.stderr
    assert "(gfx950, diag)" in tab  # the header carries smcdet_version()
    # a flag the product takes (32768, the generic-geometry A/B) is no reason to refuse
    r, n, _, _ = run_ab(tmp_path, ms((1.0, 1.0), (1.0, 1.0)), "--pairs", "2",
                        arms=("a", "b,--mh-debug-flags,32768"))
    assert r.returncode == 0 and n == 4, r.stderr


def test_microbench_names_the_diagnostic_build_before_any_device_call():
    """scripts/mh_microbench.py --variants scalar_slots on the product library
    stops before it touches the device (the exit is the same with and without
    a GPU) and says which library has the variant."""
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    env = {k: v for k, v in os.environ.items() if k != "SMCDET_HIP_LIB"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mh_microbench.py"),
                        "--variants", "scalar_slots"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode != 0 and r.stdout == ""
    assert "scalar_slots" in r.stderr and "SMCDET_HIP_LIB=" in r.stderr
    assert "libsmcdet_hip_diag.so" in r.stderr
