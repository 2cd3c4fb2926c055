"""scripts/README.md indexes scripts/: every file there has a line, and every
`scripts/<name>` the documents, the Makefile, the tests, the package and the
scripts themselves mention either exists or is in the README's retired table
(DESIGN.md keeps retired names as the provenance of recorded numbers)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
README = open(os.path.join(SCRIPTS, "README.md")).read()


def script_files():
    """Files under scripts/, relative to it, without Python's caches and the
    programs built from a probe's source beside them (`x` next to `x.hip`)."""
    names = [os.path.join(d, f) for d, _, fs in os.walk(SCRIPTS) if "__pycache__" not in d
             for f in fs if not os.path.exists(os.path.join(d, f + ".hip"))]
    return sorted(os.path.relpath(p, SCRIPTS) for p in names)


def retired():
    sec = README.split("## Retired", 1)[1]
    return set(re.findall(r"^\| `([^`]+)` \|", sec, re.M))


def test_every_script_has_an_index_line():
    index = README.split("## Index", 1)[1].split("## Retired", 1)[0]
    listed = set(re.findall(r"^\| `([^`]+)` \|", index, re.M))
    files = script_files()
    assert len(files) > 30
    assert [f for f in files if f not in listed] == []
    assert [x for x in listed if not os.path.exists(os.path.join(SCRIPTS, x))] == []
    assert sorted(f for f in files if f.endswith(".sh")) == ["build_rev.sh", "gpu_pass.sh",
                                                             "profile.sh"]
    assert not retired() & set(files)


def test_every_mention_of_a_script_exists_or_is_retired():
    where = [os.path.join(ROOT, n) for n in ("README.md", "INTEGRATION.md", "DESIGN.md", "Makefile")]
    where += glob.glob(os.path.join(ROOT, "tests", "*.py"))
    where += glob.glob(os.path.join(ROOT, "smcdet_amd", "*.py"))
    where += [os.path.join(SCRIPTS, f) for f in script_files()]
    gone = retired()
    assert len(gone) >= 46
    missing = []
    for path in where:
        with open(path, errors="replace") as f:
            txt = f.read()
        for name in set(re.findall(r"scripts/([A-Za-z0-9_][A-Za-z0-9_./-]*[A-Za-z0-9_])", txt)):
            # (a program named without its suffix is what its source here builds)
            if not (os.path.exists(os.path.join(SCRIPTS, name)) or name in gone
                    or os.path.exists(os.path.join(SCRIPTS, name + ".hip"))):
                missing.append((os.path.relpath(path, ROOT), name))
    assert missing == []
