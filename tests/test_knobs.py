"""The engine's environment variables: read_knobs() in engine.hip reads exactly
the documented test hooks, a test sets every one of them, and nothing else in
the native sources reads the environment but two diagnostics (no GPU needed:
the sources are read as text)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rna_clique_amd", "csrc")
DIAGNOSTICS = {"RC_OUT_TIMING", "RC_PICKLE_MMAP"}


def _read(path):
    with open(path) as f:
        return f.read()


def _body(src, head):
    """The brace-enclosed block that follows `head` in src."""
    i = src.index("{", src.index(head))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
        j += 1


def _knobs_read():
    return set(re.findall(r'"(RC_[A-Z0-9_]+)"', _body(_read(os.path.join(CSRC, "engine.hip")), "Knobs read_knobs()")))


def test_knobs_read_are_the_knobs_documented():
    documented = set(re.findall(r"//\s*(RC_[A-Z0-9_]+)\b", _body(_read(os.path.join(CSRC, "engine.h")),
                                                                  "struct Knobs")))
    assert _knobs_read() and _knobs_read() == documented


def test_every_knob_is_set_by_a_test():
    tests = "".join(_read(p) for p in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True))
    unset = sorted(k for k in _knobs_read() if 'setenv("%s"' % k not in tests)
    assert not unset, unset


def test_environment_is_read_nowhere_else():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        src = _read(path)
        if os.path.basename(path) == "engine.hip":
            body = _body(src, "Knobs read_knobs()")
            assert "getenv" in body
            src = src.replace(body, "")
        for m in re.finditer(r"getenv\s*\(\s*([^)]*)\)", src):
            assert m.group(1).strip('"') in DIAGNOSTICS, (os.path.basename(path), m.group(0))
