"""csrc/switches.hpp says of the DAGPU_* switches: "Every switch selects between
two paths that tests/ check against each other or against the oracle".  This
holds the suite to it: every name in kSwNames (csrc/dagpu.cpp) is set by at
least one file under tests/, and the name table has one entry per Switch
enumerator.  Also: the arm counters of the test build
(tests/test_gpu_rs_arms.py) stay out of the product library."""
import os
import re

from conftest import PKG, ROOT

TESTS = os.path.join(ROOT, "tests")


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def switch_names():
    src = open(os.path.join(PKG, "csrc", "dagpu.cpp")).read()
    m = re.search(r"kSwNames\[SW_COUNT\]\s*=\s*\{(.*?)\};", src, re.S)
    assert m, "kSwNames not found in csrc/dagpu.cpp"
    return re.findall(r'"(DAGPU_[A-Z0-9_]+)"', m.group(1))


def switch_enumerators():
    hdr = _strip_comments(open(os.path.join(PKG, "csrc", "switches.hpp")).read())
    m = re.search(r"enum\s+Switch\s*:\s*int\s*\{(.*?)\}", hdr, re.S)
    assert m, "enum Switch not found in csrc/switches.hpp"
    names = [x.strip() for x in m.group(1).split(",") if x.strip()]
    assert names[-1] == "SW_COUNT"
    return names[:-1]


def _sets(name, text):
    """Does `text` set environment variable `name`: setenv("NAME", ...) (pytest's
    monkeypatch or C), os.environ["NAME"] = ..., NAME="..." in an env mapping
    built with dict(...), or "NAME": ... in a dict literal."""
    q = rf"""["']{name}["']"""
    return any(re.search(p, text) for p in (
        rf"\bsetenv\(\s*{q}\s*,",
        rf"environ\[\s*{q}\s*\]\s*=[^=]",
        rf"\b{name}\s*=\s*[\"']",
        rf"{q}\s*:",
    ))


def test_name_table_matches_the_enum():
    names, enums = switch_names(), switch_enumerators()
    assert len(names) == len(enums) == len(set(names))
    # the table is indexed by the enumerator: SW_X <-> DAGPU_X, in order
    assert ["DAGPU_" + e[len("SW_"):] for e in enums] == names


def test_every_switch_is_set_by_a_test():
    texts = {}
    for d, _, files in os.walk(TESTS):
        if "golden" in d.split(os.sep) or "__pycache__" in d.split(os.sep):
            continue
        for f in files:
            if f.endswith((".py", ".c", ".cpp", ".hip", ".sh")) and f != os.path.basename(__file__):
                texts[os.path.join(d, f)] = open(os.path.join(d, f), errors="replace").read()
    unset = [n for n in switch_names() if not any(_sets(n, t) for t in texts.values())]
    assert not unset, f"no file under tests/ sets {unset}"


def test_setter_match_is_exact():
    assert _sets("DAGPU_ENC_SLICED", 'monkeypatch.setenv("DAGPU_ENC_SLICED", "0")')
    assert _sets("DAGPU_ENC_SLICED", 'env = dict(os.environ, DAGPU_ENC_SLICED="0")')
    assert _sets("DAGPU_ENC_SLICED", '{"DAGPU_ENC_SLICED": "0"}')
    assert _sets("DAGPU_ENC_SLICED", 'os.environ["DAGPU_ENC_SLICED"] = "0"')
    # another switch's name, prose, reads and deletions do not count
    assert not _sets("DAGPU_ENC_SLICED", 'monkeypatch.setenv("DAGPU_ENC_SLICED2", "0")')
    assert not _sets("DAGPU_ENC_SLICED", 'dict(os.environ, DAGPU_ENC_SLICED2="0")')
    assert not _sets("DAGPU_ENC_SLICED", '"""the packed encoder (DAGPU_ENC_SLICED=0)"""')
    assert not _sets("DAGPU_ENC_SLICED", 'monkeypatch.delenv("DAGPU_ENC_SLICED", raising=False)')
    assert not _sets("DAGPU_ENC_SLICED", 'if os.environ["DAGPU_ENC_SLICED"] == "0":')


_SYMBOLS_CHILD = r"""
import ctypes, sys
product, hooked = ctypes.CDLL(sys.argv[1]), ctypes.CDLL(sys.argv[2])
assert not hasattr(product, "dagpu_test_rs_arms")
f = hooked.dagpu_test_rs_arms
f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
counts = (ctypes.c_uint64 * 72)(*([7] * 72))
assert f(counts, 72, 1) == 72  # 9 arms x k = 1..128
assert list(counts) == [0] * 72  # nothing launched in this process
print("SYMBOLS_OK")
"""


def test_arm_counters_only_in_the_test_build():
    """In a child process: loading two builds of the library into the test
    process itself would register their device code twice."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _SYMBOLS_CHILD, os.path.join(PKG, "libdagpu.so"),
                        os.path.join(PKG, "libdagpu_test.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SYMBOLS_OK" in r.stdout, r.stderr[-2000:]
