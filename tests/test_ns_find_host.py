"""The namespace search of nmt ProveNamespace (csrc/ns_find.hpp: classify against
the root, then lower / upper bound) on the CPU: tests/host/ns_find_check.cpp, a
stand-alone host program, compares it with a linear scan for every sorted
namespace multiset over 3 distinct values in rows of 1 .. 16 leaves, with and
without a parity half, for the values, the gaps between them and both ends.
Built plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "ns_find_check.cpp")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_ns_find_check(tmp_path, name, flags):
    exe = str(tmp_path / ("ns_find_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    # multisets of n leaves over 3 values: (n + 1)(n + 2) / 2, two passes, nine queries each
    rows = 2 * sum((n + 1) * (n + 2) // 2 for n in range(1, 17))
    assert int(fields["rows"]) == rows and int(fields["checks"]) == 9 * rows and int(fields["ordered"]) == 81
    assert all(int(fields[c]) > 0 for c in ("outside", "present", "absent"))
    assert int(fields["outside"]) + int(fields["present"]) + int(fields["absent"]) == 9 * rows
