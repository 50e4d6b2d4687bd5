"""The per-share writer of csrc/square_write.hpp, the code the square-write
kernel runs, on the CPU in a stand-alone program (tests/host/square_write_check.cpp)
built plain and with the address and undefined-behaviour sanitizers: every
accepted block of tests/square_corpus.py, its plan and txs in heap blocks of
exactly their sizes, every share compared with dagpu_square_construct's.  A
read one byte outside a plan or its txs fails the sanitized run."""
import os
import struct
import subprocess

import numpy as np
import pytest

from celestia_da import square as sq

from conftest import ROOT
from square_corpus import corpus

SRC = os.path.join(ROOT, "tests", "host", "square_write_check.cpp")


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("square_write") / "cases.bin"
    n = shares = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", 0))
        for _, txs, m in corpus():
            try:
                k, ods = sq.construct_native(txs, m)
            except sq.ShareError:
                continue
            _, plan = sq.plan_native(txs, m)
            src = b"".join(txs)
            f.write(struct.pack("<QQQ", plan.size, len(src), k))
            f.write(plan.tobytes() + src + np.ascontiguousarray(ods).tobytes())
            n, shares = n + 1, shares + k * k
        f.seek(0)
        f.write(struct.pack("<Q", n))
    return str(path), n, shares


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_square_write_check(tmp_path, cases_file, name, flags):
    path, n, shares = cases_file
    exe = str(tmp_path / ("square_write_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    assert n >= 40 and int(fields["cases"]) == n and int(fields["shares"]) == shares
    assert int(fields["seams"]) > 1000  # segment seams were crossed, not only whole-word copies
