"""The host executor, the lane emulation and the generalised gather lane of
csrc/square_units.hpp / square_read.hpp in a stand-alone program
(tests/host/square_units_check.cpp) built plain and with the address and
undefined-behaviour sanitizers.  The cases file holds every square of
square_units_cases.squares() with the unit table and the unit bytes the Python
mirror gives, and the tampered k = 4 squares with the verdict each must get;
squares, tables and unit payloads live in heap blocks of exactly their sizes,
so a read or write one byte outside fails the sanitized run."""
import os
import struct
import subprocess

import pytest

from celestia_da import shares as sh

import square_read_cases as rc
import square_units_cases as cases
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "square_units_check.cpp")


def _mirror_code(shares):
    """What the serial walk returns, by the mirror: 1 where parse_txs fails."""
    try:
        for ns in (sh.TX_NAMESPACE, sh.PAY_FOR_BLOB_NAMESPACE):
            sh.parse_txs(rc.compact_range(list(shares), ns))
    except sh.ShareError:
        return 1
    return 0


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("square_units") / "cases.bin"
    n = shares = units = nbytes = host = refused = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", 0))
        for _, k, s, _ in cases.squares():
            rec, scan = rc.mirror_records(list(s))
            want, data = cases.mirror_units(s)
            f.write(struct.pack("<QQQQQ", k, len(rec), len(want), 0, 0) + scan.tobytes())
            f.write(b"".join(x.to_bytes() for x in s) + rec.tobytes() + want.tobytes() + b"".join(data))
            n, shares, units, nbytes = n + 1, shares + k * k, units + len(want), nbytes + sum(map(len, data))
        for _, s, must in cases.tampered():
            rec, scan = rc.mirror_records(list(s))
            code = _mirror_code(s)
            f.write(struct.pack("<QQQQQ", 4, len(rec), 0, 1 if must else 2, code) + scan.tobytes())
            f.write(b"".join(x.to_bytes() for x in s) + rec.tobytes())
            n, shares, host, refused = n + 1, shares + 16, host + bool(must), refused + code
        f.seek(0)
        f.write(struct.pack("<Q", n))
    return str(path), n, shares, units, nbytes, host, refused


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_square_units_check(tmp_path, cases_file, name, flags):
    path, n, shares, units, nbytes, host, refused = cases_file
    exe = str(tmp_path / ("square_units_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    assert n >= 60 and int(fields["cases"]) == n and int(fields["shares"]) == shares
    assert int(fields["units"]) == units > 1000 and int(fields["bytes"]) == nbytes
    assert int(fields["host"]) == host >= 7 and int(fields["refused"]) == refused == 1
