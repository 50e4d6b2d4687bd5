"""The host executor, the unit walk and the gather's per-lane function of
csrc/square_read.hpp in a stand-alone program (tests/host/square_read_check.cpp)
built plain and with the address and undefined-behaviour sanitizers.  The cases
file holds every accepted corpus square, the hand-made k = 64 squares and the
tampered k = 4 squares with what the Python mirror says about them; squares
and payloads live in heap blocks of exactly their sizes, so a read or write one
byte outside fails the sanitized run."""
import os
import struct
import subprocess

import pytest

from celestia_da import _abi
from celestia_da import shares as sh

import square_read_cases as cases
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "square_read_check.cpp")


def _full_case(f, k, shares):
    shares = list(shares)
    rec, summary = cases.mirror_records(shares)
    f.write(struct.pack("<QQQQ", k, k * k, len(rec), 1) + summary.tobytes())
    f.write(b"".join(s.to_bytes() for s in shares) + rec.tobytes())
    units = payload = 0
    for r, q in zip(rec, sh.parse_shares(shares, False)):
        if q.is_padding():
            continue
        data = cases.seq_payload(q)
        f.write(data)
        payload += len(data)
        if not r["flags"] & _abi.SEQ_SPARSE:
            # where the mirror's units lie in the payload
            found = sh.parse_compact_shares(q.shares)
            at, table = int(r["reserved"]) - 38, []
            for u in found:
                at += sh.delim_len(len(u))
                assert data[at:at + len(u)] == u
                table.append((at, len(u)))
                at += len(u)
            f.write(struct.pack("<Q", len(table)) + b"".join(struct.pack("<QQ", *t) for t in table))
            units += len(table)
    return len(rec), payload, units


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("square_read") / "cases.bin"
    n = shares = records = payload = units = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", 0))
        full = [(k, s) for _, _, k, s in cases.accepted()] + [(k, s) for _, k, s, _ in cases.hand_made()]
        for k, s in full:
            r, p, u = _full_case(f, k, s)
            n, shares, records, payload, units = n + 1, shares + k * k, records + r, payload + p, units + u
        for _, s, code, index, ver in cases.tampered():
            f.write(struct.pack("<QQQQ", 4, 16, 0, 0) + struct.pack("<8i", code, index, ver, 0, 0, 0, 0, 0))
            f.write(b"".join(x.to_bytes() for x in s))
            n, shares = n + 1, shares + 16
        f.seek(0)
        f.write(struct.pack("<Q", n))
    return str(path), n, shares, records, payload, units


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_square_read_check(tmp_path, cases_file, name, flags):
    path, n, shares, records, payload, units = cases_file
    exe = str(tmp_path / ("square_read_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    assert n >= 50 and int(fields["cases"]) == n and int(fields["shares"]) == shares
    assert int(fields["records"]) == records and int(fields["payload"]) == payload and int(fields["units"]) == units
    assert units > 1000 and int(fields["edges"]) > 1000  # shares whose content starts inside an 8-byte word
