"""The device planner on the CPU (dagpu_square_plan_emulate_host: the kernels'
algorithm of csrc/square_plan.hpp as host loops, 256 lanes per phase) against
the host planner (dagpu_square_plan through square.plan_native), which decides
every expectation: an accepted block's plan byte for byte and its width, a
rejected block's status kind, and for the three errors of Construct's append
loop the tx index of the message.  The same blocks go through a stand-alone
program (tests/host/square_plan_check.cpp) built plain and with the address and
undefined-behaviour sanitizers; that program also proves the integer
blob_min_square_size / subtree_width_u equal to the double forms."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from celestia_da import _abi
from celestia_da import shares as sh
from celestia_da import square as sq

import square_corpus
import square_plan_device_cases as cases
from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "host", "square_plan_check.cpp")
APPEND_ERRORS = ((re.compile(r"not enough space to append tx at index (\d+)$"), _abi.PLAN_NO_SPACE_TX),
                 (re.compile(r"not enough space to append blob tx at index (\d+)$"), _abi.PLAN_NO_SPACE_BLOB_TX),
                 (re.compile(r"normal tx at index (\d+) can not be appended after blob tx$"),
                  _abi.PLAN_TX_AFTER_BLOB_TX))


def host_verdict(txs, max_square_size):
    """(k, plan bytes, None) of the host planner, or (None, None, (kind, index
    or None)) with the status the device planner owes for the host's error."""
    try:
        k, plan = sq.plan_native(txs, max_square_size)
        return k, plan.tobytes(), None
    except sh.ShareError as e:
        for rx, kind in APPEND_ERRORS:
            m = rx.search(str(e))
            if m:
                return None, None, (kind, int(m.group(1)))
        return None, None, (_abi.PLAN_LAYOUT, None)


def check_block(name, txs, max_square_size, arena, rec, word):
    k, plan, err = host_verdict(txs, max_square_size)
    kind, index = sq.plan_status(word)
    assert int(rec["status"]) == int(word), name
    if err is None:
        assert word == 0, f"{name}: status {kind} index {index} for a block the host accepts"
        assert int(rec["k"]) == k and int(rec["plan_off"]) % 16 == 0, name
        got = sq.plan_of(arena, rec)
        assert got is not None and got.tobytes() == plan, f"{name}: plan differs"
        assert int(rec["nblob"]) == len(sq.plan_blobs(np.frombuffer(plan, np.uint8))), name
    else:
        assert kind == err[0], f"{name}: kind {kind} index {index}, the host's error maps to {err}"
        if err[1] is not None:
            assert index == err[1], f"{name}: index {index}, the host's message names {err[1]}"
        assert int(rec["plan_bytes"]) == 0 and sq.plan_of(arena, rec) is None, name
    return err is None


@pytest.mark.parametrize("group", ["corpus", "parser", "layout"])
def test_blocks_one_by_one(group):
    blocks = {"corpus": square_corpus.corpus, "parser": cases.parser_blocks, "layout": cases.layout_blocks}[group]()
    accepted = 0
    for name, txs, m in blocks:
        arena, rec, status = sq.plan_emulate([txs], m)
        accepted += check_block(name, txs, m, arena, rec[0], status[0])
    assert 0 < accepted < len(blocks)  # every group holds blocks of both kinds


def test_crafted_txs_cover_both_verdicts():
    """The crafted txs are told apart as the host tells them: a block [good
    blob tx, crafted] is accepted exactly when the crafted tx is a blob tx."""
    from celestia_da import blobtx as bt
    kinds = {name: bt.unmarshal_blob_tx(tx)[1] for name, tx in cases.crafted_txs()}
    assert sum(kinds.values()) >= 15 and sum(not v for v in kinds.values()) >= 20
    for name in ("field_1_twice", "unknown_wt0", "unknown_wt1", "unknown_wt5", "varint_10_bytes",
                 "empty_inner_absent", "share_version_1", "namespace_version_1", "empty_blob_data"):
        assert kinds[name], name
    for name in ("sdk_tx_shape", "no_blob", "ns_id_27", "ns_id_29", "wire_type_3", "field_number_0",
                 "varint_11_bytes", "length_past_tx", "length_past_blob"):
        assert not kinds[name], name


def test_all_blocks_in_one_call():
    """Every 128-wide-limit block of the lists in one batch: blocks do not disturb each other."""
    blocks = [b for b in square_corpus.corpus() + cases.all_blocks() if b[2] == 128]
    arena, rec, status = sq.plan_emulate([txs for _, txs, _ in blocks], 128)
    ends = sorted((int(r["plan_off"]), int(r["plan_off"]) + int(r["plan_bytes"])) for r in rec if r["plan_bytes"])
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))  # plans do not overlap
    for (name, txs, m), r, w in zip(blocks, rec, status):
        check_block(name, txs, m, arena, r, w)


@pytest.mark.parametrize("name,blocks,m", cases.batches(), ids=[b[0] for b in cases.batches()])
def test_batches(name, blocks, m):
    arena, rec, status = sq.plan_emulate(blocks, m)
    ok = [check_block(f"{name}[{i}]", txs, m, arena, rec[i], status[i]) for i, txs in enumerate(blocks)]
    if name == "rejected_between":
        assert ok == [True, False, True]
    if name == "widths_1_2_8":
        assert [int(r["k"]) for r in rec] == [1, 2, 8, 2, 1]
    if name == "empty_between":
        assert int(rec[1]["k"]) == 1 and ok == [True, True, True]


def test_too_many_blobs():
    """Blobs without data cost no share: five of them pass the append loop of a
    4-share square.  The host rejects the block in Export; the planner before
    it sorts."""
    tx = cases.blob_tx(b"x", *[cases.blob_msg(cases.ns_id(cases.NS1), b"")] * 5)
    with pytest.raises(sh.ShareError, match="blob data can not be empty"):
        sq.plan_native([tx], 2)
    _, rec, status = sq.plan_emulate([[tx]], 2)
    assert sq.plan_status(status[0])[0] == _abi.PLAN_TOO_MANY_BLOBS and int(rec[0]["plan_bytes"]) == 0


def test_refusals():
    L = _abi.lib()
    assert L.dagpu_square_plan_device_workspace_size(1, 10, 256) == 0
    assert L.dagpu_square_plan_device_workspace_size(1, 10, 96) == 0
    with pytest.raises(ValueError, match="power of two <= 128"):
        sq.plan_emulate([[b"x"]], 256)
    src, offs, ntx, lens = sq.pack_blocks([[b"abc", b"de"], [b"f"]])
    arena, rec, status = np.zeros(1 << 20, np.uint8), np.zeros(2, sq.plan_record_dtype()), np.zeros(4, np.uint32)

    def call(offs=offs, ntx=ntx, lens=lens, arena=arena, off=0):
        return L.dagpu_square_plan_emulate_host(2, _abi.addr(src), _abi.addr(offs), src.size, _abi.addr(ntx),
                                                _abi.addr(lens), 128, 64, _abi.addr(arena) + off, arena.size - off,
                                                _abi.addr(rec), _abi.addr(status))
    assert call() == 0 and list(status[:2]) == [0, 0]
    bad = lens.copy()
    bad[1] = 1
    assert call(lens=bad) == _abi.ERR_ARG and b"add up" in L.dagpu_last_error(None)
    bad[1] = 4
    assert call(lens=bad) == _abi.ERR_ARG
    assert call(offs=np.array([0, 6, 5], np.uint64)) == _abi.ERR_ARG
    assert call(offs=np.array([0, 5, 7], np.uint64)) == _abi.ERR_ARG  # past src_bytes
    assert call(off=4) == _abi.ERR_ARG  # alignment
    # an arena below the bound: the block gets a status, nothing is written past the arena
    small = np.full(256, 0xA5, np.uint8)
    rc = L.dagpu_square_plan_emulate_host(2, _abi.addr(src), _abi.addr(offs), src.size, _abi.addr(ntx),
                                          _abi.addr(lens), 128, 64, _abi.addr(small), 128, _abi.addr(rec),
                                          _abi.addr(status))
    assert rc == 0 and sq.plan_status(status[0])[0] == _abi.PLAN_ARENA and (small == 0xA5).all()


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("square_plan") / "cases.bin"
    blocks = square_corpus.corpus() + cases.all_blocks()
    plans = rejected = ntx = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(blocks)))
        for _, txs, m in blocks:
            _, plan, err = host_verdict(txs, m)
            kind, index = err if err else (0, 0)
            f.write(struct.pack("<QQQQQ", m, len(txs), kind, (1 << 64) - 1 if index is None else index,
                                len(plan) if plan else 0))
            f.write(np.array([len(t) for t in txs], np.uint64).tobytes() + b"".join(txs) + (plan or b""))
            plans, rejected, ntx = plans + (err is None), rejected + (err is not None), ntx + len(txs)
    return str(path), len(blocks), plans, rejected, ntx


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_square_plan_check(tmp_path, cases_file, name, flags):
    path, n, plans, rejected, ntx = cases_file
    exe = str(tmp_path / ("square_plan_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC, "-L", PKG, "-ldagpu",
                    "-Wl,-rpath," + PKG], check=True, timeout=300)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    assert int(fields["cases"]) == n >= 200 and int(fields["txs"]) == ntx
    assert int(fields["plans"]) == plans >= 100 and int(fields["rejected"]) == rejected >= 40
    assert int(fields["widths"]) == 3 * (128 * 128 + 2)
