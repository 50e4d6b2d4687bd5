"""Every GF(2^8) Reed-Solomon kernel arm, tail chunks included.

The dispatchers (launch_leo8_encode in rs_gf8.hip, launch_leo8_encode_sliced /
launch_leo8_fill_sliced in rs_gf8_sliced.hip, launch_leo8_decode_only in
rs_decode.hip) choose between the packed and the bit-sliced kernels by shape
and by the DAGPU_ENC_SLICED / DAGPU_ENC_SLICED2 / DAGPU_DEC_SLICED switches.
Each test below runs one group of cases (tests/rs_arms_child.py) in a child
process on the test build of the library (libdagpu_test.so, DAGPU_TEST_HOOKS),
which counts launches per arm: a case compares the whole output buffer bit for
bit with the oracle and asserts the arm that ran, so a switch that selected
nothing, or a shape that took another kernel than meant, fails.

Arm -> cases that reach it:
  packed encode          encode tail (k = 1..128, shard 576 / 1088, nvec 3 / 4);
                         encode whole and both square cases, DAGPU_ENC_SLICED=0
  packed reverse encode  unreachable at k = 128; k < 128 is
                         tests/test_gpu_repair_fill.py's (q3, right_half patterns)
  4-vector sliced encode encode whole k = 16 / 32 / 64 default, k = 128 and
                         both square cases under DAGPU_ENC_SLICED2=0
  2-vector sliced encode encode whole k = 128 default
  sliced fill / reverse  repair k = 128 subgrid / q3 (fill route on)
  small decode           decode tail k = 1..64, shard 320 / 576
  packed k = 128 decode  decode tail k = 128; decode whole and the shared-pattern
                         batch and Repair under DAGPU_DEC_SLICED=0
  sliced k = 128 decode  decode whole k = 128 default; repair, default decoder
"""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "rs_arms_child.py")


def _run_group(group, ncases):
    env = dict(os.environ, DAGPU_LIB=os.path.join(PKG, "libdagpu_test.so"))
    # the cases set the switches they mean to; none may leak in from outside
    for name in ("DAGPU_ENC_SLICED", "DAGPU_ENC_SLICED2", "DAGPU_DEC_SLICED", "DAGPU_REPAIR_FILL"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, CHILD, group], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    fails = [line for line in r.stdout.split("\n") if line.startswith("FAIL")]
    assert not fails, "\n".join(fails[:20])
    m = re.search(rf"^DONE {group} (\d+) cases, 0 failed$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == ncases


def test_encode_tail_chunks_take_the_packed_encoder():
    """dagpu_encode, k = 1..128, shard 576 / 1088 (one or two whole 512-B chunks
    and a 64-B tail), nvec 3 / 4: parity of every vector equals oracle.encode;
    a lane wrongly active past the shard's end would write into the next shard."""
    _run_group("encode_tail", 8 * 2 * 2)


def test_encode_whole_chunks_every_arm():
    """k = 16..128, (nvec, shard) = (4, 512) and (16, 1024) -- the second with a
    block count that is a multiple of 8 (XCD remap) and two chunks per shard:
    4-vector sliced at k < 128 and 2-vector sliced at k = 128 by default,
    4-vector at k = 128 under DAGPU_ENC_SLICED2=0, packed under DAGPU_ENC_SLICED=0."""
    _run_group("encode_whole", 4 * 2 * 2 + 2)


def test_decode_tail_chunks():
    """dagpu_decode, k = 1..128, shard 320 / 576, four erasure patterns (random
    k kept, random k + k/4 kept, all data lost, all parity lost), missing
    shards holding 0xA5 in half of the cases: small decoder, packed at k = 128."""
    _run_group("decode_tail", 8 * 2 * 4)


def test_decode_k128_whole_chunks_both_arms():
    """k = 128, shard 512 / 1024, the four patterns: bit-sliced by default,
    packed (256-B chunks 0..3 live) under DAGPU_DEC_SLICED=0, and the batch of
    24 vectors with shared erasure patterns through the packed decoder."""
    _run_group("decode_k128_whole", 2 * 4 * 2 + 1)


def test_square_path_on_the_alternative_encoders():
    """da.extend_shares of one k = 128 square and DeviceSquares(128, 3) under
    DAGPU_ENC_SLICED2=0 and under DAGPU_ENC_SLICED=0: every EDS byte equals
    oracle.extend_and_dah's (row pass with the Q0 copy, column pass strides,
    several squares per launch)."""
    _run_group("square", 2 * 2)


def test_repair_k128_through_the_packed_decoder():
    """One k = 128 square under DAGPU_DEC_SLICED=0, with the fill route on and
    off (DAGPU_REPAIR_FILL=0): the random k x k sub-grid and the Q3-only
    pattern repair to the original EDS, and a corrupted present share raises
    ErrByzantineData with the axis and index the default decoder reports."""
    _run_group("repair", 1 + 2 * 3)
