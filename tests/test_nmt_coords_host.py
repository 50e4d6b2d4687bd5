"""Index maps of the NMT leaf and level kernels (csrc/nmt_coords.hpp) on the
CPU: tests/host/nmt_coords_check.cpp, a stand-alone host program, enumerates
the shift-and-mask maps for every power of two k = 1..512, n = 1..3, the three
leaf launches of the pipeline and every tree level, and checks them lane by
lane against the division formulas the kernels used before: same (square,
cell) and (square, axis, tree, node), each once, nothing out of range, record
indices equal to level_rec's, and the 32-bit lane offsets within the bounds the
header states (sampled at k = 8192, where a cell's offset passes 2^32)."""
import os
import subprocess

from conftest import ROOT


def test_nmt_coords_against_former_maps(tmp_path):
    exe = str(tmp_path / "nmt_coords_check")
    src = os.path.join(ROOT, "tests", "host", "nmt_coords_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    # k = 1..512 x n = 1..3: 6 n k^2 leaves over the three full/half launches
    assert int(fields["leaves"]) > 6 * 6 * 512 * 512
    assert int(fields["nodes"]) > 6 * 2 * 512 * 512 and int(fields["sampled"]) > 0
