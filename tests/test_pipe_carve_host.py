"""Workspace carve of the sliced dagpu_extend_batch_device (csrc/pipe_carve.hpp)
on the CPU: tests/host/pipe_carve_check.cpp, a stand-alone host program, runs
the carve over k = 1..512, n = 1..300, S = 1..8 and every cut level, and checks
that the regions are pairwise disjoint and end inside dagpu_workspace_size(k, n)
whenever the carve defers tree levels, and that it reports the fallback exactly
when they cannot fit."""
import os
import subprocess

from conftest import ROOT


def test_pipe_carve_regions(tmp_path):
    exe = str(tmp_path / "pipe_carve_check")
    src = os.path.join(ROOT, "tests", "host", "pipe_carve_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    # both outcomes occur: deferred carves and fallbacks
    assert int(fields["deferred"]) > 0 and int(fields["fallback"]) > 0
    assert int(fields["checked"]) == int(fields["deferred"]) + int(fields["fallback"])
