"""The C++ plan_crossword (celestia-app_amd/csrc/crossword_plan.hpp, HIP-free)
on the CPU: tests/host/crossword_plan_check.cpp, a stand-alone host program,
prints its plan for a presence bitmap, and every field must equal the Python
plan() of tests/test_repair_order_host.py, which that module ties to the
oracle's sequential rsmt2d order.  The maps are the ones that module's _case
draws at k = 2, 4, 8 (both shapes, the same seeded stream), plus two fixed
ones: all present, and one cell present.  repair_host.cpp exact_repair names
the byzantine axis from this plan; before the plan had a header of its own it
ran only on a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_repair_order_host import _case, plan


def _drawn_maps(k):
    """Presence maps of test_gpu_repair_procedures_match_sequential_oracle's cases."""
    rng = np.random.default_rng(1000 + k)
    maps = []
    for t in range({2: 60, 4: 40, 8: 16}[k]):
        shape = "subgrid" if t % 2 else "random"
        frac = float(rng.choice([0.1, 0.3, 0.5, 0.7, 0.9]))
        maps.append(_case(k, rng, frac, int(rng.integers(0, 3)), shape)[1])
    return maps


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host") / "crossword_plan_check")
    src = os.path.join(ROOT, "tests", "host", "crossword_plan_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], check=True, timeout=120)
    return exe


def _cxx_plans(exe, k, maps):
    """plan_crossword (C++) of every presence map: the fields as printed."""
    text = "".join(f"{k}\n" + "".join("1" if v else "0" for v in m.ravel()) + "\n" for m in maps)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    plans = []
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            plans.append({"attempts": []})
        elif f[0] == "attempt":
            ax, i, lvl, *ortho = map(int, f[1:])
            plans[-1]["attempts"].append((ax, i, lvl, ortho))
        elif f[0] == "att_level":
            plans[-1]["att_level"] = list(map(int, f[1:]))
        else:
            plans[-1][f[0]] = int(f[1])
    assert len(plans) == len(maps)
    return plans


def _py_plan(pres, k):
    """plan() in the C++ plan's fields."""
    w = 2 * k
    att, complete = plan(pres, k)
    att_level = [-1] * (2 * w)
    for ax, i, lvl, _ in att:
        att_level[ax * w + i] = lvl
    return {"attempts": [(int(ax), int(i), int(lvl), [int(o) for o in ortho]) for ax, i, lvl, ortho in att],
            "att_level": att_level, "nlevels": max([a[2] for a in att], default=-1) + 1,
            "complete": int(complete)}


@pytest.mark.parametrize("k", [2, 4, 8])
def test_cxx_plan_crossword_equals_python_plan(k, plan_exe):
    w = 2 * k
    full = np.ones((w, w), bool)
    one = np.zeros((w, w), bool)
    one[w - 1, 1] = True
    maps = _drawn_maps(k) + [full, one]
    got = _cxx_plans(plan_exe, k, maps)
    for t, (pres, g) in enumerate(zip(maps, got)):
        assert g == _py_plan(pres, k), t
    # the two fixed maps: nothing to attempt; complete only when all is present
    assert got[-2] == {"attempts": [], "att_level": [-1] * (2 * w), "nlevels": 0, "complete": 1}
    assert got[-1] == {"attempts": [], "att_level": [-1] * (2 * w), "nlevels": 0, "complete": 0}
    # the drawn maps do exercise the plan: attempts, orthogonal completions, several levels
    assert any(g["nlevels"] > 1 for g in got) and any(a[3] for g in got for a in g["attempts"])
