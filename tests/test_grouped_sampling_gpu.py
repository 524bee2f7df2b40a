"""The sampling solves of a large 3-D grid in lock-step with grouped metric applications (engine._solve_grouped) against one
solve after the other (NK_GROUP=0, a child process: the library reads the knob once): the same residuals, mean, KL value, work
counters and CG iteration counts, bit for bit."""
import json
import os
import subprocess
import sys

import pytest

from tests import group_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ungrouped():
    env = dict(os.environ, NK_GROUP="0")
    child = subprocess.run([sys.executable, "-m", "tests.group_cases", "sampling"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    return json.loads(child.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(gc.SAMPLING_CASES))
def test_grouped_sampling_equals_single_solves(ungrouped, name, monkeypatch):
    taken = []
    from nifty_amd import engine

    real = engine._solve_grouped
    monkeypatch.setattr(engine, "_solve_grouped", lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    grouped = gc.sampling_case(name)
    assert taken, "the lock-step path was not taken"
    print(name, grouped["solve_lengths"], grouped["cg_iterations"], grouped["counters"])
    assert grouped == ungrouped[name]
    if name == "staggered4":
        assert len(set(json.loads(grouped["solve_lengths"].replace("None", "null")))) > 1, "the solves should stop at different iterations"
