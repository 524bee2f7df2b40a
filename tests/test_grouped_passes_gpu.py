"""Grouped launches of the sandwich's first and final pass (nk_hartley_sandwich_group through FusedModel.lh_metric_group,
nk_hartley_sandwich_pair's grouped first passes) against the single launches: bit equality everywhere, no tolerances."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import group_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = gc.PASS_SHAPES  # odd workgroup counts per member, unequal axes, a partial last group of eight in both
# ((32, 64, 256) is not among them: the sandwich pipeline needs every axis >= 64, nk_plan_sandwich refuses that plan)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "x".join(map(str, p[0])) + ("-f64" if p[1] == torch.float64 else "-f32"))
def setup(request):
    shape, dtype = request.param
    model, xs, ds, rs = gc.pass_setup(shape, dtype)
    assert model.group_ready()
    return model, xs, ds, rs, [model.linearize(x) for x in xs]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_group_with_direction_update_equals_single_calls(setup, count):
    """Prologue class 8: members share in2 / xi / afield, each rewrites its own `in`; identity addend and curvature dot.
    out, the small part (through w8 and the spectrum scatter), w8, max |w8|, the curvature slot, the rolled scalars and the
    written-back direction."""
    model, xs, ds, rs, lps = setup
    _same(gc.class8_group(model, lps[0], ds, rs, count), gc.class8_single(model, lps[0], ds, rs, count))


@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_group_sharing_the_direction_equals_single_calls(setup, count):
    """Prologue class 5: members share `in` at different linearisation points."""
    model, xs, ds, rs, lps = setup
    _same(gc.class5_group(model, lps, ds[0], count), gc.class5_single(model, lps, ds[0], count))


def test_group_rejects_a_member_that_writes_what_another_reads(setup):
    model, xs, ds, rs, lps = setup
    jobs, _ = gc.class8_jobs(model, ds, rs, 2)
    jobs[1]["d"].xi = jobs[0]["d"].xi  # both members would rewrite the same `in`
    with pytest.raises(ValueError):
        model.lh_metric_group(lps[0], jobs)
    jobs, _ = gc.class8_jobs(model, ds, rs, 2)
    jobs[1]["cg_direction"] = (jobs[0]["d"], jobs[1]["cg_direction"][1])  # member 1 reads what member 0 rewrites
    with pytest.raises(ValueError):
        model.lh_metric_group(lps[0], jobs)
    torch.cuda.synchronize()


def test_five_sample_kl_metric_equals_unpaired_loop(setup):
    """FusedKL.apply_metric over five samples (pairs with grouped first passes for the middle samples) against single launches."""
    model, xs, ds, rs, lps = setup
    paired = gc.kl_metric(model, xs, ds[0])
    os.environ["NK_PAIR_FINAL"] = "0"
    try:
        single = gc.kl_metric(model, xs, ds[0])
    finally:
        del os.environ["NK_PAIR_FINAL"]
    _same(paired, single)


def test_group_knob_off_gives_the_same_bits():
    """NK_GROUP=0 (read once per process: a child) against the grouped launches of this process, digest by digest."""
    env = dict(os.environ, NK_GROUP="0")
    child = subprocess.run([sys.executable, "-m", "tests.group_cases", "passes"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    off = json.loads(child.stdout.strip().splitlines()[-1])
    on = gc.passes_digests()
    assert on.keys() == off.keys()
    assert [k for k in on if on[k] != off[k]] == []
