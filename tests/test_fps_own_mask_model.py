"""CPU: the own-candidate mask of fps_bucket_kernel, in tools/fps_bucket_model.py.  The wave that wins an iteration takes the box
test of the next one from a mask it worked out ahead of time against its own candidate.  Under rule (a) that mask is the mask of
the hand-off itself; under rule (b) it may be older and then contains it.  Every iteration is checked, on the clouds and kernel
shapes the GPU test runs (tests/test_gpu_fps_own_mask.py), and both the reuse and the fall-back path must occur."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from toothgroupnetwork_amd import synth

M = 256
CASES = [(4096, 70, 512, 16), (4096, 71, 512, 16), (2048, 72, 256, 8)]      # n, seed, threads, slots per wave


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("fps_bucket_model", os.path.join(REPO, "tools", "fps_bucket_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def plain(model):
    return {(n, seed): model.plain_fps(synth.arch_cloud(n, seed, False), M) for n, seed, _, _ in CASES}


@pytest.mark.parametrize("rule", ["a", "b"])
@pytest.mark.parametrize("n,seed,nt,p", CASES)
def test_reused_mask_against_the_mask_of_the_hand_off_in_every_iteration(model, plain, n, seed, nt, p, rule):
    xyz = synth.arch_cloud(n, seed, False)
    trace = []
    idx, stats = model.simulate(xyz, M, nt=nt, p=p, own_rule=rule, trace=trace)
    assert np.array_equal(idx, plain[(n, seed)])
    assert [t[0] for t in trace] == list(range(1, M))             # no iteration left out
    reused = 0
    for j, wl, was_reused, used, exact in trace:
        assert 0 <= wl < nt // 64 and used.shape == exact.shape
        if rule == "a" or not was_reused:
            assert np.array_equal(used, exact), f"iteration {j}, wave {wl}"
        else:
            assert not (exact & ~used).any(), f"iteration {j}, wave {wl}: a bucket of the hand-off's mask is missing"
        reused += was_reused
    assert stats["winner_clean"] == reused / (M - 1)
    assert 0.0 < stats["winner_clean"] < 1.0                      # both paths
    assert 0.0 <= stats["winner_same_wave"] < 1.0
    assert stats["own_rule"] == rule
    assert stats["extra_touched"] == 0.0 if rule == "a" else stats["extra_touched"] >= 0.0


def test_existing_statistics_do_not_depend_on_the_rule(model):
    xyz = synth.arch_cloud(4096, 70, False)
    (ia, sa), (ib, sb) = (model.simulate(xyz, M, nt=512, p=16, own_rule=r) for r in "ab")
    assert np.array_equal(ia, ib)
    for k in ("touched", "changed", "refreshed", "busiest_touched", "busiest_refreshed", "busiest_hist", "winner_clean", "winner_same_wave"):
        assert sa[k] == sb[k], k
