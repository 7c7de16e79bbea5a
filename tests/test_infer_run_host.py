"""Host side of the inference entry point (toothgroupnetwork_amd/infer_run.py, tools/infer.py) and the scheduling of the staged run
(inference.run_staged) with plain functions as stages: no GPU."""
import json
import os
import threading
import time

import numpy as np
import pytest

from toothgroupnetwork_amd import infer_run, inference, results, sharding


# ---- collect_scans ---------------------------------------------------------------------------------------------------------------------
def _touch(path, text="v 0 0 0\n"):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return str(path)


@pytest.fixture()
def tree(tmp_path):
    root = tmp_path / "scans"
    made = {name: _touch(str(root / rel)) for name, rel in {
        "b_upper": "PB/PB_upper.obj", "b_lower": "PB/PB_lower.obj", "a_upper": "PA/PA_upper.obj", "deep": "group/nested/PC/PC_lower.obj",
        "out": "PD/PD_upper.obj", "root": "ROOT_upper.obj", "other": "PA/PA_upper.json", "stl": "PB/PB_upper.stl"}.items()}
    split = tmp_path / "split.txt"
    split.write_text("PB\nPA\n  PC  \nnobody\n")
    return str(root), str(split), made


def test_collect_scans_takes_the_split_sorted(tree):
    root, split, made = tree
    got = infer_run.collect_scans(root, split)
    assert got == sorted([made["a_upper"], made["b_lower"], made["b_upper"], made["deep"]])
    assert made["root"] not in got and made["out"] not in got


def test_collect_scans_empty_split_takes_every_sub_directory(tree):
    root, _, made = tree
    got = infer_run.collect_scans(root, "")
    assert got == sorted(made[k] for k in ("a_upper", "b_lower", "b_upper", "deep", "out"))


def test_collect_scans_missing_split_file(tree, tmp_path):
    missing = str(tmp_path / "no_such_split.txt")
    with pytest.raises(FileNotFoundError, match="no_such_split.txt"):
        infer_run.collect_scans(tree[0], missing)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_parser_has_the_reference_flags_and_defaults():
    a = infer_run.parse_args([])
    assert a.save_path == "test_results" and a.model_name == "tgnet"
    for flag in ("input_dir_path", "split_txt_path", "checkpoint_path", "checkpoint_path_bdl"):
        assert hasattr(a, flag)
    assert (a.batch, a.workers, a.seed, a.gt_dir, a.gpus, a.backend) == (8, None, None, None, 0, None)
    b = infer_run.parse_args(["--input_dir_path", "in", "--split_txt_path", "", "--save_path", "out", "--model_name", "dgcnn",
                              "--checkpoint_path", "c", "--checkpoint_path_bdl", "d", "--seed", "3", "--gpus", "2", "--backend", "gloo"])
    assert (b.input_dir_path, b.split_txt_path, b.save_path, b.model_name, b.checkpoint_path, b.checkpoint_path_bdl) == ("in", "", "out", "dgcnn", "c", "d")
    assert (b.seed, b.gpus, b.backend) == (3, 2, "gloo")


def test_unknown_model_name_is_the_factorys_value_error():
    with pytest.raises(ValueError) as e:
        infer_run.parse_args(["--model_name", "pointnet3"])
    assert all(name in str(e.value) for name in inference.MODEL_NAMES) and len(inference.MODEL_NAMES) == 6


# ---- output files ----------------------------------------------------------------------------------------------------------------------
def test_output_naming_and_the_lower_jaws_plus_20(tmp_path):
    upper, lower = _touch(str(tmp_path / "in" / "P1" / "P1_upper.obj")), _touch(str(tmp_path / "in" / "P1" / "P1_lower.obj"))
    nojaw = _touch(str(tmp_path / "in" / "P2" / "P2.obj"), "# neither\nv 0 0 0\n")
    sem, ins = np.array([0, 11, 18, 21, 28, 0]), np.array([0, 1, 2, 3, 4, 0])

    def pipeline(path):
        return {"sem": sem.copy(), "ins": ins.copy()}

    save = str(tmp_path / "out")
    done = infer_run.run_scans(pipeline, [lower, upper, nojaw], save, batch=2, workers=1)
    assert done["written"] == [os.path.join(save, "P1_lower.json"), os.path.join(save, "P1_upper.json")]
    assert [f["path"] for f in done["failed"]] == [nojaw] and "jaw" in done["failed"][0]["error"]
    assert sorted(os.listdir(save)) == ["P1_lower.json", "P1_upper.json"]
    got_sem, got_ins = results.read_labels(os.path.join(save, "P1_upper.json"), with_instances=True)
    assert np.array_equal(got_sem, sem) and np.array_equal(got_ins, ins)
    got_sem, got_ins = results.read_labels(os.path.join(save, "P1_lower.json"), with_instances=True)
    assert np.array_equal(got_sem, [0, 31, 38, 41, 48, 0]) and np.array_equal(got_ins, ins)
    assert json.load(open(os.path.join(save, "P1_lower.json")))["jaw"] == "lower"


# ---- shards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_shards_are_disjoint_and_cover_the_list(n, world):
    paths = [f"scan{i:02d}.obj" for i in range(n)]
    shares = [infer_run.shard(paths, r, world) for r in range(world)]
    flat = [p for share in shares for p in share]
    assert len(flat) == len(set(flat)) == n and sorted(flat) == paths
    assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1


# ---- the engine with fake stages -------------------------------------------------------------------------------------------------------
class Fakes:
    """Plain functions as the five stages; they record the thread and the order of every call."""

    def __init__(self, n, fail=None, delay=0.0, short=None):
        self.paths = [f"scan{i:02d}" for i in range(n)]
        self.fail, self.delay = fail or {}, delay                 # {stage: index that raises there}
        self.short = short                                        # the compute call that holds this scan answers one entry too few
        self.calls = {k: [] for k in ("load", "prepare", "sample", "compute", "finish")}
        self.groups = []                                          # the scans of every compute call
        self.lock = threading.Lock()

    def _note(self, stage, what):
        with self.lock:
            self.calls[stage].append((threading.current_thread().name, what))

    def _maybe_fail(self, stage, i):
        if self.fail.get(stage) == i:
            raise NotImplementedError(f"scripted failure in {stage}")

    def load(self, path):
        i = self.paths.index(path)
        time.sleep(self.delay * (len(self.paths) - i))            # the first loads finish last
        self._note("load", i)
        self._maybe_fail("load", i)
        return i

    def prepare(self, i):
        self._note("prepare", i)
        self._maybe_fail("prepare", i)
        return i * 10

    def sample(self, prepared):
        self._note("sample", list(prepared))
        for p in prepared:
            self._maybe_fail("sample", p // 10)
        return [p + 1 for p in prepared]

    def compute(self, scans, prepared, sampled):
        assert prepared == [i * 10 for i in scans] and sampled == [i * 10 + 1 for i in scans]
        self.groups.append(list(scans))
        for i in scans:
            self._note("compute", i)
        for i in scans:
            self._maybe_fail("compute", i)
        return [-i for i in scans][:len(scans) - (self.short in scans)]

    def finish(self, i, sampled, computed):
        assert computed == -i
        self._note("finish", i)
        self._maybe_fail("finish", i)
        return {"scan": i}

    def run(self, **kw):
        return inference.run_staged(self.paths, self.load, self.prepare, self.sample, self.compute, self.finish, **kw)


def _pool_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("tgn-")]


def test_engine_order_threads_and_chunks():
    f = Fakes(12, delay=0.002)
    stats = {}
    got = f.run(batch=1, workers=4, stats=stats)
    assert got == [{"scan": i} for i in range(12)]                          # path order, though load 1 finished last of its chunk
    assert [i for _, i in f.calls["compute"]] == list(range(12))
    assert {name for name, _ in f.calls["compute"]} == {threading.current_thread().name}
    assert [i for _, i in f.calls["load"][:5]] != [0, 1, 2, 3, 4], "the loads must have finished out of order for this test to say anything"
    chunks = [c for _, c in f.calls["sample"]]
    # at most 4 x batch, the first one batch (the calling thread waits for it), a ragged last chunk
    assert chunks == [[0], [10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110]]
    assert len({name for name, _ in f.calls["sample"]} | {name for name, _ in f.calls["prepare"]}) == 1
    assert all(name.startswith("tgn-load") for name, _ in f.calls["load"])
    assert all(name.startswith("tgn-finish") for name, _ in f.calls["finish"]) and len({n for n, _ in f.calls["finish"]}) <= 4
    assert set(stats) == {"load", "sample", "compute", "finish"} and all(v >= 0 for v in stats.values())
    assert _pool_threads() == []


def test_engine_handles_an_empty_list_and_a_wrapper():
    assert Fakes(0).run(batch=2, workers=2) == []
    seen = []

    def on_thread(fn, *a):
        seen.append((threading.current_thread().name, fn.__name__))
        return fn(*a)

    f = Fakes(3)
    assert f.run(batch=2, workers=2, on_thread=on_thread) == [{"scan": i} for i in range(3)]
    assert {fn for _, fn in seen} == {"prepare", "sample", "finish"}        # not load (host only), not compute (the calling thread)
    assert all(not name.startswith("tgn-load") and name.startswith("tgn-") for name, _ in seen)


@pytest.mark.parametrize("stage", ["load", "prepare", "sample", "compute", "finish"])
def test_engine_reraises_a_scans_own_exception_with_its_path(stage):
    f = Fakes(7, fail={stage: 2})
    first = "scan01" if stage == "sample" else "scan02"                     # a failing launch fails its chunk, scans 1..4: the first is raised
    with pytest.raises(NotImplementedError, match=f"{first}: scripted failure in {stage}"):
        f.run(batch=1, workers=3)
    assert _pool_threads() == []


@pytest.mark.parametrize("stage", ["load", "prepare", "sample", "compute", "finish"])
def test_engine_skip_records_the_error_and_completes_the_rest(stage):
    f = Fakes(7, fail={stage: 5})
    got = f.run(batch=1, workers=3, on_error="skip")
    lost = {5, 6} if stage == "sample" else {5}                             # a failing launch fails its chunk: scans 5 and 6
    for i, g in enumerate(got):
        if i in lost:
            assert set(g) == {"error"} and f"scan{i:02d}" in g["error"] and f"scripted failure in {stage}" in g["error"]
        else:
            assert g == {"scan": i}
    assert _pool_threads() == []


def test_engine_computes_groups_of_a_chunks_scans_in_path_order():
    f = Fakes(11, delay=0.001)
    got = f.run(batch=2, workers=3, group=2)
    assert got == [{"scan": i} for i in range(11)]
    assert f.groups == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10]]        # chunks [0, 1] [2..9] [10]: a group never spans two
    assert {name for name, _ in f.calls["compute"]} == {threading.current_thread().name}
    assert _pool_threads() == []


def test_engine_groups_close_the_gap_a_failed_scan_leaves():
    f = Fakes(11, fail={"prepare": 3})
    got = f.run(batch=2, workers=3, group=2, on_error="skip")
    assert f.groups == [[0, 1], [2, 4], [5, 6], [7, 8], [9], [10]]
    assert set(got[3]) == {"error"} and "scan03: scripted failure in prepare" in got[3]["error"]
    assert [g for i, g in enumerate(got) if i != 3] == [{"scan": i} for i in range(11) if i != 3]
    assert _pool_threads() == []


def test_engine_a_failing_compute_call_fails_its_group_and_no_other():
    f = Fakes(11, fail={"compute": 5})
    got = f.run(batch=2, workers=3, group=2, on_error="skip")
    for i, g in enumerate(got):
        if i in (4, 5):
            assert set(g) == {"error"} and f"scan{i:02d}: scripted failure in compute" in g["error"] and "NotImplementedError" in g["error"]
        else:
            assert g == {"scan": i}
    assert _pool_threads() == []
    with pytest.raises(NotImplementedError, match="scan04: scripted failure in compute"):    # the group's first scan in path order
        Fakes(11, fail={"compute": 5}).run(batch=2, workers=3, group=2)
    assert _pool_threads() == []


def test_engine_a_compute_call_that_answers_too_few_fails_its_group():
    f = Fakes(11, short=7)
    got = f.run(batch=2, workers=3, group=2, on_error="skip")
    for i, g in enumerate(got):
        if i in (6, 7):
            assert set(g) == {"error"} and f"RuntimeError: scan{i:02d}: the compute stage returned 1 entries for 2 scans" in g["error"]
        else:
            assert g == {"scan": i}
    assert _pool_threads() == []


def test_engine_refuses_an_unknown_error_mode():
    with pytest.raises(ValueError, match="on_error"):
        Fakes(1).run(on_error="ignore")


def test_default_workers_come_from_the_projects_cpu_accounting(monkeypatch):
    monkeypatch.setattr(sharding, "cpus_for_this_rank", lambda local_world, *a, **k: {1: 64, 8: 6}[local_world])
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert inference.default_workers() == 16                                # capped
    monkeypatch.setenv("WORLD_SIZE", "8")
    assert inference.default_workers() == 6


def test_infer_paths_runs_any_other_callable_one_by_one_with_the_same_error_rules():
    def pipeline(path):
        if path == "b":
            raise ValueError("no foreground")
        return {"sem": np.array([1]), "ins": np.array([1])}

    with pytest.raises(ValueError, match="b: no foreground"):
        inference.infer_paths(pipeline, ["a", "b", "c"])
    got = inference.infer_paths(pipeline, ["a", "b", "c"], on_error="skip")
    assert set(got[0]) == set(got[2]) == {"sem", "ins"} and set(got[1]) == {"error"} and "b: no foreground" in got[1]["error"]
