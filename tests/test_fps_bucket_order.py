"""CPU: the order in which fps_bucket_kernel deals grid cells out to its buckets (a Hilbert curve over 16^3 cells, exported by
tgn_fps_bucket_order), and tools/fps_bucket_model.py, the numpy restatement of the kernel's bookkeeping built on it."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from toothgroupnetwork_amd import synth


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("fps_bucket_model", os.path.join(REPO, "tools", "fps_bucket_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    from toothgroupnetwork_amd import _lib
    out = np.full(4096, 0xFFFF, dtype=np.uint16)
    _lib.check(_lib.lib().tgn_fps_bucket_order(4, out.ctypes.data_as(ctypes.c_void_p)), "tgn_fps_bucket_order")
    return out


def test_table_is_a_permutation(table):
    assert np.array_equal(np.sort(table.astype(np.int64)), np.arange(4096))


def test_consecutive_indices_are_face_adjacent_cells(table):
    cell = np.argsort(table.astype(np.int64))                     # curve position -> cell x | y << 4 | z << 8
    xyz = np.stack([cell & 15, (cell >> 4) & 15, cell >> 8], axis=1)
    step = np.abs(np.diff(xyz, axis=0))
    assert np.array_equal(step.sum(axis=1), np.ones(4095, dtype=step.dtype))      # one step along one axis


def test_index_zero_is_a_corner_cell(table):
    cell = int(np.argsort(table.astype(np.int64))[0])
    assert all(c in (0, 15) for c in (cell & 15, (cell >> 4) & 15, cell >> 8))


def test_export_refuses_other_grids():
    from toothgroupnetwork_amd import _lib
    out = np.zeros(32768, dtype=np.uint16)
    assert _lib.lib().tgn_fps_bucket_order(5, out.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib().tgn_fps_bucket_order(4, None) == _lib.ERR_INVALID_ARGUMENT


def test_model_mapping_equals_the_kernels_table(model, table):
    assert np.array_equal(model.hilbert_table(4), table)
    assert np.array_equal(model.library_table(4), table)          # the tool's own way to the library


@pytest.mark.parametrize("order", ["hilbert", "z", "kd"])
@pytest.mark.parametrize("cloud,n,m,nt,p", [("uniform", 2000, 256, 256, 8), ("arch", 6000, 512, 512, 16)])
def test_model_samples_equal_the_oracle(model, oracle, order, cloud, n, m, nt, p):
    xyz = synth.uniform_cloud(n, seed=11) if cloud == "uniform" else synth.arch_cloud(n, 12, False)
    idx, stats = model.simulate(xyz, m, order=order, bits=4, perm=3, nt=nt, p=p)
    assert np.array_equal(idx, oracle.farthest_point_sample(xyz[None], m)[0])
    assert np.array_equal(idx, model.plain_fps(xyz, m))           # what the tool's --check compares with
    assert stats["buckets"] == -(-n // 64) and 1.0 <= stats["busiest_touched"] <= stats["touched"] <= stats["buckets"]
    assert stats["refreshed"] <= stats["changed"] <= stats["touched"]
