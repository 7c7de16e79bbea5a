"""CPU: the midpoint-subdivision contract (include/tgn_pointops.h: tgn_subdivide_midpoint) as tests/subdivide_ref.py states it twice --
the two statements agree in bits on the shared case list and their output has the structure the contract promises -- and the checks of
the C ABI and of preprocess.subdivide_midpoint that come before any device call.  No compute on a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subdivide_ref as S  # noqa: E402

CASES = ["one_triangle", "shared_edge_opposite", "shared_edge_same", "tetrahedron", "edge_of_three_triangles", "repeated_index",
         "unreferenced_vertex", "no_normals", "arch_shuffled", "arch_rotated"]


def test_the_case_list_is_what_the_names_say():
    c = S.cases()
    assert sorted(c) == sorted(CASES)
    assert "vertex_normals" not in c["no_normals"] and all("vertex_normals" in m for k, m in c.items() if k != "no_normals")
    assert c["arch_shuffled"]["vertices"].shape == (1200, 3) and c["arch_shuffled"]["triangles"].shape == (2262, 3)
    a, b = c["arch_shuffled"]["triangles"], c["arch_rotated"]["triangles"]
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1))
    base = S.arch_mesh(40, 30, 5)["triangles"]
    assert not np.array_equal(a, base) and np.array_equal(np.unique(a, axis=0), np.unique(base, axis=0)), "the same triangles, out of order"


def _edges(t):
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return {(min(p, q), max(p, q)) for p, q in e.tolist()}


@pytest.mark.parametrize("name", CASES)
def test_the_two_statements_agree_in_bits(name):
    mesh = S.cases()[name]
    assert S.same_bits(S.reference(name), S.subdivide_unique(mesh))
    if mesh["triangles"].shape[0] <= 16:                               # twice: the second pass walks the first one's output
        assert S.same_bits(S.reference(name, 2), S.subdivide_unique(mesh, 2))


@pytest.mark.parametrize("name", CASES)
def test_structure_of_the_output(name):
    mesh, out = S.cases()[name], S.reference(name)
    v, t = mesh["vertices"], mesh["triangles"]
    nv, nf, E = v.shape[0], t.shape[0], len(_edges(t))
    assert set(out) == set(mesh)
    assert out["vertices"].shape == (nv + E, 3) and out["triangles"].shape == (4 * nf, 3)
    assert np.array_equal(out["vertices"][:nv].view(np.int64), v.view(np.int64)), "old vertices keep their indices and bits"
    if "vertex_normals" in mesh:
        n = out["vertex_normals"]
        assert n.shape == (nv + E, 3) and np.array_equal(n[:nv].view(np.int64), mesh["vertex_normals"].view(np.int64))
    nt = out["triangles"]
    assert nt.min() >= 0 and nt.max() < nv + E
    assert np.array_equal(np.unique(nt[nt >= nv]), np.arange(nv, nv + E)), "every new vertex is used"
    # every child keeps its parent's orientation: the children are built from midpoints, so each child's area vector is exactly a
    # quarter of the parent's up to rounding -- the same direction wherever the parent is not degenerate
    ov = out["vertices"]
    parent = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    child = np.cross(ov[nt[:, 1]] - ov[nt[:, 0]], ov[nt[:, 2]] - ov[nt[:, 0]]).reshape(nf, 4, 3)
    solid = np.linalg.norm(parent, axis=1) > 0
    assert solid.sum() >= nf - 2
    cosine = (child * parent[:, None, :]).sum(-1) / (np.linalg.norm(child, axis=2) * np.linalg.norm(parent, axis=1)[:, None] + 1e-300)
    assert (cosine[solid] > 1.0 - 1e-6).all()


def test_the_tetrahedron_keeps_euler_characteristic_two():
    for k in (1, 2):
        out = S.reference("tetrahedron", k)
        V, F, E = out["vertices"].shape[0], out["triangles"].shape[0], len(_edges(out["triangles"]))
        assert (V, E, F) == {1: (10, 24, 16), 2: (34, 96, 64)}[k] and V - E + F == 2


def test_first_occurrence_order_by_hand():
    """Two triangles sharing edge {1, 2} with opposite orientation: the walk meets (0,1), (1,2), (2,0), then (2,1) again, (1,3), (3,2)."""
    mesh = S.cases()["shared_edge_opposite"]
    out = S.reference("shared_edge_opposite")
    v = mesh["vertices"]
    want = [0.5 * (v[0] + v[1]), 0.5 * (v[1] + v[2]), 0.5 * (v[0] + v[2]), 0.5 * (v[1] + v[3]), 0.5 * (v[2] + v[3])]
    assert np.array_equal(out["vertices"][4:], np.array(want))
    assert out["triangles"].tolist() == [[0, 4, 6], [4, 1, 5], [5, 2, 6], [4, 5, 6],
                                         [2, 5, 8], [5, 1, 7], [7, 3, 8], [5, 7, 8]]
    rep = S.reference("repeated_index")                                # (0, 0, 1): the edge {0, 0} gets a copy of vertex 0
    assert np.array_equal(rep["vertices"][3], S.cases()["repeated_index"]["vertices"][0])


def test_capi_refuses_two_to_the_31_before_any_launch():
    """nv + 3 nf >= 2^31 is TGN_ERR_UNSUPPORTED with a message that names the limit; negative counts and NULL pointers are
    TGN_ERR_INVALID_ARGUMENT.  All of it comes before the first HIP call (the buffers are never touched), so it holds without a device."""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for nv, nf in ((2 ** 31 - 3, 1), (0, (2 ** 31 + 2) // 3), (2 ** 31, 0), (5, 2 ** 40)):
        rc = L.tgn_subdivide_midpoint(nv, nf, p, p, p, p, p, p, p, p, 64, None)
        assert rc == _lib.ERR_UNSUPPORTED, (nv, nf)
        assert L.tgn_last_error().decode() == (f"tgn_subdivide_midpoint: nv + 3 * nf >= 2147483648 unsupported (nv={nv} nf={nf}; vertex indices "
                                               "and half-edge numbers are 32-bit)")
    assert L.tgn_subdivide_midpoint_workspace_bytes((2 ** 31 + 2) // 3) == 0 and L.tgn_subdivide_midpoint_workspace_bytes(-1) == 0
    assert L.tgn_subdivide_midpoint(-1, 1, p, p, p, p, p, p, p, p, 64, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.tgn_subdivide_midpoint(1, -1, p, p, p, p, p, p, p, p, 64, None) == _lib.ERR_INVALID_ARGUMENT
    for missing in (2, 4, 5, 7, 8, 9):                                 # vertices, triangles, out_vertices, out_triangles, n_new, workspace
        args = [3, 1] + [p] * 8 + [64, None]
        args[missing] = None
        assert L.tgn_subdivide_midpoint(*args) == _lib.ERR_INVALID_ARGUMENT, missing
    args = [3, 1] + [p] * 8 + [64, None]
    args[6] = None                                                     # normals without out_normals
    assert L.tgn_subdivide_midpoint(*args) == _lib.ERR_INVALID_ARGUMENT
    # a workspace one byte short is refused too (still before any HIP call)
    need = L.tgn_subdivide_midpoint_workspace_bytes(1)
    assert need >= 1024 * 12 + 3 * 8
    assert L.tgn_subdivide_midpoint(3, 1, p, p, p, p, p, p, p, p, need - 1, None) == _lib.ERR_INVALID_ARGUMENT


def test_workspace_grows_with_the_table():
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    sizes = [L.tgn_subdivide_midpoint_workspace_bytes(nf) for nf in (0, 1, 170, 171, 2262, 13662)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # capacity: a power of two of at least 2 * 3 nf, 12 bytes a slot; 8 bytes a half-edge; each array rounded up to 256 bytes
    assert sizes[3] - sizes[2] >= 2048 * 12 - 1024 * 12, "3 * 171 = 513 half-edges need 2048 slots, 3 * 170 = 510 fit 1024"
    assert sizes[5] >= 131072 * 12 + 3 * 13662 * 8


def test_wrapper_checks_come_before_any_device_call(monkeypatch):
    """An out-of-range index and number_of_iterations = 0 are ValueError on a machine without a GPU, and the library is never asked."""
    from toothgroupnetwork_amd import _lib, preprocess
    mesh = S.cases()["unreferenced_vertex"]

    def no_library():
        raise AssertionError("the check must come before the library is touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="number_of_iterations"):
        preprocess.subdivide_midpoint(mesh, number_of_iterations=0)
    bad = dict(mesh, triangles=np.array([[0, 1, 2], [2, 1, 6], [0, -1, 2]], dtype=np.int64))
    with pytest.raises(ValueError, match=r"triangle 1 = \[2, 1, 6\] has an index outside \[0, 6\)"):
        preprocess.subdivide_midpoint(bad)
    bad = dict(mesh, triangles=np.array([[0, 1, 2], [0, -1, 2]], dtype=np.int64))
    with pytest.raises(ValueError, match=r"triangle 1 = \[0, -1, 2\]"):
        preprocess.subdivide_midpoint(bad)
    # no triangles: copies, no device
    empty = dict(mesh, triangles=np.zeros((0, 3), dtype=np.int64))
    out = preprocess.subdivide_midpoint(empty, 3)
    assert S.same_bits(out, {k: np.ascontiguousarray(v) for k, v in empty.items()})
    assert all(out[k] is not empty[k] and not np.shares_memory(out[k], empty[k]) for k in out)


def test_pipelines_refuse_a_mesh_that_cannot_reach_24000_before_any_launch(monkeypatch):
    """nv + 3 nf <= 24 000 decides it on the host: NotImplementedError with the reference's own failure named, no library call."""
    from toothgroupnetwork_amd import _lib, inference

    def no_library():
        raise AssertionError("decided on the host")
    monkeypatch.setattr(_lib, "lib", no_library)
    assert inference.needs_subdivision(24000, 1) is False and inference.needs_subdivision(30000, 50000) is False
    assert inference.needs_subdivision(23999, 1) is True            # 23 999 + 3 > 24 000: only the pass can tell
    assert inference.needs_subdivision(7000, 13662) is True
    for nv, nf in ((1200, 2262), (23997, 1), (0, 0)):
        with pytest.raises(NotImplementedError, match="the reference fails on such a mesh too"):
            inference.needs_subdivision(nv, nf)
