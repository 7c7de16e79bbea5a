"""CPU: libtgn_pointops.so loads and exports every function declared in include/*.h, the ctypes
signature table covers them, and the product path refuses CPU tensors (no fallback).  No compute."""
import ctypes
import glob
import os
import re

import pytest
import torch

from conftest import REPO


def _declared_functions():
    names = []
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)  # preprocessor lines
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{}]*\)\s*;", src):
            if m.group(1) not in ("defined",):
                names.append(m.group(1))
    return sorted(set(names))


def test_header_declares_the_reference_launchers():
    names = _declared_functions()
    for ref in ["furthestsampling_cuda_launcher", "knnquery_cuda_launcher", "grouping_forward_cuda_launcher",
                "grouping_backward_cuda_launcher", "interpolation_forward_cuda_launcher",
                "interpolation_backward_cuda_launcher", "subtraction_forward_cuda_launcher",
                "subtraction_backward_cuda_launcher", "aggregation_forward_cuda_launcher",
                "aggregation_backward_cuda_launcher"]:
        assert ref in names
    assert len(names) >= 30


def test_library_exports_every_declared_symbol():
    from toothgroupnetwork_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(handle, name), f"{name} declared in include/ but not exported"


_C_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
              "size_t": ctypes.c_size_t}
_C_TYPE_WORDS = {"void", "char", "short", "int", "long", "unsigned", "float", "double", "size_t", "tgn_stream_t", "*"}


def _ctype(decl):
    """The ctypes mirror of one C result or parameter declaration: char * (const or not) -> c_char_p, any other pointer and
    tgn_stream_t -> c_void_p, void -> None, a scalar -> its own type (an unknown one is a KeyError)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if words[-1] not in _C_TYPE_WORDS:
        words = words[:-1]                                          # the parameter's name
    if "*" in words:
        return ctypes.c_char_p if words == ["char", "*"] else ctypes.c_void_p
    if words == ["tgn_stream_t"]:
        return ctypes.c_void_p
    return None if words == ["void"] else _C_SCALARS[" ".join(words)]


def _declared_signatures():
    """name -> (restype, [argtypes]) of every function declared in include/*.h, in the form of _lib.SIGNATURES."""
    out = {}
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)
        for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_\s*]*?)\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{}()]*)\)\s*;", src):
            args = m.group(3).strip()
            out[m.group(2)] = (_ctype(m.group(1)), [] if args in ("", "void") else [_ctype(a) for a in args.split(",")])
    return out


def test_ctypes_table_matches_header():
    from toothgroupnetwork_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_functions()
    declared = _declared_signatures()
    for name, (res, args) in _lib.SIGNATURES.items():     # a wrong count is a TypeError at call time, a wrong type garbage in the kernel
        assert (res, list(args)) == declared[name], (name, (res, list(args)), declared[name])
    L = _lib.lib()
    assert b"gfx950" in L.tgn_version()
    assert L.tgn_fps_resident_capacity() >= 24000  # a whole 24 000-point scan stays in registers
    assert L.tgn_ball_query_workspace_bytes(1, 24000, 4096) >= 0


def test_checked_view_checks_every_status_function():
    """ops() raises for every c_int function that is not listed as value-returning, so a new entry point cannot go unchecked by
    accident; the raw view checks nothing."""
    from toothgroupnetwork_amd import _lib
    ints = {name for name, (res, _) in _lib.SIGNATURES.items() if res is ctypes.c_int}
    assert _lib.VALUE_RETURNING <= ints, sorted(_lib.VALUE_RETURNING - ints)
    O, L = _lib.ops(), _lib.lib()
    for name in _lib.SIGNATURES:
        want = _lib._raise_on_status if name in ints - _lib.VALUE_RETURNING else None
        assert getattr(O, name).errcheck is want, name
        assert getattr(L, name).errcheck is None, name


def test_checked_view_raises_with_the_name_of_the_function_that_failed():
    """The two refusals below (the raw view's status 3, before any launch) as the package's operators see them."""
    from toothgroupnetwork_amd import _lib
    O = _lib.ops()
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    with pytest.raises(RuntimeError) as e:
        O.tgn_knnquery(1, 1, 129, p, p, p, p, p, p, None)
    assert str(e.value) == ("libtgn_pointops tgn_knnquery failed (status 3): "
                            "tgn_knnquery: nsample 129 > 128 unsupported (the reference's limit is 100)")
    with pytest.raises(RuntimeError, match=r"^libtgn_pointops tgn_pt_attention_forward failed \(status 3\): .*\(got 12\)$"):
        O.tgn_pt_attention_forward(1, 4, 24, 12, *([p] * 18), None)


def test_checked_view_converts_pointer_arguments():
    """tgn_furthestsampling_dense with B = 0 returns TGN_OK before it looks at a pointer or makes a HIP call: None and c_void_p pass,
    a CPU tensor (whose address must never reach a kernel) and anything that is no pointer are refused before the call."""
    from toothgroupnetwork_amd import _lib
    O = _lib.ops()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert O.tgn_furthestsampling_dense(0, 0, 0, None, None, None, None, 0, None) == 0
    assert O.tgn_furthestsampling_dense(0, 0, 0, p, None, p, p, 0, ctypes.c_void_p(0)) == 0
    with pytest.raises(ctypes.ArgumentError, match="no CPU fallback"):
        O.tgn_furthestsampling_dense(0, 0, 0, torch.zeros(3), None, None, None, 0, None)
    with pytest.raises(ctypes.ArgumentError, match="TypeError: expected a CUDA tensor, None or a c_void_p, got int"):
        O.tgn_furthestsampling_dense(0, 0, 0, ctypes.addressof(buf), None, None, None, 0, None)


def test_checked_view_leaves_value_returning_functions_alone():
    from toothgroupnetwork_amd import _lib
    O, L = _lib.ops(), _lib.lib()
    assert O.tgn_get_tuning(b"fps_lean", -1) == L.tgn_get_tuning(b"fps_lean", -1) != -1
    assert O.tgn_get_tuning(b"no_such_switch", 77) == 77
    assert O.tgn_fps_resident_capacity() == L.tgn_fps_resident_capacity() >= 24000


def test_knnquery_refuses_more_than_128_neighbours_before_any_launch():
    """The exact-heap kernel keeps kKnnHeapMax = 128 entries per query in LDS and there is no other kernel behind it: a larger
    nsample is TGN_ERR_UNSUPPORTED with its message.  The check comes before the first HIP call (the buffers are never
    touched), so it holds without a device."""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.tgn_knnquery(1, 1, 129, p, p, p, p, p, p, None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert L.tgn_last_error().decode() == "tgn_knnquery: nsample 129 > 128 unsupported (the reference's limit is 100)"


def test_pt_attention_refuses_an_uninstantiated_width_before_any_launch():
    """tgn_pt_attention_forward passes its argument checks with 12 weight channels (at least 4, dividing c = 24), but the kernel exists
    for 4, 8, 16, 32 and 64 only: the dispatch (csrc/dispatch.h) matches nothing, launches nothing and says which value it got."""
    from toothgroupnetwork_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # x_k / x_v must be 16-byte aligned
    rc = L.tgn_pt_attention_forward(1, 4, 24, 12, *([p] * 18), None)
    assert rc == _lib.ERR_UNSUPPORTED
    assert L.tgn_last_error().decode() == "tgn_pt_attention_forward: weight channels must be 4, 8, 16, 32 or 64 (got 12)"


def test_ops_refuse_cpu_tensors_loudly():
    from toothgroupnetwork_amd import pointnet2_utils as U, pointops as P
    xyz = torch.rand(1, 64, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.farthest_point_sample(xyz, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.query_ball_point(0.2, 4, xyz, xyz[:, :4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.furthestsampling(xyz[0], torch.tensor([64], dtype=torch.int32), torch.tensor([8], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.knnquery(4, xyz[0], xyz[0], torch.tensor([64], dtype=torch.int32), torch.tensor([64], dtype=torch.int32))


def test_missing_library_fails_loudly(monkeypatch):
    from toothgroupnetwork_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libtgn_pointops.so")
    with pytest.raises(_lib.TgnLibraryError, match="not been built"):
        _lib.lib()
    with pytest.raises(_lib.TgnLibraryError, match="not been built"):
        _lib.ops()


def test_product_never_imports_the_oracle():
    bad = []
    for root in ("toothgroupnetwork_amd", "external_libs", "tools"):    # shipped runners and benches included
        for dirpath, _, files in os.walk(os.path.join(REPO, root)):
            for f in files:
                if f.endswith(".py"):
                    txt = open(os.path.join(dirpath, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M):
                        bad.append(os.path.join(dirpath, f))
    txt = open(os.path.join(REPO, "pointops_cuda.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M)
    assert bad == []
