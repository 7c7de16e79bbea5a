"""Host: the table of tests/containment_cases.py is complete and well-formed, and the checks of tests/arena.py have teeth.

No GPU: completeness and hygiene read the table and _lib.SIGNATURES; the self-test plants three defects with plain torch
operations on an arena built on the CPU and shows that each is reported and that a clean call is not."""
import ctypes

import pytest
import torch

import containment_cases as T
from arena import CANARY, CANARY_B, Arena, compare_outputs, run_guarded, run_plain


def _pointer_entry_points():
    from toothgroupnetwork_amd import _lib
    return {name for name, (_, args) in _lib.SIGNATURES.items() if ctypes.c_void_p in args}


def test_every_entry_point_with_a_pointer_has_a_row_or_a_reason():
    from toothgroupnetwork_amd import _lib
    need, covered = _pointer_entry_points(), T.covered()
    unknown = (covered | set(T.EXEMPT)) - set(_lib.SIGNATURES)
    assert not unknown, f"not in _lib.SIGNATURES: {sorted(unknown)}"
    missing = need - covered - set(T.EXEMPT)
    assert not missing, f"entry points with a pointer argument and neither a row in tests/containment_cases.py nor a reason in EXEMPT: {sorted(missing)}"
    both = covered & set(T.EXEMPT)
    assert not both, f"covered by a row AND exempt: {sorted(both)}"
    print(f"\n{len(need)} entry points take a pointer: {len(covered)} covered by {len(T.ROWS)} rows, {len(T.EXEMPT)} exempt")


def test_exempt_holds_the_three_categories_only():
    for name, reason in T.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 20, (name, reason)
        if name in T.EXEMPT_HOST:
            assert reason.startswith(T._HOST), (name, reason)
        elif name.endswith("_cuda_launcher"):
            assert reason == T._FWD and ("tgn_" + name[:-len("_cuda_launcher")]) in T.covered(), name
        else:
            assert name.startswith("tgn_sa_") and reason == T._SA, f"{name}: not one of the three categories EXEMPT may hold"
    assert sum(n.endswith("_cuda_launcher") for n in T.EXEMPT) == 10
    assert set(T.EXEMPT_HOST) <= set(T.EXEMPT)


def test_row_hygiene():
    from toothgroupnetwork_amd import _lib
    names = [r["name"] for r in T.ROWS]
    assert len(set(names)) == len(names), "row names repeat"
    for r in T.ROWS:
        assert r["covers"] and len(r["shapes"]) >= 1 and len(r["tunings"]) >= 1, r["name"]
        assert r["compare"] in ("bytes", "bound"), r["name"]
        if r["compare"] == "bound":
            assert set(r["covers"]) <= set(T.BOUND_ALLOWED), f"{r['name']}: compare='bound' is allowed for {T.BOUND_ALLOWED} only"
        for ws, fn in r["sizes"].items():
            assert fn.startswith("header: ") or (fn.endswith("_workspace_bytes") and fn in _lib.SIGNATURES), (r["name"], ws, fn)
    assert set(T.BOUND_ALLOWED) == {"tgn_pt_softmax_aggregate_backward", "tgn_aggregation_backward"}


def test_every_workspace_operand_names_its_size_function():
    """every row's operands, built on the CPU (the size functions need no device): names are unique, a `ws` operand has its size
    function in the row, the roles are the arena's"""
    for r in T.ROWS:
        for si in range(len(r["shapes"])):
            ops = r["build"](r["shapes"][si])
            names = [o[0] for o in ops]
            assert len(set(names)) == len(names), (r["name"], names)
            for name, role, x in ops:
                assert role in ("in", "out", "ws"), (r["name"], name, role)
                assert role != "ws" or name in r["sizes"], f"{r['name']}: workspace {name} has no size function named in its row"
                assert role != "in" or torch.is_tensor(x), f"{r['name']}: input {name} has no contents"
            assert any(role != "in" for _, role, _ in ops), r["name"]


# ---------------------------------------------------------------------------------------------------------------------------
# the harness on the CPU: three planted defects and a clean call
# ---------------------------------------------------------------------------------------------------------------------------
N = 37
OPERANDS = [("x", "in", torch.arange(N, dtype=torch.float32)), ("y", "out", ((N,), torch.float32)), ("ws", "ws", ((64,), torch.uint8))]
CPU = torch.device("cpu")


def _clean(v):
    """y = 2 x, the workspace scribbled on"""
    v["y"].copy_(v["x"] * 2)
    v["ws"].fill_(7)
    return 0


def _behind(t, nbytes):
    """the `nbytes` bytes behind the last element of view t, as a uint8 view of the same storage"""
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), t.storage_offset() * t.element_size() + t.numel() * t.element_size(),
                                                  (nbytes,), (1,))


def _three_runs(call):
    a = run_guarded(OPERANDS, call, CANARY, CPU, "self-test, run A")
    b = run_guarded(OPERANDS, call, CANARY_B, CPU, "self-test, run B")
    c = run_plain(OPERANDS, call, CPU)
    return a[1], b[1], c[1]


def test_harness_passes_a_clean_call():
    a, b, c = _three_runs(_clean)
    compare_outputs(a, b, "A against B")
    compare_outputs(a, c, "A against C")
    assert torch.equal(a["y"].view(torch.float32), torch.arange(N, dtype=torch.float32) * 2)


def test_harness_reports_a_write_one_byte_past_the_output():
    def call(v):
        _clean(v)
        if v["y"].untyped_storage().nbytes() > 4 * N + 64:      # (in the arena: run C's own allocation ends with the output)
            _behind(v["y"], 1).fill_(0)
        return 0
    with pytest.raises(AssertionError, match=r"1 bytes outside the outputs changed.*the guard band 0 bytes behind y"):
        run_guarded(OPERANDS, call, CANARY, CPU, "planted overrun")
    with pytest.raises(AssertionError, match="behind y"):
        run_guarded(OPERANDS, call, CANARY_B, CPU, "planted overrun")


def test_harness_reports_a_write_past_the_workspace_and_into_an_input():
    def past_ws(v):
        _clean(v)
        _behind(v["ws"], 3).fill_(1)
        return 0
    with pytest.raises(AssertionError, match="3 bytes outside the outputs changed.*behind ws"):
        run_guarded(OPERANDS, past_ws, CANARY, CPU, "planted workspace overrun")

    def into_input(v):
        _clean(v)
        v["x"][5] = -1.0
        return 0
    with pytest.raises(AssertionError, match=r"x at byte 2[0-3] of 148"):
        run_guarded(OPERANDS, into_input, CANARY, CPU, "planted input write")


def test_harness_reports_an_element_read_behind_an_input():
    def call(v):
        _clean(v)
        if v["x"].untyped_storage().nbytes() > 4 * N + 64:
            v["y"][N - 1] = _behind(v["x"], 4).view(torch.float32)[0]       # the padded lane took its neighbour's value
        return 0
    a, b, c = _three_runs(call)
    with pytest.raises(AssertionError, match="output y differs in 4 of 148 bytes, the first at byte 144"):
        compare_outputs(a, b, "A against B")
    with pytest.raises(AssertionError, match="output y differs"):
        compare_outputs(a, c, "A against C")


def test_harness_reports_an_output_element_nobody_wrote():
    def call(v):
        v["y"][:N - 1].copy_(v["x"][:N - 1] * 2)
        return 0
    a, b, c = _three_runs(call)
    with pytest.raises(AssertionError, match="output y differs in 4 of 148 bytes, the first at byte 144"):
        compare_outputs(a, b, "A against B")
    with pytest.raises(AssertionError, match="output y differs"):
        compare_outputs(a, c, "A against C")


def test_arena_roles_fill_and_prefilled_outputs():
    ar = Arena(fill=0x11)
    ar.add("w", like=torch.ones(5), role="in")
    ar.add("acc", like=torch.zeros(3), role="out")
    ar.add("o", shape=(2,), dtype=torch.int32, role="out")
    ar.add("s", like=torch.zeros(8, dtype=torch.uint8), role="ws")
    w, acc, o, s = ar.build(CPU)
    assert int(o[0]) == 0x11111111 and float(acc.sum()) == 0.0 and int(ar.buf[0]) == 0x11 and Arena().fill == CANARY
    acc += 1
    o.fill_(4)
    s.fill_(9)
    ar.check("writes to out and ws only")
    assert set(ar.out_bytes()) == {"acc", "o"}       # a workspace is never compared
    ar.reset_outputs()
    assert float(acc.sum()) == 0.0 and int(s.sum()) == 0
    w[0] = 2
    with pytest.raises(AssertionError, match=r"w at byte [0-3] of 20"):
        ar.check("an input changed")
