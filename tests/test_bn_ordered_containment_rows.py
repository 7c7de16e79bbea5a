"""The containment rows of tgn_bn_rows_forward_ordered and tgn_bn_rows_backward_ordered (csrc/bnorm.hip), added to the table of
tests/containment_cases.py through its row(...) function when this module is imported -- once: a second import finds the names
covered and adds nothing.

pytest collects tests/ in name order and this file's name sorts before tests/test_containment_host.py and
tests/test_gpu_containment.py, so in a run over tests/ the completeness and hygiene tests of the first see the two rows and the
parametrised GPU test of the second runs them like every other row: three runs per shape on guarded operands, bytes compared.

Limit, as for tests/test_bwd_ordered_containment_rows.py: either of those two files run ALONE does not import this one, reports the two
entry points as missing and runs no case of theirs.  The suite commands over tests/ are the check.

Operands are those of the tgn_bn_rows_* rows (multiples of 1/16; save_mean on that grid and save_invstd = 1/2 in the backward), but for
the workspace: exactly tgn_bn_rows_ordered_workspace_bytes(rows, C) bytes that start as the arena's fill, two different fills in the
two guarded runs (the header: any contents).  Neither call has a float atomic: bytes are compared.

Shapes (rows, C, running statistics given, relu), the seams of tests/test_gpu_bn_ordered.py: one block and one column; the widest C at
the fewest rows; C that does not divide 256, the block count rounded to a multiple of C / gcd(256, C); C > 256, a block keeps only
part of the columns and zero-fills the rest of its partials; one element and an odd tail past a block's 8192, both the four-in-flight
loop and its tail; the 1024-block cap."""
import torch

import containment_cases as T

NAMES = ("tgn_bn_rows_forward_ordered", "tgn_bn_rows_backward_ordered")
SHAPES = [(2, 1, True, True), (2, 1024, True, False), (7, 3, False, True), (1000, 35, True, True), (300, 320, False, False),
          (8193, 4, True, False), (8197, 4, False, True), (262145, 32, True, True)]


def _ws(shape):
    return T.W("ws", T._L().tgn_bn_rows_ordered_workspace_bytes(shape[0], shape[1]))


def _fwd_build(shape):
    return [op for op in T._bn_fwd_build(shape) if op[0] != "ws"] + [_ws(shape)]


def _bwd_build(shape):
    return [op for op in T._bn_bwd_build(shape) if op[0] != "ws"] + [_ws(shape)]


def _register():
    if set(NAMES) & T.covered():
        return
    P = T.P
    T.row("tgn_bn_rows_forward_ordered", ["tgn_bn_rows_forward_ordered"], SHAPES, _fwd_build,
          lambda s: lambda L, v, st: L.tgn_bn_rows_forward_ordered(s[0], s[1], P(v["x"]), P(v["gamma"]), P(v["beta"]), 1e-5, 0.1, P(v.get("running_mean")),
                                                                   P(v.get("running_var")), P(v.get("nbt")), int(s[3]), P(v["y"]), P(v["save_mean"]),
                                                                   P(v["save_invstd"]), P(v["ws"]), v["ws"].numel(), st),
          sizes={"ws": "tgn_bn_rows_ordered_workspace_bytes"}, compare="bytes")
    T.row("tgn_bn_rows_backward_ordered", ["tgn_bn_rows_backward_ordered"], SHAPES, _bwd_build,
          lambda s: lambda L, v, st: L.tgn_bn_rows_backward_ordered(s[0], s[1], P(v["x"]), P(v["y"]), P(v["dy"]), P(v["gamma"]), P(v["save_mean"]),
                                                                    P(v["save_invstd"]), int(s[3]), P(v["dx"]), P(v["dgamma"]), P(v["dbeta"]), P(v["ws"]),
                                                                    v["ws"].numel(), st),
          sizes={"ws": "tgn_bn_rows_ordered_workspace_bytes"}, compare="bytes")


_register()


def test_both_entry_points_have_a_row():
    assert set(NAMES) <= T.covered()
    _register()                                                    # a second registration adds nothing
    assert sorted(r["name"] for r in T.ROWS if set(r["covers"]) & set(NAMES)) == sorted(NAMES)
    assert all(r["compare"] == "bytes" and r["after"] is None for r in T.ROWS if r["name"] in NAMES)


def test_the_rows_build_on_the_cpu_with_a_workspace_as_large_as_the_size_function_says():
    import bn_ordered_ref as R
    by_name = {r["name"]: r for r in T.ROWS}
    for shape in SHAPES:
        rows, C, running, relu = shape
        for name, outputs in ((NAMES[0], {"y": (rows, C), "save_mean": (C,), "save_invstd": (C,)}), (NAMES[1], {"dx": (rows, C), "dgamma": (C,), "dbeta": (C,)})):
            ops = {n: x for n, _, x in by_name[name]["build"](shape)}
            assert ops["ws"] == ((R.workspace_bytes(rows, C),), torch.uint8), "the arena's fill, not zeros: the header allows any contents"
            for out, want in outputs.items():
                assert ops[out] == (want, torch.float32)
            assert tuple(ops["x"].shape) == (rows, C) and (("running_mean" in ops) == running or name == NAMES[1])
    assert any(s[1] > 256 for s in SHAPES) and any(256 % s[1] for s in SHAPES) and any(R.grid(s[0], s[1]) == 1024 for s in SHAPES)
