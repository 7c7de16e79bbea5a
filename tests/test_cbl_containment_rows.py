"""The containment rows of tgn_cbl_stage_forward and tgn_cbl_stage_backward (csrc/cbl.hip), added to the table of
tests/containment_cases.py through its row(...) function when this module is imported -- once: a second import finds the names
covered and adds nothing.

pytest collects tests/ in name order and this file's name sorts before tests/test_containment_host.py and
tests/test_gpu_containment.py, so in a run over tests/ the completeness and hygiene tests of the first see the two rows and the
parametrised GPU test of the second runs them like every other row: three runs per shape on guarded operands, bytes compared.

Limit: `pytest tests/test_containment_host.py` (or tests/test_gpu_containment.py) run ALONE does not import this file, reports the two
entry points as missing and runs no case of theirs.  The suite commands, `pytest -m "not gpu"` and `pytest -m gpu` over tests/, are
the check.

Operands: latent features are multiples of 1/64 in [-1, 1], neighbour indices and labels are valid, the workspace is exactly
tgn_cbl_stage_workspace_bytes(m), every output exactly what the header states.  The backward's pair weights are multiples of 1/1024
with exact zeros among them (a skipped pair), its lists are ordered_ref.reverse_lists_torch of the same indices, built on the CPU.  Neither call
has a float atomic, so the three runs compare bytes.  Shapes (m, k1, c): the smallest of everything; one point past a workgroup of the
forward at the criterion's own width; the widest list at the two-pieces-per-lane-group width with several workgroups; the widest row,
35 slots (the first stage's list) and a last workgroup that is not full."""
import torch

import containment_cases as T
import ordered_ref
from operator_forms import gen_for, q16

F32, I32, I64 = torch.float32, torch.int32, torch.int64
NAMES = ("tgn_cbl_stage_forward", "tgn_cbl_stage_backward")


def _shapes():
    from toothgroupnetwork_amd import losses
    return [(1, 1, 4), (losses.CBL_FUSED_BLOCK_POINTS + 1, 8, 32), (300, 63, 64), (130, 35, 128)]


def _inputs(shape):
    m, k1, c = shape
    g = gen_for(f"cbl_stage{m}")
    return g, [T.I("f", q16(g, m, c) / 4), T.I("idx", T.ridx(g, m, (m, k1)))]


def _fwd_build(shape):
    m, k1, c = shape
    g, ops = _inputs(shape)
    return ops + [T.I("labels", T.ridx(g, 3, (m,), I64)), T.O("loss", (1,)), T.O("count", (1,), I64), T.O("pair_w", (m, k1)),
                  T.W("ws", T._L().tgn_cbl_stage_workspace_bytes(m))]


def _bwd_build(shape):
    m, k1, c = shape
    g, ops = _inputs(shape)
    rev_start, rev_pair = ordered_ref.reverse_lists_torch(ops[1][2])
    return ops + [T.I("pair_w", q16(g, m, k1) / 64), T.I("count", torch.tensor([max(m // 2, 1)], dtype=I64)), T.I("rev_start", rev_start),
                  T.I("rev_pair", rev_pair), T.I("grad_loss", torch.tensor([0.75], dtype=F32)), T.O("grad_f", (m, c))]


def _register():
    if set(NAMES) & T.covered():
        return
    P = T.P
    T.row("tgn_cbl_stage_forward", ["tgn_cbl_stage_forward"], _shapes(), _fwd_build,
          lambda s: lambda L, v, st: L.tgn_cbl_stage_forward(s[0], s[1], s[2], P(v["f"]), P(v["idx"]), P(v["labels"]), P(v["loss"]), P(v["count"]),
                                                             P(v["pair_w"]), P(v["ws"]), v["ws"].numel(), st),
          sizes={"ws": "tgn_cbl_stage_workspace_bytes"}, compare="bytes")
    T.row("tgn_cbl_stage_backward", ["tgn_cbl_stage_backward"], _shapes(), _bwd_build,
          lambda s: lambda L, v, st: L.tgn_cbl_stage_backward(s[0], s[1], s[2], P(v["f"]), P(v["idx"]), P(v["pair_w"]), P(v["count"]),
                                                              P(v["rev_start"]), P(v["rev_pair"]), P(v["grad_loss"]), P(v["grad_f"]), st),
          compare="bytes")


_register()


def test_both_entry_points_have_a_row():
    assert set(NAMES) <= T.covered()
    _register()                                                    # a second registration adds nothing
    assert sorted(r["name"] for r in T.ROWS if set(r["covers"]) & set(NAMES)) == sorted(NAMES)


def test_the_rows_build_on_the_cpu_with_outputs_as_large_as_the_header_says():
    by_name = {r["name"]: r for r in T.ROWS}
    for shape in _shapes():
        m, k1, c = shape
        fwd = {name: x for name, _, x in by_name["tgn_cbl_stage_forward"]["build"](shape)}
        assert fwd["loss"] == ((1,), F32) and fwd["count"] == ((1,), I64) and fwd["pair_w"] == ((m, k1), F32)
        assert fwd["ws"] == ((T._L().tgn_cbl_stage_workspace_bytes(m),), torch.uint8)
        assert not fwd["f"].is_cuda and fwd["f"].dtype == F32 and fwd["idx"].dtype == I32 and fwd["labels"].dtype == I64
        bwd = {name: x for name, _, x in by_name["tgn_cbl_stage_backward"]["build"](shape)}
        assert bwd["grad_f"] == ((m, c), F32)
        assert tuple(bwd["rev_start"].shape) == (m + 1,) and tuple(bwd["rev_pair"].shape) == (m * k1,) and bwd["rev_pair"].dtype == I32
        assert m * k1 < 64 or (bwd["pair_w"] == 0).any()
