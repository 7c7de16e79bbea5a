"""The containment rows of tgn_reverse_lists and tgn_scatter_ordered (csrc/scatter_ordered.hip), added to the table of
tests/containment_cases.py through its row(...) function when this module is imported -- once: a second import finds the names
covered and adds nothing.

pytest collects tests/ in name order and this file's name sorts before tests/test_containment_host.py and
tests/test_gpu_containment.py, so in a run over tests/ the completeness and hygiene tests of the first see the two rows and the
parametrised GPU test of the second runs them like every other row: three runs per shape on guarded operands, bytes compared.

Limit, as for tests/test_cbl_containment_rows.py: either of those two files run ALONE does not import this one, reports the two entry
points as missing and runs no case of theirs.  The suite commands over tests/ are the check.

Operands.  Indices are valid; the workspace is exactly tgn_reverse_lists_workspace_bytes and starts as the arena's fill (the header:
any contents); every output is an `O` operand, so an element the call did not write shows as a difference between the two fills --
rows that nothing targets and rows without pairs included.  The scatter's values are multiples of 1/16, its lists those of
tests/ordered_ref.py built on the CPU.  Neither call has a float atomic: bytes are compared.

Shapes of the lists (b, n, pairs per batch, int64, kind): the smallest; a square list; fine rows onto coarse rows; a hub longer than
the workgroup sort's LDS tile; a dense batch with int64 indices; one past a scan tile of rows and one past a workgroup of pairs; no
pairs at all.  Shapes of the scatter (rows, queries, k, c, g, form): every channel-lane width (c = 1, 3, 35, 64, 130: 1, 4, 64, 64 and
three passes of 64 lanes), the three forms, a hub, segment lengths that are no multiple of the four pairs in flight."""
import numpy as np
import torch

import containment_cases as T
import ordered_ref as R
from operator_forms import gen_for, q16

F32, I32, I64 = torch.float32, torch.int32, torch.int64
NAMES = ("tgn_reverse_lists", "tgn_scatter_ordered")
SCAN_TILE, BLOCK, LONG_TILE = 1024, 256, 1024      # kRevScanTile, kRevBlock, kRevLongTile of csrc/scatter_ordered.hip

LIST_SHAPES = [(1, 1, 1, False, "random"), (1, 65, 65 * 16, False, "random"), (1, 40, 300 * 3, False, "random"),
               (1, 300, LONG_TILE + 77, False, "hub"), (3, 50, 37 * 8, True, "random"), (2, SCAN_TILE + 1, BLOCK + 1, False, "random"),
               (2, 9, 0, False, "random")]
SCATTER_SHAPES = [(1, 1, 1, 1, 1, "pairs"), (33, 70, 3, 3, 1, "pairs"), (65, 65, 16, 35, 1, "pairs"), (40, 300, 3, 64, 1, "query"),
                  (40, 90, 5, 130, 1, "query"), (50, 61, 6, 64, 4, "query"), (61, 61, 7, 35, 1, "identity"), (30, 300, 5, 4, 1, "hub"),
                  (33, 70, 3, 130, 1, "minus")]


def _list_idx(shape):
    b, n, pairs, i64, kind = shape
    g = gen_for(f"reverse_lists{n}")
    idx = torch.full((b, pairs), n // 2, dtype=torch.int64) if kind == "hub" else torch.randint(0, n, (b, pairs), generator=g)
    return idx.to(I64 if i64 else I32)


def _lists_build(shape):
    b, n, pairs, i64, kind = shape
    return [T.I("idx", _list_idx(shape)), T.O("rev_start", (b * n + 1,), I32), T.O("rev_pair", (b * pairs,), I32),
            T.W("ws", T._L().tgn_reverse_lists_workspace_bytes(b, n, pairs))]


def _scatter_build(shape):
    rows, m, k, c, g_, form = shape
    g = gen_for(f"scatter_ordered{rows}{c}")
    pairs = rows * k if form == "identity" else m * k
    ops = []
    if form != "identity":
        idx = torch.randint(0, rows, (m, k), generator=g)
        if form == "hub":
            idx[:, 0] = rows - 1
        rev_start, rev_pair = R.reverse_lists(idx.numpy(), rows)
        ops += [T.I("rev_start", torch.from_numpy(rev_start)), T.I("rev_pair", torch.from_numpy(rev_pair))]
    if form == "query":
        ops += [T.I("src", q16(g, m, c)), T.I("coef", q16(g, pairs, g_))]
    else:
        ops += [T.I("src", q16(g, pairs, c))]
    return ops + [T.O("out", (rows, c))]


def _register():
    if set(NAMES) & T.covered():
        return
    P = T.P
    T.row("tgn_reverse_lists", ["tgn_reverse_lists"], LIST_SHAPES, _lists_build,
          lambda s: lambda L, v, st: L.tgn_reverse_lists(s[0], s[1], s[2], P(v["idx"]), int(s[3]), P(v["rev_start"]), P(v["rev_pair"]), P(v["ws"]),
                                                         v["ws"].numel(), st),
          sizes={"ws": "tgn_reverse_lists_workspace_bytes"}, compare="bytes")
    T.row("tgn_scatter_ordered", ["tgn_scatter_ordered"], SCATTER_SHAPES, _scatter_build,
          lambda s: lambda L, v, st: L.tgn_scatter_ordered(s[0], s[3], s[2], s[4], P(v.get("rev_start")), P(v.get("rev_pair")), P(v["src"]),
                                                           P(v.get("coef")), -1.0 if s[5] == "minus" else 1.0, P(v["out"]), st),
          compare="bytes")


_register()


def test_both_entry_points_have_a_row():
    assert set(NAMES) <= T.covered()
    _register()                                                    # a second registration adds nothing
    assert sorted(r["name"] for r in T.ROWS if set(r["covers"]) & set(NAMES)) == sorted(NAMES)
    assert all(r["compare"] == "bytes" for r in T.ROWS if r["name"] in NAMES)


def test_the_rows_build_on_the_cpu_with_outputs_as_large_as_the_header_says():
    by_name = {r["name"]: r for r in T.ROWS}
    for shape in LIST_SHAPES:
        b, n, pairs, i64, kind = shape
        ops = {name: x for name, _, x in by_name["tgn_reverse_lists"]["build"](shape)}
        assert ops["rev_start"] == ((b * n + 1,), I32) and ops["rev_pair"] == ((b * pairs,), I32)
        assert ops["ws"] == ((T._L().tgn_reverse_lists_workspace_bytes(b, n, pairs),), torch.uint8) and (ops["ws"][0][0] > 0 or not b * n)
        assert not ops["idx"].is_cuda and ops["idx"].dtype == (I64 if i64 else I32) and tuple(ops["idx"].shape) == (b, pairs)
    assert any(s[2] > LONG_TILE and s[4] == "hub" for s in LIST_SHAPES) and any(s[1] > SCAN_TILE for s in LIST_SHAPES)
    for shape in SCATTER_SHAPES:
        rows, m, k, c, g_, form = shape
        ops = {name: x for name, _, x in by_name["tgn_scatter_ordered"]["build"](shape)}
        assert ops["out"] == ((rows, c), F32)
        assert ("coef" in ops) == (form == "query") and ("rev_start" in ops) == (form != "identity")
        if form != "identity":
            assert tuple(ops["rev_start"].shape) == (rows + 1,) and tuple(ops["rev_pair"].shape) == (m * k,) and ops["rev_pair"].dtype == I32
            assert int(ops["rev_start"][-1]) == m * k
        if form == "hub":
            assert int((ops["rev_start"][1:] - ops["rev_start"][:-1]).max()) >= m
        else:
            lengths = np.diff(R.identity_lists(rows, k)[0] if form == "identity" else ops["rev_start"].numpy())
            assert rows == 1 or (lengths % 4 != 0).any()      # the tail loop behind the four pairs in flight runs
