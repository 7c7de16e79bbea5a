"""GPU: every C-ABI entry point of include/tgn_pointops.h held to the memory it declares (tests/containment_cases.py).

The parity and bound tests compare what the kernels compute.  This one looks at what they touch.  Each case makes the same raw
library call three times on the same operand values:

  A  every operand a view into one arena filled with 0xA5 (tests/arena.py), 64 KiB of the fill around each: workspaces exactly as
     large as their size function says, outputs exactly as large as the header says;
  B  the same in a fresh arena filled with 0xFF (NaN as a float, -1 as an integer);
  C  ordinary separate torch allocations, every workspace twice the reported size.

Every run: status 0; after a synchronisation not one byte of a guard band or of an input differs from the arena's snapshot (an
overrun of an output or workspace lands in the band behind it); the stream's index-error word is 0 (a guard word read as an index
would go through the "bad index reads point 0" path and give a plausible result).  Then A against B and A against C, every output
byte for byte as uint8: a guard value that reached a result, an output element nobody wrote (it still holds the fill, and the two
fills differ) and a result that depends on the size of the workspace all show up as a difference.

Not covered, by construction: an over-read whose value never reaches a result, such as a vector load past the end of an operand
that is masked afterwards.  It is invisible to this method, and only a page boundary makes it matter.  Neither are operands at
4-byte-only alignment (the `offset` form of tests/test_gpu_operator_forms.py), bad arguments and NaN propagation.

The last test prints, per row, how many (shape, tuning) cases ran, and fails for a pre-filled output that no case of its row
changed: where an output starts as zeros in all three runs, a call that did nothing would otherwise pass.  Both read counters that
the cases fill as they run in this process: under -k, -x, --lf or with the cases spread over several processes the counts are partial
and that last check is silent for every row that did not run in full (it cannot fail wrongly, it only says less)."""
import collections

import pytest
import torch

import containment_cases as T
from arena import CANARY, CANARY_B, compare_outputs, run_guarded, run_plain

pytestmark = pytest.mark.gpu

CASES = [(r, si, ti) for r in T.ROWS for si in range(len(r["shapes"])) for ti in range(len(r["tunings"]))]
RAN = collections.Counter()
MOVED = {}      # (row, pre-filled output) -> some case changed it: a call that does nothing would pass every comparison there


def _id(case):
    r, si, ti = case
    shape = f"late{si}" if isinstance(r["shapes"], T._Late) else "-".join(str(x) for x in r["shapes"][si]).replace(" ", "")
    tune = ",".join(f"{k}={v}" for k, v in r["tunings"][ti].items())
    return f"{r['name']}-{shape}" + (f"-{tune}" if tune else "")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_entry_point_stays_inside_its_operands(dev, case):
    from toothgroupnetwork_amd import _lib
    r, si, ti = case
    shape, tune = r["shapes"][si], r["tunings"][ti]
    what = f"{r['name']} {shape} {tune}"
    L, st = _lib.lib(), _lib.stream()
    assert r["compare"] == "bytes", f"{what}: no row needs compare='bound' (tests/containment_cases.py says why), so this test compares bytes only"
    operands = r["build"](shape)
    for name, role, _ in operands:
        assert role != "ws" or name in r["sizes"], f"{what}: workspace {name} has no size function named in its row"

    raw = r["call"](shape)

    def call(views):
        return raw(L, views, st)

    def finish(status, views, run):
        assert status == 0, f"{what}, run {run}: status {status}: {L.tgn_last_error().decode('utf-8', 'replace')}"
        assert L.tgn_take_index_error(st) == 0, f"{what}, run {run}: the call latched the stream's index-error word on valid arguments"
        if r["after"]:
            r["after"](views, f"{what}, run {run}")

    with _lib.tuning(**tune):
        assert L.tgn_clear_index_error(st) == 0
        outs = {}
        for run, fill in (("A", CANARY), ("B", CANARY_B)):
            status, outs[run], views = run_guarded(operands, call, fill, dev, f"{what}, run {run}", sync=torch.cuda.synchronize)
            finish(status, views, run)
        status, outs["C"], views = run_plain(operands, call, dev, sync=torch.cuda.synchronize)
        finish(status, views, "C")
    compare_outputs(outs["A"], outs["B"], f"{what}: arena fill {CANARY:#x} against {CANARY_B:#x}")
    compare_outputs(outs["A"], outs["C"], f"{what}: arena against ordinary allocations with a doubled workspace")
    RAN[r["name"]] += 1
    for name, role, x in operands:
        if role == "out" and torch.is_tensor(x):
            before = x.contiguous().view(-1).view(torch.uint8).to(dev)
            MOVED[(r["name"], name)] = MOVED.get((r["name"], name), False) or not torch.equal(before, outs["A"][name])


def test_zz_every_row_ran(capsys):
    """prints the number of (shape, tuning) cases that ran per row; when the whole module ran, every row ran all of its cases"""
    with capsys.disabled():
        print("\ncontainment cases per row:")
        for r in T.ROWS:
            print(f"  {r['name']:52s} {RAN[r['name']]:4d} of {len(r['shapes']) * len(r['tunings'])}")
        print(f"  {'total':52s} {sum(RAN.values()):4d} of {len(CASES)}")
    full = {r["name"] for r in T.ROWS if RAN[r["name"]] == len(r["shapes"]) * len(r["tunings"])}
    idle = sorted(k for k, moved in MOVED.items() if not moved and k[0] in full)
    assert not idle, f"pre-filled outputs that no case of their row changed (the call writes nothing there?): {idle}"
