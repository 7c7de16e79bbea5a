"""GPU: forward and backward of losses.contrast_boundary_loss(fused=True) replay as a graph, as tests/test_gpu_losses_cbl_graph.py does it
for the unfused criterion -- and to the eager BITS, gradients included: the fused backward (csrc/cbl.hip) has no float atomic, where the
unfused one can only be held to a bound.  The rest of the fused stage's GPU tests is tests/test_gpu_losses_cbl_fused.py.

Constraint: this test opens a stream to capture on, and must be collected AFTER tests/test_gpu_hotpath_configs.py, whose
test_phased_plan_is_measured_and_sane_on_other_shapes[half] fails when a further stream has been used before the hot path's own
(DESIGN.md section 9).  Hence a file of its own, behind tests/test_gpu_losses.py, whose graph test opens a stream in the same way."""
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import cbl_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu


def _step(points, f, target, case):
    from toothgroupnetwork_amd import losses
    loss, counts = losses.contrast_boundary_loss(points, f, target, case["nsample"], case["stride"], fused=True)
    grads = torch.autograd.grad(loss.sum(), f)
    return (loss.detach(), counts) + grads


def test_forward_and_backward_replay_as_a_graph_to_the_eager_bits(dev):
    from toothgroupnetwork_amd import pointops
    case = CC.build("binary2")
    p = [torch.from_numpy(x).to(dev) for x in case["p"]]
    o = [pointops.register_offsets(torch.from_numpy(x).to(dev), x.tolist()) for x in case["o"]]
    f = [torch.from_numpy(x).to(dev).requires_grad_() for x in case["f"]]
    target = torch.from_numpy(case["target"]).to(dev)
    points = [[a, b] for a, b in zip(p, o)]
    eager = [t.clone() for t in _step(points, f, target, case)]
    assert bool((eager[1] > 0).all()) and all(bool(g.any()) for g in eager[2:])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(points, f, target, case)               # allocator and neighbour-list warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _step(points, f, target, case)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for i, (got, want) in enumerate(zip(captured, eager)):
            assert torch.equal(got, want), ("loss", "counts", "gradient 0", "gradient 1", "gradient 2")[i]
