"""GPU: a composition of switched operators under config.cfg.ordered_backward replays as a graph to the eager bits.

queryandgroup (pointops._QueryGroup) -> slices -> point_transformer.pt_softmax_aggregate with a fixed cotangent, at n = 200,
nsample = 16, c = 32, g = 4: the gradients of p (through the grouped coordinates, as centre and as neighbour), x_k and x_v all flow
through the one neighbour list.  Forward and backward are captured in a torch.cuda.graph and replayed twice; p.grad, x_k.grad and
x_v.grad come out the same bits each time, and the same bits as the eager run.  With float atomics (the switch off) only a bound
could be asked.  While a stream is capturing, ordered.reverse_lists bypasses its memo, so the graph owns the lists it replays from.

Constraint, as for tests/test_gpu_losses_cbl_fused_graph.py: this test opens a stream to capture on and must be collected AFTER
tests/test_gpu_hotpath_configs.py.  Hence a file of its own whose name sorts behind it."""
import pytest
import torch

from operator_forms import gen_for

pytestmark = pytest.mark.gpu

N, NSAMPLE, C, G = 200, 16, 32, 4


def _step(p, x_k, x_v, idx, o, go):
    from toothgroupnetwork_amd import point_transformer as PT, pointops as P
    grouped = P.queryandgroup(NSAMPLE, p, p, x_k, idx, o, o, use_xyz=True)               # (n, nsample, 3 + c)
    rel, x_kg = grouped[:, :, :3], grouped[:, :, 3:]
    p_r = x_kg * 0.5 + rel.sum(2, keepdim=True)                                          # (n, nsample, c)
    logit = x_kg[:, :, :G] - rel[:, :, :1]                                               # (n, nsample, g)
    out = PT.pt_softmax_aggregate(x_v, p_r, logit, idx)
    return tuple(torch.autograd.grad(out, [p, x_k, x_v], go))


def test_forward_and_backward_replay_as_a_graph_to_the_eager_bits(dev):
    from toothgroupnetwork_amd import config, ordered, pointops as P
    g = gen_for("ordered_graph")
    p = torch.rand(N, 3, generator=g).to(dev).requires_grad_()
    x_k, x_v = (torch.randn(N, C, generator=g).to(dev).requires_grad_() for _ in range(2))
    go = torch.randn(N, C, generator=g).to(dev)
    o = P.register_offsets(torch.tensor([N], dtype=torch.int32, device=dev), [N])
    idx = P.knn_indices(NSAMPLE, p.detach(), None, o, o)
    with config.override(ordered_backward=True):
        eager = [t.clone() for t in _step(p, x_k, x_v, idx, o, go)]
        again = _step(p, x_k, x_v, idx, o, go)
        for a, b, what in zip(eager, again, ("p.grad", "x_k.grad", "x_v.grad")):
            assert bool(a.any()) and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: two eager runs"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _step(p, x_k, x_v, idx, o, go)               # allocator warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        builds = ordered.lists_cache_stats()["builds"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = _step(p, x_k, x_v, idx, o, go)
        assert ordered.lists_cache_stats()["builds"] > builds, "the capture must build its own lists, not read the memo's"
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(captured, eager, ("p.grad", "x_k.grad", "x_v.grad")):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{what}: replay against eager"
