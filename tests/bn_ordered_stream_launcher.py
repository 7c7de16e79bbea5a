#!/usr/bin/env python3
"""Child process of tests/test_gpu_bn_ordered.py ("contention") and tests/test_gpu_bn_ordered_graph.py ("graph"): the two checks of
the ordered BatchNorm that need a second stream.

It runs in a process of its own for the reason tests/cluster_stream_launcher.py gives: a stream, once created, stays with the process,
and an extra stream in the test process changes which hardware queues the streams of later tests share.

contention  point_transformer.bn_rows forward + backward under config.cfg.ordered_bn at (1000, 35) and (8197, 4), once on an idle
            device, then 20 times while a second stream keeps running grouping launches of this library (pointops.grouping over a
            24 000-row table, re-issued in front of every repetition and never waited for).  Every repetition's y, dx, dgamma, dbeta,
            save_mean, save_invstd and running statistics are byte-equal to the idle run's.
graph       the same forward + backward at (8197, 4) captured on a side stream and replayed three times, the running statistics put
            back and the outputs zeroed in front of each: every replay equals the eager bits; the capture allocates its own
            workspace (the module's is neither read nor grown).

Prints "bn ordered <mode> ok" and exits 0 when every comparison holds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import torch  # noqa: E402

from toothgroupnetwork_amd import config, point_transformer as PT, pointops  # noqa: E402

DEV = torch.device("cuda", 0)


def _case(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * 2.0 + 3.0).to(DEV)
    return x, torch.randn(rows, C, generator=g).to(DEV)


def _module(C):
    bn = torch.nn.BatchNorm1d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C))
        bn.bias.copy_(torch.linspace(-1.0, 1.0, C))
    return bn


def _step(bn, x, dy):
    """-> everything one forward + backward writes, as copies that hold no autograd graph.  (A graph kept alive keeps the
    AccumulateGrad nodes of bn.weight and bn.bias alive, with the stream they were made on; a later backward on another stream is then
    synchronised with that one, which a capture does not survive when it is the default stream.)"""
    xg = x.detach().requires_grad_(True)
    y = PT.bn_rows(bn, xg, relu=True)
    stats = [t.clone() for t in y.grad_fn.saved_tensors[3:5]]
    dx, dgamma, dbeta = torch.autograd.grad(y, [xg, bn.weight, bn.bias], dy)
    return [t.detach().clone() for t in (y, dx, dgamma, dbeta, *stats, bn.running_mean, bn.running_var, bn.num_batches_tracked)]


def _same(a, b):
    return all(torch.equal(p.reshape(-1).view(torch.uint8), q.reshape(-1).view(torch.uint8)) for p, q in zip(a, b))


def contention():
    side = torch.cuda.Stream()
    g = torch.Generator().manual_seed(5)
    table = torch.randn(24000, 64, generator=g).to(DEV)
    idx = torch.randint(0, 24000, (24000, 36), generator=g).to(torch.int32).to(DEV)
    for rows, C in ((1000, 35), (8197, 4)):
        x, dy = _case(rows, C, rows)
        with config.override(ordered_bn=True):
            idle = _step(_module(C), x, dy)
            torch.cuda.synchronize()
            for rep in range(20):
                with torch.cuda.stream(side):
                    for _ in range(4):
                        pointops.grouping(table, idx)
                got = _step(_module(C), x, dy)
                if not _same(got, idle):
                    print(f"bn ordered contention mismatch: ({rows}, {C}) repetition {rep}")
                    return 1
        torch.cuda.synchronize()
    print("bn ordered contention ok")
    return 0


def graph():
    rows, C = 8197, 4
    x, dy = _case(rows, C, 7)
    with config.override(ordered_bn=True):
        bn = _module(C)
        eager = _step(bn, x, dy)
        with torch.no_grad():       # back to where the eager step started: every replay then repeats exactly that step
            start = [bn.running_mean.clone().fill_(0.0), bn.running_var.clone().fill_(1.0), bn.num_batches_tracked.clone().fill_(0)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _step(bn, x, dy)                              # allocator warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        parked = {k: (v.data_ptr(), v.numel()) for k, v in bn.__dict__["_tgn_bn_ws_ordered"].items()}
        cuda_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cuda_graph, stream=side):
            captured = _step(bn, x, dy)
        if {k: (v.data_ptr(), v.numel()) for k, v in bn.__dict__["_tgn_bn_ws_ordered"].items()} != parked:
            print("bn ordered graph: the capture touched the module's parked workspace")
            return 1
    for replay in range(3):
        with torch.no_grad():
            for t, s in zip((bn.running_mean, bn.running_var, bn.num_batches_tracked), start):
                t.copy_(s)
        for t in captured[:6]:
            t.zero_()
        cuda_graph.replay()
        torch.cuda.synchronize()
        now = captured[:6] + [bn.running_mean, bn.running_var, bn.num_batches_tracked]
        if not _same(now, eager):
            print(f"bn ordered graph mismatch: replay {replay}")
            return 1
    print("bn ordered graph ok")
    return 0


if __name__ == "__main__":
    sys.exit({"contention": contention, "graph": graph}[sys.argv[1]]())
