"""GPU: point_transformer.bn_rows under config.cfg.ordered_bn replays as a graph to the eager bits.

Forward and backward at (8197, 4) -- five blocks, the four-in-flight loop and its tail -- are captured on one side stream in a
torch.cuda.graph and replayed three times; y, dx, dgamma, dbeta, the saved statistics and the running statistics come out the same
bits each time, and the same bits as the eager run.  The ordered calls make no host synchronisation and take no ticket, so there is
nothing a replay could find in another state; while a stream is capturing, ordered.py hands the calls a workspace of the capture's
own instead of the module's parked one, so the graph owns every buffer it replays from.  Modelled on
tests/test_gpu_ordered_backward_graph.py.

The capture runs in a child process (tests/bn_ordered_stream_launcher.py): this file sorts in front of
tests/test_gpu_hotpath_configs.py, whose timing check depends on the streams the test process has created before it (DESIGN.md
section 9)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_forward_and_backward_replay_as_a_graph_to_the_eager_bits():
    r = subprocess.run([sys.executable, os.path.join(HERE, "bn_ordered_stream_launcher.py"), "graph"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bn ordered graph ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
