"""The backward of the gather family, both forms: every gradient that flows through a neighbour list is stated here, once.

A scatter-add ``out[idx[q]] += term(q)`` with float atomics gives other bits from launch to launch.  Turned round it does not:
``reverse_lists`` builds, per target row, the ascending list of the pair numbers that target it (tgn_reverse_lists), and ``scatter``
lets one lane group own a row and add that row's terms in list order (tgn_scatter_ordered; include/tgn_pointops.h states both
contracts, csrc/scatter_ordered.hip holds the kernels).  The ``*_backward`` functions at the end of this module each state one
gradient in its atomic form (a zero-filled accumulator and the operator's own backward kernel) and in its ordered form (the two
calls above) and choose by ``config.cfg.ordered_backward`` (TGN_ORDERED_BACKWARD=1, ``tools/train.py --ordered_backward``; off by
default), which is read here and nowhere else, at call time.  The ``backward`` methods of pointops, pointnet2_utils and
point_transformer call them; the fused contrastive-boundary stage (losses.py) takes its lists from ``reverse_lists`` too.  No CPU
path, no fallback.

The lists are memoised per index tensor -- the blocks of a Point-Transformer stage share one ``knn_indices`` tensor, and inside a
layer ``_QueryGroup`` and the attention tail share one too -- keyed like the kNN memo of pointops on the tensor's identity (held
weakly: the entry goes with the tensor), its version counter (an in-place write misses) and the current stream.  Writes that torch
cannot see (``.data``, raw pointers) do not bump the version: call ``lists_cache_clear()`` after them.  While a stream is being
captured the memo is neither read nor written: a graph must own every buffer it replays from, and rebuilds the lists when it is
replayed on new indices.

The other reduction of a training step with an arrival order is stated here too, in both forms: the per-column sums of the fused
BatchNorm over rows (``bn_rows_forward`` / ``bn_rows_backward``, csrc/bnorm.hip; ``point_transformer._BNRows`` calls them), with
float64 atomics or, with ``config.cfg.ordered_bn`` (TGN_ORDERED_BN=1; off by default, a switch of its own), thread by thread and block
by block in the order include/tgn_pointops.h states.  ``tr_set["reproducible"]`` (training.py, ``tools/train.py --reproducible``)
sets both switches.
"""
import torch
from torch.utils.weak import WeakTensorKeyDictionary

from . import config
from ._lib import ops, require_cuda, stream

_LISTS = WeakTensorKeyDictionary()     # idx tensor -> {(n, batch, wrap, stream): (version, rev_start, rev_pair)}
_stats = {"hits": 0, "builds": 0}


def lists_cache_clear():
    _LISTS.clear()


def lists_cache_stats():
    """{"hits": memo hits, "builds": tgn_reverse_lists calls} since the process started."""
    return dict(_stats)


def _build(idx, n, batch, wrap):
    if wrap:        # the dense gathers wrap a negative index like torch's advanced indexing (pointnet2_utils.py:56-60)
        idx = torch.where(idx < 0, idx + n, idx)
    pairs = idx.numel() // batch if batch else 0
    rev_start = torch.empty(batch * n + 1, dtype=torch.int32, device=idx.device)
    rev_pair = torch.empty(batch * pairs, dtype=torch.int32, device=idx.device)
    nbytes = int(ops().tgn_reverse_lists_workspace_bytes(batch, n, pairs))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=idx.device) if nbytes else None
    ops().tgn_reverse_lists(batch, n, pairs, idx, int(idx.dtype == torch.int64), rev_start, rev_pair, ws, nbytes, stream())
    _stats["builds"] += 1
    return rev_start, rev_pair


def reverse_lists(idx, n, batch=1, wrap=False):
    """idx: `batch` equal runs of indices into [0, n) (any shape; int32 or int64, contiguous) -> (rev_start (batch * n + 1,),
    rev_pair (idx.numel(),)) int32: rev_pair[rev_start[r] : rev_start[r + 1]] holds, ascending, the pair numbers q with
    (q // pairs_per_batch) * n + idx.flatten()[q] == r.  An index outside [0, n) counts as row 0 of its batch;
    wrap=True first maps a negative index i to i + n.  No synchronisation."""
    require_cuda(idx)
    if idx.dtype not in (torch.int32, torch.int64) or not idx.is_contiguous():
        raise ValueError(f"idx must be int32 or int64 and contiguous here, got {idx.dtype} with strides {tuple(idx.stride())}")
    n, batch = int(n), int(batch)
    if batch < 0 or n < 0 or (batch and idx.numel() % batch) or (idx.numel() and not batch * n):
        raise ValueError(f"idx of {idx.numel()} entries does not split into {batch} runs over {n} rows")
    if torch.cuda.is_current_stream_capturing():
        return _build(idx, n, batch, wrap)
    try:
        version = idx._version
    except RuntimeError:        # an inference tensor carries no version counter: no memo for it
        return _build(idx, n, batch, wrap)
    key = (n, batch, bool(wrap), torch.cuda.current_stream().cuda_stream)
    book = _LISTS.get(idx)
    if book is None:
        book = _LISTS[idx] = {}
    hit = book.get(key)
    if hit is not None and hit[0] == version:
        _stats["hits"] += 1
        return hit[1], hit[2]
    rev_start, rev_pair = _build(idx, n, batch, wrap)
    book[key] = (version, rev_start, rev_pair)
    return rev_start, rev_pair


def scatter(src, n_rows, lists=None, coef=None, k=1, sign=1.0):
    """The ordered sum of tgn_scatter_ordered -> (n_rows, c) float32, every element written.

    src (..., c) float32 contiguous: one row per pair, or with `coef` (pairs, g) one row per QUERY (pair q reads row q // k and is
    weighted by coef[q, ch % g]).  lists = (rev_start, rev_pair) of reverse_lists; None: the identity segments, row r owns the pairs
    r * k .. r * k + k - 1.  sign +1 or -1."""
    require_cuda(src, coef)
    if src.dtype != torch.float32 or not src.is_contiguous() or (coef is not None and (coef.dtype != torch.float32 or not coef.is_contiguous())):
        raise ValueError("src and coef must be float32 and contiguous here")
    c = src.shape[-1]
    rows_src = src.numel() // c if c else 0
    k, n_rows = int(k), int(n_rows)
    g = 1
    if coef is not None:
        g = coef.shape[-1]
        pairs = coef.numel() // g if g else 0
        if not g or c % g or pairs != rows_src * k:
            raise ValueError(f"coef {tuple(coef.shape)} does not weight {rows_src} source rows of {c} channels with k = {k}")
    else:
        pairs = rows_src
    if lists is None:
        rev_start = rev_pair = None
        if n_rows * k != pairs:
            raise ValueError(f"identity segments: {n_rows} rows of k = {k} pairs are not the {pairs} pairs given")
    else:
        rev_start, rev_pair = lists
        if rev_start.numel() != n_rows + 1 or rev_pair.numel() != pairs or rev_start.dtype != torch.int32 or rev_pair.dtype != torch.int32:
            raise ValueError(f"lists of {rev_start.numel() - 1} rows and {rev_pair.numel()} pairs (int32) do not fit {n_rows} rows and {pairs} pairs")
    out = torch.empty(n_rows, c, dtype=torch.float32, device=src.device)
    ops().tgn_scatter_ordered(n_rows, c, k, g, rev_start, rev_pair, src, coef, float(sign), out, stream())
    return out


# ---- the gradients, each in both forms ---------------------------------------------------------------------------------------------
def gather_lists(idx, n, dense=None):
    """What gather_backward sums along, for a backward that calls it twice on one idx (None in the atomic form, which needs none)."""
    if config.cfg.ordered_backward:
        return reverse_lists(idx, n) if dense is None else reverse_lists(idx, n, dense[0], wrap=True)


def gather_backward(src, idx, n, dense=None, lists=None):
    """The gradient of the plain gather out[q] = x[idx[q]] from src (..., c) float32 contiguous, one row per index.
    Packed (dense None): idx (m, nsample) int32 onto n rows -> (n, c).  Dense = (batch, indices per cloud): `batch` clouds (0 too) of
    n rows, idx int32 or int64 with a cloud's own row numbers, negative ones wrapping as in the forward -> (batch, n, c)."""
    c = src.shape[-1]
    if config.cfg.ordered_backward:
        grad = scatter(src.flatten(0, -2), n if dense is None else dense[0] * n, lists or gather_lists(idx, n, dense))
        return grad if dense is None else grad.view(dense[0], n, c)
    if dense is None:
        grad = torch.zeros(n, c, dtype=torch.float32, device=src.device)
        ops().tgn_grouping_backward(idx.shape[0], idx.shape[1], c, src, idx, grad, stream())
    else:
        grad = torch.zeros(dense[0], n, c, dtype=torch.float32, device=src.device)
        ops().tgn_scatter_add_points(dense[0], n, dense[1], c, src, idx, int(idx.dtype == torch.int64), grad, stream())
    return grad


def weighted_gather_backward(src, idx, weight, n, batch=None):
    """The gradient of the weighted gather out[q] = sum_j f[idx[q, j]] * weight[q, j] onto f, from src (..., c), one row per query.
    Packed (batch None): idx (queries, k) int32 onto n rows -> (n, c).  Dense: idx (batch, queries, k) int32 or int64 with a cloud's
    own row numbers -> (batch, n, c); the atomic kernel reads them as global int32 rows of the flattened (batch * n, c) features."""
    c, k, b = src.shape[-1], idx.shape[-1], 1 if batch is None else batch        # (an empty batch, 0, is still the dense form)
    if config.cfg.ordered_backward:
        grad = scatter(src.flatten(0, -2), b * n, reverse_lists(idx, n, b), coef=weight.view(-1, 1), k=k)
    else:
        if batch is not None:
            idx = (idx + (torch.arange(batch, device=idx.device, dtype=idx.dtype) * n).view(batch, 1, 1)).to(torch.int32).contiguous()
        grad = torch.zeros(b * n, c, dtype=torch.float32, device=src.device)
        ops().tgn_interpolation_backward(idx.shape[:-1].numel(), c, k, src, idx, weight, grad, stream())
    return grad if batch is None else grad.view(batch, n, c)


def subtraction_backward(src, idx, n2):
    """Both gradients of out[i, j] = a[i] - b[idx[i, j]] from src (n, nsample, c) -> (g_a (n, c), g_b (n2, c)): one atomic launch, or
    the identity segments for a and the signed sum along the lists for b."""
    n, nsample, c = src.shape
    if config.cfg.ordered_backward:
        pair_rows = src.view(n * nsample, c)
        return scatter(pair_rows, n, None, k=nsample), scatter(pair_rows, n2, reverse_lists(idx, n2), sign=-1.0)
    g_a, g_b = src.new_zeros(n, c), src.new_zeros(n2, c)
    ops().tgn_subtraction_backward(n, nsample, c, idx, src, g_a, g_b, stream())
    return g_a, g_b


def centres_backward(g_rel):
    """The gradient of the centres of pointops._QueryGroup, out[i, j] = xyz[idx[i, j]] - new_xyz[i], from g_rel (m, nsample, 3)
    -> (m, 3): torch's sum beside the atomic kernels, the identity segments with sign -1 in the ordered form."""
    if config.cfg.ordered_backward:
        m, nsample, c = g_rel.shape
        return scatter(g_rel.view(m * nsample, c), m, None, k=nsample, sign=-1.0)
    return -g_rel.sum(1)


def softmax_aggregate_backward(x_v, p_r, sm, idx, grad_out):
    """The Point-Transformer tail's backward -> (g_xv, g_pr, g_logit): the kernel with its atomic d_xv scatter into a zero-filled
    g_xv, or the kernel with that scatter left out and d_xv summed along the lists instead, over the d_pr the kernel writes anyway."""
    n, nsample, c = p_r.shape
    on = config.cfg.ordered_backward
    g_xv = None if on else torch.zeros_like(x_v)
    g_pr = torch.empty_like(p_r)
    g_lg = torch.empty_like(sm)
    ops().tgn_pt_softmax_aggregate_backward(n, nsample, c, sm.shape[2], x_v, p_r, sm, idx, grad_out, g_xv, g_pr, g_lg, stream())
    if on:
        g_xv = scatter(g_pr.view(n * nsample, c), x_v.shape[0], reverse_lists(idx, x_v.shape[0]))
    return g_xv, g_pr, g_lg


# ---- BatchNorm over rows, both forms (csrc/bnorm.hip) ---------------------------------------------------------------------------------
def _bn_workspace(bn, rows, C, device, on):
    """A module's workspace for the current (device, stream), parked on the module (DataParallel replicas share its __dict__ entries,
    two streams must never meet in one buffer).  Atomic form: accumulators + ticket, zero-filled once and left zeroed by the kernels.
    Ordered form: the blocks' partial sums, any contents, grown to the largest `rows` seen; while a stream is being captured a
    buffer of the capture's own, as for the lists above."""
    zeroed = bn.__dict__.setdefault("_tgn_bn_ws", {})
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    if not on:
        ws = zeroed.get(key)
        if ws is None:
            ws = zeroed[key] = torch.zeros(int(ops().tgn_bn_rows_workspace_bytes(C)), dtype=torch.uint8, device=device)
        return ws
    nbytes = int(ops().tgn_bn_rows_ordered_workspace_bytes(rows, C))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    partials = bn.__dict__.setdefault("_tgn_bn_ws_ordered", {})
    ws = partials.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = partials[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def bn_rows_forward(bn, x, weight, bias, relu):
    """Training-mode BatchNorm1d [+ ReLU] of module `bn` over the rows of x (rows, C) float32 contiguous -> (y, save_mean, save_invstd,
    ws); the running statistics and num_batches_tracked are updated by the kernel.  The statistics are summed with float64 atomics, or,
    with config.cfg.ordered_bn, in the fixed order include/tgn_pointops.h states.  ws is what bn_rows_backward takes: the zeroed
    workspace of the atomic form, None for the ordered one -- the backward follows the form its forward took."""
    rows, C = x.shape
    on = config.cfg.ordered_bn
    y = torch.empty_like(x)
    stat = torch.empty(2, C, dtype=torch.float32, device=x.device)             # batch mean, 1 / sqrt(var + eps)
    mean, invstd = stat[0], stat[1]
    ws = _bn_workspace(bn, rows, C, x.device, on)
    track = bn.track_running_stats and bn.running_mean is not None
    head = (rows, C, x, weight, bias, float(bn.eps), float(bn.momentum), bn.running_mean if track else None,
            bn.running_var if track else None, bn.num_batches_tracked if track else None, int(relu), y, mean, invstd, ws)
    if on:
        ops().tgn_bn_rows_forward_ordered(*head, ws.numel(), stream())
    else:
        ops().tgn_bn_rows_forward(*head, stream())
    return y, mean, invstd, None if on else ws


def bn_rows_backward(bn, ws, x, y, dy, weight, mean, invstd, relu):
    """-> (dx, dgamma, dbeta) of bn_rows_forward from dy (rows, C) float32 contiguous; y is read under ReLU only (the mask is y > 0).
    ws None: dbeta and dgamma summed in the fixed order, else with float64 atomics into that workspace."""
    rows, C = x.shape
    dx = torch.empty_like(x)
    dwb = torch.empty(2, C, dtype=torch.float32, device=x.device)
    dgamma, dbeta = dwb[0], dwb[1]
    head = (rows, C, x, y, dy, weight, mean, invstd, int(relu), dx, dgamma, dbeta)
    if ws is None:
        ws = _bn_workspace(bn, rows, C, x.device, True)
        ops().tgn_bn_rows_backward_ordered(*head, ws, ws.numel(), stream())
    else:
        ops().tgn_bn_rows_backward(*head, ws, stream())
    return dx, dgamma, dbeta
