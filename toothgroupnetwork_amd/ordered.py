"""The atomic-free backward of the gather family: every raw-pointer call of csrc/scatter_ordered.hip.

A scatter-add ``out[idx[q]] += term(q)`` with float atomics gives other bits from launch to launch.  Turned round it does not:
``reverse_lists`` builds, per target row, the ascending list of the pair numbers that target it (tgn_reverse_lists), and ``scatter``
lets one lane group own a row and add that row's terms in list order (tgn_scatter_ordered; include/tgn_pointops.h states both
contracts).  The ``backward`` methods of pointops, pointnet2_utils and point_transformer call the two when
``config.cfg.ordered_backward`` is set (TGN_ORDERED_BACKWARD=1, ``tools/train.py --ordered_backward``); it is read at call time and
off by default.  No CPU path, no fallback.

The lists are memoised per index tensor -- the blocks of a Point-Transformer stage share one ``knn_indices`` tensor, and inside a
layer ``_QueryGroup`` and the attention tail share one too -- keyed like the kNN memo of pointops on the tensor's identity (held
weakly: the entry goes with the tensor), its version counter (an in-place write misses) and the current stream.  Writes that torch
cannot see (``.data``, raw pointers) do not bump the version: call ``lists_cache_clear()`` after them.  While a stream is being
captured the memo is neither read nor written: a graph must own every buffer it replays from, and rebuilds the lists when it is
replayed on new indices.
"""
import torch
from torch.utils.weak import WeakTensorKeyDictionary

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
    (q // pairs_per_batch) * n + idx.flatten()[q] == r.  An index outside [0, n) counts as row 0 of its batch, as in
    losses.reverse_lists; wrap=True first maps a negative index i to i + n.  No synchronisation."""
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


def softmax_aggregate_backward(x_v, p_r, sm, idx, grad_out):
    """The Point-Transformer tail's backward with its d_xv scatter left out of the kernel and summed along the lists instead, over
    the d_pr the kernel writes anyway -> (g_xv, g_pr, g_logit)."""
    n, nsample, c = p_r.shape
    g_pr = torch.empty_like(p_r)
    g_lg = torch.empty_like(sm)
    ops().tgn_pt_softmax_aggregate_backward(n, nsample, c, sm.shape[2], x_v, p_r, sm, idx, grad_out, None, g_pr, g_lg, stream())
    g_xv = scatter(g_pr.view(n * nsample, c), x_v.shape[0], reverse_lists(idx, x_v.shape[0]))
    return g_xv, g_pr, g_lg
