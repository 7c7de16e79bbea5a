"""The contract of csrc/scatter_ordered.hip in numpy (include/tgn_pointops.h: tgn_reverse_lists, tgn_scatter_ordered).

reverse_lists: a stable argsort of the target rows, for `batch` runs over n rows each.
reverse_lists_torch: the same contract for one square list (m, k1) onto its own m rows as plain torch, on whatever device the tensor
is on: the lists the fused contrastive-boundary stage saves for its backward (ordered.reverse_lists(idx, m)), stated without the
kernel -- what tgn_reverse_lists is compared with on the device (tests/test_gpu_ordered_backward.py) and timed against
(tools/ordered_backward_bench.py).
scatter: out[r, ch] is the float32 sum, from +0.0f, taken SEQUENTIALLY in list order over the pairs of row r of term(q, ch), every
term rounded to float32 before it is added.  numpy's float32 arithmetic rounds every operation, so the loop below -- one add per
list position, all rows that are that long at once -- is that sum bit for bit.
"""
import numpy as np
import torch

F32 = np.float32


def reverse_lists(idx, n, batch=1):
    """idx: `batch` equal runs of integers (any shape) -> rev_start (batch * n + 1,), rev_pair (idx.size,), int32.  An index outside
    [0, n) counts as row 0 of its batch."""
    flat = np.asarray(idx).astype(np.int64).reshape(batch, -1)
    flat = np.where((flat < 0) | (flat >= n), 0, flat)
    keys = (flat + np.arange(batch, dtype=np.int64)[:, None] * n).reshape(-1)
    order = np.argsort(keys, kind="stable")
    rev_start = np.searchsorted(keys[order], np.arange(batch * n + 1), side="left")
    return rev_start.astype(np.int32), order.astype(np.int32)


def reverse_lists_torch(idx):
    """The lists the fused backward gathers along: idx (m, k1) integer neighbour lists -> (rev_start (m + 1,), rev_pair (m * k1,)),
    int32, where rev_pair[rev_start[i] : rev_start[i + 1]] holds the pair numbers q = i' * k1 + j with idx[i', j] == i in ascending
    order.  An index outside [0, m) counts as 0, the point the kernels read for it.  Plain torch on the tensor's device, CPU included:
    a STABLE sort of the flattened lists (equal neighbours keep the order of their pair numbers) and the cumulative counts of the
    m values, taken as a searchsorted over the sorted keys -- torch.bincount reads its size back from a CUDA tensor, which would
    synchronise and cannot be captured.  No synchronisation."""
    if not isinstance(idx, torch.Tensor) or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise TypeError(f"idx must be an integer tensor, got {getattr(idx, 'dtype', type(idx).__name__)}")
    if idx.dim() != 2:
        raise ValueError(f"idx must be (m, k1), got {tuple(idx.shape)}")
    m = idx.shape[0]
    flat = idx.reshape(-1)
    flat = torch.where((flat < 0) | (flat >= m), torch.zeros_like(flat), flat)
    keys, order = torch.sort(flat, stable=True)
    rev_start = torch.searchsorted(keys, torch.arange(m + 1, dtype=keys.dtype, device=keys.device), out_int32=True)
    return rev_start, order.to(torch.int32)


def identity_lists(n_rows, k):
    return (np.arange(n_rows + 1, dtype=np.int64) * k).astype(np.int32), np.arange(n_rows * k, dtype=np.int32)


def terms(src, coef=None, k=1, sign=1.0):
    """(pairs, c) float32: sign * src[q] (pair rows), or (sign * src[q // k]) * coef[q, ch % g] (query rows), each product rounded"""
    src = np.ascontiguousarray(src, dtype=F32).reshape(-1, np.shape(src)[-1])
    t = F32(sign) * src
    if coef is None:
        return t
    coef = np.ascontiguousarray(coef, dtype=F32).reshape(-1, np.shape(coef)[-1])
    pairs, g = coef.shape
    c = src.shape[1]
    assert c % g == 0 and pairs == src.shape[0] * k
    return (t[np.arange(pairs) // k] * coef[:, np.arange(c) % g]).astype(F32)


def scatter(n_rows, lists, src, coef=None, k=1, sign=1.0):
    """lists = (rev_start, rev_pair), or None for the identity segments of k pairs per row -> (n_rows, c) float32"""
    t = terms(src, coef, k, sign)
    rev_start, rev_pair = identity_lists(n_rows, k) if lists is None else (np.asarray(lists[0]).astype(np.int64), np.asarray(lists[1]).astype(np.int64))
    rev_start = rev_start.astype(np.int64)
    assert rev_start.shape == (n_rows + 1,) and rev_pair.shape == (t.shape[0],)
    out = np.zeros((n_rows, t.shape[1]), dtype=F32)
    length = rev_start[1:] - rev_start[:-1]
    for j in range(int(length.max()) if n_rows else 0):
        rows = np.nonzero(length > j)[0]
        out[rows] = out[rows] + t[rev_pair[rev_start[rows] + j]]
    return out


def scatter_f64(n_rows, lists, src, coef=None, k=1, sign=1.0):
    """(exact, sum of |terms|) in float64 from the same float32 inputs, terms unrounded: what a bound is scaled by"""
    src = np.asarray(src, dtype=np.float64).reshape(-1, np.shape(src)[-1])
    if coef is None:
        t = sign * src
    else:
        coef = np.asarray(coef, dtype=np.float64).reshape(-1, np.shape(coef)[-1])
        t = sign * src[np.arange(coef.shape[0]) // k] * coef[:, np.arange(src.shape[1]) % coef.shape[1]]
    rev_start, rev_pair = identity_lists(n_rows, k) if lists is None else lists
    rev_start = np.asarray(rev_start).astype(np.int64)
    row_of = np.empty(t.shape[0], dtype=np.int64)
    row_of[np.asarray(rev_pair).astype(np.int64)] = np.repeat(np.arange(n_rows), rev_start[1:] - rev_start[:-1])
    exact, absum = np.zeros((n_rows, t.shape[1])), np.zeros((n_rows, t.shape[1]))
    np.add.at(exact, row_of, t)
    np.add.at(absum, row_of, np.abs(t))
    return exact, absum
