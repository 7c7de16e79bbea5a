"""The closed form the fused contrastive-boundary kernels compute (include/tgn_pointops.h: tgn_cbl_stage_forward / _backward), in
float64 numpy, for tests/test_cbl_fused_host.py: the per-pair weights and the gradient written out by hand, where tests/cbl_ref.py
lets autograd differentiate the criterion.  That the two agree pins the derivation before any kernel runs.

  d_ij = sqrt(|f_i - f_idx[i,j]|^2 + 1e-12), e_ij = exp(-d_ij + min_j d_ij), neg_i = sum_j e_ij, pos_i = sum_j e_ij [label equal],
  r_i = pos_i / neg_i; a point contributes when 0 < #equal < k1, with -log(r_i + 1e-12); loss = 0.1 * sum / max(count, 1)
  pair_w[i, j] = e_ij ([label equal] - r_i) / (neg_i (r_i + 1e-12) d_ij) for a contributing point, 0 for every other row
  grad_f[i] = s (sum_j pair_w[i, j] (f_i - f_idx[i,j]) - sum_{q in rev(i)} pair_w[q] (f_{q // k1} - f_i)), s = grad_loss 0.1 / max(count, 1)
  rev(i): the pair numbers q = i' k1 + j with idx[i', j] == i, ascending"""
import numpy as np

WEIGHT, EPS = 0.1, 1e-12


def reverse_lists(idx):
    """(rev_start (m + 1,), rev_pair (m k1,)) by a Python loop over the pairs in ascending pair number"""
    m, k1 = idx.shape
    lists = [[] for _ in range(m)]
    for q, i in enumerate(np.asarray(idx).reshape(-1).tolist()):
        lists[i].append(q)
    start = np.zeros(m + 1, np.int64)
    start[1:] = np.cumsum([len(x) for x in lists])
    return start, np.array([q for x in lists for q in x], np.int64).reshape(-1)


def forward(f, idx, labels):
    """-> dict(loss, count, pair_w (m, k1), on (m,) bool), float64"""
    f, idx, labels = np.asarray(f, np.float64), np.asarray(idx, np.int64), np.asarray(labels, np.int64)
    k1 = idx.shape[1]
    diff = f[:, None, :] - f[idx]
    d = np.sqrt((diff ** 2).sum(-1) + EPS)
    e = np.exp(-d + d.min(1, keepdims=True))
    same = labels[idx] == labels[:, None]
    neg, pos, npos = e.sum(1), (e * same).sum(1), same.sum(1)
    on = (npos > 0) & (npos < k1)
    r = pos / neg
    value = -np.log(r + EPS)
    count = int(on.sum())
    pair_w = np.where(on[:, None], e * (same - r[:, None]) / (neg[:, None] * (r[:, None] + EPS) * d), 0.0)
    return dict(loss=WEIGHT * float(value[on].sum()) / max(count, 1), count=count, pair_w=pair_w, on=on)


def backward(f, idx, pair_w, count, grad_loss=1.0):
    """-> grad_f (m, c) float64, row by row along the reverse lists"""
    f, idx = np.asarray(f, np.float64), np.asarray(idx, np.int64)
    m, k1 = idx.shape
    start, pair = reverse_lists(idx)
    w = pair_w.reshape(-1)
    g = np.zeros_like(f)
    for i in range(m):
        acc = (pair_w[i][:, None] * (f[i][None] - f[idx[i]])).sum(0)
        for q in pair[start[i]:start[i + 1]]:
            acc = acc - w[q] * (f[q // k1] - f[i])
        g[i] = acc
    return g * (grad_loss * WEIGHT / max(count, 1))
