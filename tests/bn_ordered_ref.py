"""The summation order of tgn_bn_rows_forward_ordered / tgn_bn_rows_backward_ordered (include/tgn_pointops.h, csrc/bnorm.hip) in
numpy: float32 terms, float64 accumulators, every add in the stated place.  The library is built with -ffp-contract=off and adds,
multiplies, divides and converts as IEEE 754 says, so what this file computes from the same operands is what the kernels compute, bit
for bit, for every quantity that is sums, divisions and casts: save_mean, running_mean, running_var, dbeta, dgamma.  (save_invstd
goes through a square root and a reciprocal; it is the same expression here, and the tests hold it to a bound.)

  grid(rows, C)          -> B, the blocks of the reduction: min(1024, max(1, ceil(rows C / 8192))) rounded up to a multiple of
                            C / gcd(256, C); T = 256 B threads, thread t keeps column t % C
  thread_sums(terms)     step 1: thread t adds terms[t], terms[t + T], ... in ascending order from +0.0
  block_partials(...)    step 2: in block b thread i < min(C, 256) adds the sums of threads i + C, i + 2 C, ... < 256 to its own, ascending:
                            the partial of column (256 b + i) % C; +0.0 for a column no thread of the block keeps
  combine(partials)      steps 3 and 4: per column 64 chains (chain j: blocks j, j + 64, ... ascending from +0.0), then the chains
                            j < min(B, 64) ascending from +0.0.  `block_order` permutes the blocks first: the tests use it to show that the
                            result depends on the order
  forward / backward     the terms, the two sums and the finalisation
"""
import math

import numpy as np

THREADS, CHAINS, MAX_BLOCKS, PER_BLOCK = 256, 64, 1024, 256 * 32


def grid(rows, C):
    total = rows * C
    m = C // math.gcd(THREADS, C)
    b = min(MAX_BLOCKS, max(1, -(-total // PER_BLOCK)))
    return -(-b // m) * m


def workspace_bytes(rows, C):
    return grid(rows, C) * 2 * C * 8


def thread_sums(terms, B):
    """terms (rows * C,) float64 (each already rounded as the kernel rounds it) -> (T,) float64"""
    T = B * THREADS
    trips = -(-terms.size // T)
    padded = np.zeros(trips * T, np.float64)      # (a thread past the end adds nothing; +0.0 changes no sum that started at +0.0)
    padded[:terms.size] = terms
    s = np.zeros(T, np.float64)
    for trip in padded.reshape(trips, T):
        s = s + trip
    return s


def block_partials(s, B, C):
    """(T,) thread sums -> (B, C) per-block, per-column partials"""
    per = s.reshape(B, THREADS)
    part = np.zeros((B, C), np.float64)
    owners = min(C, THREADS)
    acc = per[:, :owners].copy()
    for u in range(C, THREADS, C):               # threads i + C, i + 2 C, ...: the last round may cover a prefix of the owners only
        w = min(owners, THREADS - u)
        acc[:, :w] = acc[:, :w] + per[:, u:u + w]
    cols = (np.arange(B)[:, None] * THREADS + np.arange(owners)[None, :]) % C
    np.put_along_axis(part, cols, acc, axis=1)
    return part


def combine(part, block_order=None):
    """(B, C) partials -> (C,) sums"""
    if block_order is not None:
        part = part[np.asarray(block_order)]
    B, C = part.shape
    chains = np.zeros((CHAINS, C), np.float64)
    for b in range(B):
        chains[b % CHAINS] = chains[b % CHAINS] + part[b]
    total = np.zeros(C, np.float64)
    for j in range(min(B, CHAINS)):
        total = total + chains[j]
    return total


def ordered_sum(terms, rows, C, block_order=None):
    B = grid(rows, C)
    return combine(block_partials(thread_sums(terms.reshape(-1), B), B, C), block_order)


def forward_partials(x):
    """the two (B, C) partial arrays of the forward: for the test that permutes them"""
    rows, C = x.shape
    B = grid(rows, C)
    xd = x.astype(np.float32).astype(np.float64).reshape(-1)
    return block_partials(thread_sums(xd, B), B, C), block_partials(thread_sums(xd * xd, B), B, C)


def forward(x, eps, momentum, running_mean=None, running_var=None, block_order=None):
    """x (rows, C) float32 -> dict(save_mean, save_invstd float32; mean, var, invstd float64; running_mean, running_var float32 when
    given).  eps and momentum reach the kernel as floats."""
    rows, C = x.shape
    p1, p2 = forward_partials(x)                              # (double)x; (double)x * (double)x is exact
    s1, s2 = combine(p1, block_order), combine(p2, block_order)
    n = np.float64(rows)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    out = dict(mean=mean, var=var, invstd=invstd, save_mean=mean.astype(np.float32), save_invstd=invstd.astype(np.float32))
    if running_mean is not None:
        m = np.float64(np.float32(momentum))
        unbiased = var * (n / (n - 1.0))
        out["running_mean"] = ((1.0 - m) * running_mean.astype(np.float64) + m * mean).astype(np.float32)
        out["running_var"] = ((1.0 - m) * running_var.astype(np.float64) + m * unbiased).astype(np.float32)
    return out


def backward_sums(x, y, dy, save_mean, save_invstd, relu):
    """-> (dbeta, dgamma) float32: g = dy (0 where relu and y <= 0); the second term g * ((x - mean) * invstd) all in float32"""
    rows, C = x.shape
    f = np.float32
    g = np.where(y > 0, dy, f(0)).astype(f) if relu else dy.astype(f)
    xhat = ((x.astype(f) - save_mean.astype(f)[None, :]).astype(f) * save_invstd.astype(f)[None, :]).astype(f)
    gx = (g * xhat).astype(f)
    return (ordered_sum(g.astype(np.float64), rows, C).astype(f), ordered_sum(gx.astype(np.float64), rows, C).astype(f))
