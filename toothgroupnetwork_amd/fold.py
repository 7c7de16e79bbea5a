"""Eval-mode BatchNorm folded into the layer in front of it: the ONE place that knows the fold.

Every fused eval path starts from (W', b') with bn(layer(x)) == x @ W'.T + b'.  Pure tensor functions, on whatever device the
parameters live (the CPU included), memoised through _derived.cached until a parameter or running statistic is written.  The kernel
layouts (transposes, splits, padding) stay with the modules that know their kernels and take (W', b') from here.

The rule for b': an absent term is skipped, never replaced by 0 or 1, so the present ones arrive bit for bit (the sign of a zero
included) -- no bias: b' = shift; no BatchNorm: W' = W and b' = bias, zeros only where there is neither.
"""
import torch

from . import _derived


def scale_shift(bn):
    """Eval-mode BatchNorm as the affine map y = scale * x + shift: two packed float32 (C,) tensors, memoised on `bn`."""
    def build():
        scale = (bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)).float()
        return scale.contiguous(), (bn.bias.detach() - bn.running_mean * scale).float().contiguous()
    return _derived.cached(bn, "scale_shift", _derived.sources(bn), None, build)


def affine(layer, bn=None):
    """(W' (C_out, C_in), b' (C_out,)), packed float32, of an nn.Linear or a 1x1 nn.Conv1d / nn.Conv2d `layer` followed by the
    eval-mode BatchNorm `bn` (None: the layer alone).  Memoised on `bn` (on `layer` without one)."""
    def build():
        W = layer.weight.detach().reshape(layer.weight.shape[0], -1).float()
        bias = None if layer.bias is None else layer.bias.detach().float()
        if bn is None:
            return W.contiguous(), (W.new_zeros(W.shape[0]) if bias is None else bias.contiguous())
        scale, shift = scale_shift(bn)
        return (W * scale[:, None]).contiguous(), (shift if bias is None else bias * scale + shift).contiguous()
    if bn is None:
        return _derived.cached(layer, "affine", _derived.sources(layer), None, build)
    return _derived.cached(bn, "affine", _derived.sources(layer, bn), None, build)


def frozen(module, *tensors):
    """The fused eval paths apply: `module` is in eval mode and nothing asks for a gradient through it."""
    return (not module.training) and not (torch.is_grad_enabled() and (
        any(t is not None and t.requires_grad for t in tensors) or any(q.requires_grad for q in module.parameters())))
