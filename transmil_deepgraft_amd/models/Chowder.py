"""Drop-in ``models/Chowder.py`` (code/models/Chowder.py:19-50; Courtiol et al. 2018) on the
MI355X HIP kernels.

Same constructor and parameter names.  The forward is one autograd node over ``tm_chowder_fwd``
(instance scores ``x . w + b`` fused with the selection of the R smallest and R largest, then the
2R -> 200 -> 100 -> n_classes affine head; two launches) and ``tm_chowder_bwd``.  The reference
transposes, runs a ``Conv1d``, writes the N scores, reads them back through two ``topk`` calls,
concatenates and runs three ``Linear`` layers.  fp32 arithmetic; a bf16 bag is read as bf16.

Ties: among equal scores the lower instance index is selected first (torch leaves the order open),
so the selected indices and the gradients are bitwise stable from run to run.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _lib
from .._lib import BF16, F32
from ..engine import _p, _stream


class _ChowderFn(torch.autograd.Function):
    """(x [B, N, L], f1 weight [L] / bias [1], the three Linear weights and biases, R, want_scores)
    -> (logits [B, C], vals [B, 2R], idx [B, 2R] int32, scores [B, N] or an empty tensor)."""

    @staticmethod
    def forward(ctx, x, w, b, W1, b1, W2, b2, W3, b3, R, want_scores):
        B, N, L = x.shape
        H1, H2, C = W1.shape[0], W2.shape[0], W3.shape[0]
        if N < R:
            raise RuntimeError(f"Chowder: selected index k out of range (a bag of {N} instances, r = {R})")
        dev = x.device
        dtype = BF16 if x.dtype == torch.bfloat16 else F32
        params = [t.detach().float().contiguous() for t in (w, b, W1, b1, W2, b2, W3, b3)]
        w_, b_, W1_, b1_, W2_, b2_, W3_, b3_ = params
        nbytes = _lib.query("tm_chowder_fwd_workspace", B, N, L, R)
        work = torch.empty(max(nbytes, 4) // 4, device=dev)
        scores = torch.empty(B, N, device=dev) if want_scores else None
        vals = torch.empty(B, 2 * R, device=dev)
        idx = torch.empty(B, 2 * R, dtype=torch.int32, device=dev)
        hid = torch.empty(B, H1 + H2, device=dev)
        logits = torch.empty(B, C, device=dev)
        _lib.call("tm_chowder_fwd", dtype, _p(x), B, N, L, _p(w_), _p(b_), R, _p(W1_), _p(b1_), H1, _p(W2_), _p(b2_),
                  H2, _p(W3_), _p(b3_), C, _p(work), _p(scores), _p(vals), _p(idx), _p(hid), _p(logits), _stream())
        ctx.save_for_backward(x, w_, W1_, W2_, W3_, vals, idx, hid)
        ctx.R, ctx.dtype = R, dtype
        if scores is None:
            scores = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(vals, idx, scores)
        ctx.set_materialize_grads(False)
        return logits, vals, idx, scores

    @staticmethod
    def backward(ctx, dlogits, _dvals, _didx, _dscores):
        if dlogits is None:
            return (None,) * 11
        x, w, W1, W2, W3, vals, idx, hid = ctx.saved_tensors
        B, N, L = x.shape
        H1, H2, C, R = W1.shape[0], W2.shape[0], W3.shape[0], ctx.R
        dev = x.device
        nbytes = _lib.query("tm_chowder_bwd_workspace", B, L, R, H1, H2, C)
        work = torch.empty(max(nbytes, 4) // 4, device=dev)
        dw, db = torch.empty(L, device=dev), torch.empty(1, device=dev)
        dW1, db1 = torch.empty_like(W1), torch.empty(H1, device=dev)
        dW2, db2 = torch.empty_like(W2), torch.empty(H2, device=dev)
        dW3, db3 = torch.empty_like(W3), torch.empty(C, device=dev)
        dx = torch.empty(B, N, L, device=dev) if ctx.needs_input_grad[0] else None
        _lib.call("tm_chowder_bwd", ctx.dtype, _p(x), B, N, L, _p(w), R, _p(W1), H1, _p(W2), H2, _p(W3), C, _p(vals),
                  _p(idx), _p(hid), _p(dlogits.float().contiguous()), _p(work), _p(dw), _p(db), _p(dW1), _p(db1),
                  _p(dW2), _p(db2), _p(dW3), _p(db3), _p(dx), _stream())
        if dx is not None and dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        return dx, dw, db, dW1, db1, dW2, db2, dW3, db3, None, None


def chowder_pool(x, w, b, W1, b1, W2, b2, W3, b3, r, return_scores=False):
    """The fused node on a ``[B, N, L]`` fp32 / bf16 GPU bag: ``(logits [B, C], vals [B, 2r],
    idx [B, 2r] int32, scores [B, N] or None)``.  ``vals`` / ``idx``: the r smallest scores ascending,
    then the r largest descending, and their instance indices."""
    if not x.is_cuda:
        raise RuntimeError("Chowder (HIP) needs a GPU tensor: there is no CPU path")
    if x.dim() != 3:
        raise ValueError(f"Chowder: x must be [B, N, L], got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    logits, vals, idx, scores = _ChowderFn.apply(x.contiguous(), w, b, W1, b1, W2, b2, W3, b3, int(r),
                                                 bool(return_scores))
    return logits, vals, idx, (scores if return_scores else None)


class Chowder(nn.Module):
    """``code/models/Chowder.py:19-50``: ``f1`` scores every instance, the r smallest and r largest
    scores feed ``f2``.  ``forward`` returns ``(logits, None)`` as the reference does, or
    ``(logits, scores [B, N])`` with ``return_scores=True`` (the per-instance scores the reference
    computes and drops)."""

    def __init__(self, n_classes, features=512, r=5):
        super().__init__()
        self.L = features
        self.n_classes = n_classes
        self.R = r
        self.f1 = nn.Sequential(nn.Conv1d(self.L, 1, 1))
        self.f2 = nn.Sequential(nn.Linear(r * 2, 200), nn.Linear(200, 100), nn.Linear(100, self.n_classes))

    def forward(self, x, return_scores=False):
        if not x.is_cuda:
            raise RuntimeError("Chowder (HIP) needs a GPU tensor: there is no CPU path")
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] != self.L:
            raise ValueError(f"Chowder: x must be [N, {self.L}] or [B, N, {self.L}], got {tuple(x.shape)}")
        f1, f2 = self.f1[0], self.f2
        logits, _, _, scores = chowder_pool(x, f1.weight.reshape(-1), f1.bias, f2[0].weight, f2[0].bias,
                                            f2[1].weight, f2[1].bias, f2[2].weight, f2[2].bias, self.R,
                                            return_scores)
        # f2 acts on [B, 1, 2r] and squeeze(0) only drops a batch of one (:46-48)
        out = logits if logits.shape[0] == 1 else logits.unsqueeze(1)
        return out, scores
