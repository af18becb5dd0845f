"""Drop-in ``CLAM_MB`` of ``models/model_clam.py`` (code/models/model_clam.py:195-268; Lu et al.
2021, multi-branch CLAM) on the MI355X HIP kernels.

Same constructor, submodule layout and parameter names, so the reference's state dict loads with
``strict=True``.  The forward is one autograd node, ``clam_pool``: ``h = ReLU(x W1^T + b1)`` and
``Z = h [Wa;Wb]^T + [ba;bb]`` on the HIP GEMM (f32 MFMA) with the bias + ReLU as one HIP pass, then
``tm_clam_fwd`` (two launches: the K attention scores, the K softmax-pooled rows ``M = p h`` and the
bag logits from one read of Z and h; the per-class two-sided top-``k_sample`` selection and the
instance classifiers' cross entropy with the label read on the device).  The backward is
``tm_clam_bwd`` plus the GEMM / column-sum launches of the three Linear layers and one ReLU-backward
pass.  fp32 throughout, like AttMIL's fp32 mode (there is no ``set_compute_dtype``).

The reference ranks the softmaxed attention; the kernels rank the raw fp32 scores (the softmax is
monotone) and, among equal scores, take the lower instance index first (torch leaves that order
open), so the selected indices and every gradient repeat bitwise from run to run.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..engine import Pool, _p, _stream
from ..gated import _f32c, device_label, embed, embed_bwd

IN_FEATURES = 1024
MAX_CLASSES = 8
MAX_K_SAMPLE = 32


class _ClamFn(torch.autograd.Function):
    """(x [N, 1024], fc weight / bias, attention_a / _b / _c weights and biases, the stacked bag
    classifiers [K, L] / [K], the stacked instance classifiers [K, 2, L] / [K, 2], label (a device
    int64 tensor or None), k_sample, subtyping) -> (logits [1, K], instance_loss [], A_raw [K, N],
    M [K, L], idx / inst_preds / inst_targets [K, 2 k_sample] int32)."""

    @staticmethod
    def forward(ctx, x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wcls, bcls, Wic, bic, label, k_sample, subtyping):
        N = x.shape[0]
        K, D, L = Wc.shape[0], Wc.shape[1], W1.shape[0]
        dev = x.device
        W1_, b1_, Wc_, bc_, Wcls_, bcls_, Wic_, bic_ = (_f32c(t) for t in (W1, b1, Wc, bc, Wcls, bcls, Wic, bic))
        Wab = torch.cat([Wa.detach(), Wb.detach()]).float().contiguous()
        bab = torch.cat([ba.detach(), bb.detach()]).float().contiguous()
        h, Z = embed(x, W1_, b1_, Wab, bab)
        work = torch.empty(max(_lib.query("tm_clam_fwd_workspace", N, K), 4) // 4, device=dev)
        A_raw, stats = torch.empty(K, N, device=dev), torch.empty(K, 2, device=dev)
        M, logits = torch.empty(K, L, device=dev), torch.empty(1, K, device=dev)
        inst = label is not None
        k2 = 2 * k_sample
        loss = torch.empty((), device=dev) if inst else None
        idx, preds, targets = (torch.empty(K, k2, dtype=torch.int32, device=dev) if inst else None for _ in range(3))
        dil = torch.empty(K, k2, 2, device=dev) if inst else None
        _lib.call("tm_clam_fwd", _p(Z), _p(h), N, L, D, K, _p(Wc_), _p(bc_), _p(Wcls_), _p(bcls_), _p(Wic_), _p(bic_),
                  _p(label), k_sample, int(subtyping), _p(work), _p(A_raw), _p(stats), _p(M), _p(logits), _p(loss),
                  _p(idx), _p(preds), _p(targets), _p(dil), _stream())
        ctx.save_for_backward(x, W1_, Wab, Wc_, Wcls_, Wic_, h, Z, A_raw, stats, M, idx, dil)
        ctx.k_sample, ctx.inst = k_sample, inst
        if not inst:
            loss = torch.zeros((), device=dev)
            idx, preds, targets = (torch.empty(0, dtype=torch.int32, device=dev) for _ in range(3))
        ctx.mark_non_differentiable(A_raw, M, idx, preds, targets)
        ctx.set_materialize_grads(False)
        return logits, loss, A_raw, M, idx, preds, targets

    @staticmethod
    def backward(ctx, dlogits, dloss, *_unused):
        if dlogits is None and (dloss is None or not ctx.inst):
            return (None,) * 16
        x, W1, Wab, Wc, Wcls, Wic, h, Z, A_raw, stats, M, idx, dil = ctx.saved_tensors
        N = x.shape[0]
        K, D, L = Wc.shape[0], Wc.shape[1], W1.shape[0]
        D2 = 2 * D
        dev = x.device
        inst = ctx.inst and dloss is not None
        if dlogits is not None:
            dlogits = dlogits.float().contiguous()
        if dloss is not None:
            dloss = dloss.float().contiguous()
        k = ctx.k_sample if inst else 0
        work = torch.empty(max(_lib.query("tm_clam_bwd_workspace", N, D, K, k), 4) // 4, device=dev)
        dZ, dh = torch.empty(N, D2, device=dev), torch.empty(N, L, device=dev)
        dWc, dbc = torch.empty(K, D, device=dev), torch.empty(K, device=dev)
        dWcls, dbcls = torch.empty(K, L, device=dev), torch.empty(K, device=dev)
        dWic = torch.empty(K, 2, L, device=dev) if inst else None
        dbic = torch.empty(K, 2, device=dev) if inst else None
        _lib.call("tm_clam_bwd", _p(Z), _p(h), _p(A_raw), _p(stats), _p(M), N, L, D, K, _p(Wc), _p(Wcls), _p(Wic),
                  _p(idx if inst else None), _p(dil if inst else None), k, _p(dlogits), _p(dloss if inst else None),
                  _p(work), _p(dZ), _p(dh), _p(dWc), _p(dbc), _p(dWcls), _p(dbcls), _p(dWic), _p(dbic), _stream())
        # attention_a / attention_b, the ReLU, then the first Linear
        dx, dW1, db1, dWab, dbab = embed_bwd(dZ, dh, h, x, W1, Wab, Pool(dev), need_dx=ctx.needs_input_grad[0],
                                             need_dW1=True, need_db1=True)
        return (dx, dW1, db1, dWab[:D], dbab[:D], dWab[D:], dbab[D:], dWc, dbc, dWcls, dbcls, dWic, dbic,
                None, None, None)


def _check_input(x):
    if not x.is_cuda:
        raise RuntimeError("CLAM_MB (HIP) needs a GPU tensor: there is no CPU path")
    if x.dim() != 2 or x.shape[1] != IN_FEATURES:
        raise ValueError(f"CLAM_MB: x must be [N, {IN_FEATURES}], got {tuple(x.shape)}")
    return x.float().contiguous()


def clam_pool(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wcls, bcls, Wic, bic, label=None, k_sample=8, subtyping=False):
    """The fused node on a ``[N, 1024]`` fp32 GPU bag.  ``Wcls [K, L]`` / ``bcls [K]`` are the K bag
    classifiers stacked, ``Wic [K, 2, L]`` / ``bic [K, 2]`` the K instance classifiers.  ``label``: a
    GPU int64 tensor (its first element is read by the kernel, never on the host) switches the
    instance evaluation on.  Returns device tensors only and never synchronises:
    ``(logits [1, K], A_raw [K, N], M [K, L], instance_loss [], idx, inst_preds, inst_targets)``;
    the last three are int32 ``[K, 2 k_sample]`` with -1 in the slots of a class that was not evaluated
    (and in the second half of an out-of-class row), or empty without a label.  ``logits`` and
    ``instance_loss`` are differentiable."""
    x = _check_input(x)
    K, k_sample = Wc.shape[0], int(k_sample)
    if not 1 <= K <= MAX_CLASSES:
        raise RuntimeError(f"CLAM_MB: n_classes must be in [1, {MAX_CLASSES}] on the HIP path, got {K}")
    if label is not None:
        if not 1 <= k_sample <= MAX_K_SAMPLE:
            raise RuntimeError(f"CLAM_MB: k_sample must be in [1, {MAX_K_SAMPLE}] on the HIP path, got {k_sample}")
        if x.shape[0] < k_sample:
            raise RuntimeError(f"CLAM_MB: selected index k out of range (a bag of {x.shape[0]} instances, "
                               f"k_sample = {k_sample})")
        label = device_label(label, "CLAM_MB")
    logits, loss, A_raw, M, idx, preds, targets = _ClamFn.apply(x, W1, b1, Wa, ba, Wb, bb, Wc, bc, Wcls, bcls, Wic,
                                                                bic, label, k_sample, bool(subtyping))
    return logits, A_raw, M, loss, idx, preds, targets


def clam_scores(x, W1, b1, Wa, ba, Wb, bb, Wc, bc):
    """``A_raw [K, N]`` alone (``attention_only``): the two GEMMs and the score pass.  Not differentiable."""
    x = _check_input(x)
    with torch.no_grad():
        h, Z = embed(x, _f32c(W1), _f32c(b1), torch.cat([Wa, Wb]).float().contiguous(),
                      torch.cat([ba, bb]).float().contiguous())
        K, D = Wc.shape
        A_raw = torch.empty(K, x.shape[0], device=x.device)
        _lib.call("tm_clam_scores", _p(Z), x.shape[0], D, K, _p(_f32c(Wc)), _p(_f32c(bc)), _p(A_raw), _stream())
    return A_raw


class Attn_Net_Gated(nn.Module):
    """``model_clam.py:42-67``: the parameter container of the gated attention branch (the arithmetic
    runs in ``clam_pool``)."""

    def __init__(self, L=1024, D=256, dropout=False, n_classes=1):
        super().__init__()
        if dropout:
            raise NotImplementedError("CLAM_MB (HIP): dropout=True is not on the MI355X path")
        self.attention_a = nn.Sequential(nn.Linear(L, D), nn.Tanh())
        self.attention_b = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
        self.attention_c = nn.Linear(D, n_classes)


def _is_default_cross_entropy(fn):
    return (type(fn) is nn.CrossEntropyLoss and fn.weight is None and fn.reduction == "mean"
            and fn.ignore_index == -100 and getattr(fn, "label_smoothing", 0.0) == 0.0)


class CLAM_MB(nn.Module):
    """``code/models/model_clam.py:195-268``.  ``forward`` returns the reference's
    ``(logits [1, K], Y_prob, Y_hat [1, 1], A_raw [K, N], results_dict)``."""

    def __init__(self, gate=True, size_arg="small", dropout=False, k_sample=8, n_classes=2,
                 instance_loss_fn=nn.CrossEntropyLoss(), subtyping=False):
        super().__init__()
        if not gate:
            raise NotImplementedError("CLAM_MB (HIP): gate=False (Attn_Net) is not on the MI355X path")
        if dropout:
            raise NotImplementedError("CLAM_MB (HIP): dropout=True is not on the MI355X path")
        if not _is_default_cross_entropy(instance_loss_fn):
            raise NotImplementedError("CLAM_MB (HIP): instance_loss_fn must be a default nn.CrossEntropyLoss() "
                                      "(the instance loss is computed by the HIP kernel)")
        self.size_dict = {"small": [1024, 512, 256], "big": [1024, 512, 384]}
        size = self.size_dict[size_arg]
        self.attention_net = nn.Sequential(nn.Linear(size[0], size[1]), nn.ReLU(),
                                           Attn_Net_Gated(L=size[1], D=size[2], dropout=dropout, n_classes=n_classes))
        self.classifiers = nn.ModuleList([nn.Linear(size[1], 1) for _ in range(n_classes)])
        self.instance_classifiers = nn.ModuleList([nn.Linear(size[1], 2) for _ in range(n_classes)])
        self.k_sample = k_sample
        self.instance_loss_fn = instance_loss_fn
        self.n_classes = n_classes
        self.subtyping = subtyping
        for m in self.modules():                                    # Initialize_weights (:272-280)
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight)
                m.bias.data.zero_()

    def relocate(self):
        """The reference's ``relocate()`` (:97-105): the module on the GPU (no DataParallel split)."""
        return self.to(torch.device("cuda"))

    def _params(self):
        fc, gated = self.attention_net[0], self.attention_net[2]
        a, b, c = gated.attention_a[0], gated.attention_b[0], gated.attention_c
        return fc.weight, fc.bias, a.weight, a.bias, b.weight, b.bias, c.weight, c.bias

    def forward(self, h, label=None, instance_eval=False, return_features=False, attention_only=False):
        if not h.is_cuda:
            raise RuntimeError("CLAM_MB (HIP) needs a GPU tensor: there is no CPU path")
        if h.dim() == 3 and h.shape[0] == 1:        # [1, N, 1024]: the task's bag layout
            h = h[0]
        if h.dim() != 2 or h.shape[1] != IN_FEATURES:
            raise ValueError(f"CLAM_MB: h must be [N, {IN_FEATURES}] or [1, N, {IN_FEATURES}], got {tuple(h.shape)}")
        if attention_only:
            return clam_scores(h, *self._params())
        if instance_eval:
            if label is None:
                raise ValueError("CLAM_MB: instance_eval=True needs a label")
            label = torch.as_tensor(label).to(device=h.device, dtype=torch.int64).reshape(-1)
        else:
            label = None
        Wcls = torch.cat([m.weight for m in self.classifiers])                  # [K, L]
        bcls = torch.cat([m.bias for m in self.classifiers])                    # [K]
        Wic = torch.stack([m.weight for m in self.instance_classifiers])        # [K, 2, L]
        bic = torch.stack([m.bias for m in self.instance_classifiers])          # [K, 2]
        logits, A_raw, M, loss, _, preds, targets = clam_pool(h, *self._params(), Wcls, bcls, Wic, bic, label,
                                                              self.k_sample, self.subtyping)
        Y_hat = torch.topk(logits, 1, dim=1)[1]
        Y_prob = F.softmax(logits, dim=1)
        results_dict = {}
        if instance_eval:
            # the one device-to-host copy: the evaluated slots, in class order as the reference lists them
            pt = torch.stack([preds, targets]).cpu().numpy().reshape(2, -1)
            keep = pt[1] >= 0
            results_dict = {"instance_loss": loss, "inst_labels": pt[1][keep].astype("int64"),
                            "inst_preds": pt[0][keep].astype("int64")}
        if return_features:
            results_dict.update({"features": M})
        return logits, Y_prob, Y_hat, A_raw, results_dict
