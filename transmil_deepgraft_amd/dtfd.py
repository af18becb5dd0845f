"""DTFD-MIL (Zhang et al. 2022, double-tier feature distillation) as the reference trains it:
``ModelInterface_DTFD`` (code/models/model_interface_dtfd.py:162-279, 594-601) on the blocks of
``code/models/DTFDMIL.py``, on the MI355X HIP kernels.

The parameter containers carry the reference's names and constructor arguments, so the
``classifier.* / attention.* / dimreduction.* / attCls.*`` entries of a reference checkpoint load with
``strict=True``.  The arithmetic is one autograd node, ``dtfd_pool``: the G S rows that the permutation
selects are gathered (``tm_gather_rows``), ``h = ReLU(xg W1^T)`` and ``Z = h [Wv;Wu]^T + [bv;bu]`` run on
the HIP GEMM (f32 MFMA), and ``tm_dtfd_fwd`` (two launches) pools the G pseudo-bags, pools the G pooled
rows again and takes both cross entropies with the label read on the device.  Rows past ``G S`` reach no
output of the reference's all-N ``DimReduction`` either: their ``dx`` rows are exact zeros.  The
backward is ``tm_dtfd_bwd`` plus the GEMM / column-sum launches of the two Linear layers and one
ReLU-backward pass, and it skips what nobody needs: with only ``attCls`` trainable it is one launch.
fp32 throughout (there is no ``set_compute_dtype``).

The module lives beside ``nystrom_attention.py``, not under ``models``: the reference's ``load_model``
cannot build this model either (the Lightning module owns the parameters), so ``config.build_model``
keeps refusing ``Model.name: DTFDMIL`` and ``config.build_dtfd_task`` is the entry.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import F32
from .engine import Pool, _p, _stream
from .gated import _f32c, device_label, embed, embed_bwd

M_DIM = 512
MAX_D = 512
MAX_CLASSES = 8
MAX_BAG_SIZE = 1024
MAX_PSEUDO_BAGS = 64
_GATHER_ROWS = 65535          # tm_gather_rows' rows per launch


class _DtfdFn(torch.autograd.Function):
    """(x [N, F], idx [G S] int64, dimreduction.fc1 weight, attention V / U / weights, classifier.fc,
    the same of attCls, label (a device int64 tensor or None), G, S, return_cam) ->
    (sub [G, C], slide [1, C], sub_loss [], slide_loss [], M [G, L], p1 [G, S], p2 [G], Y_prob [1, C],
    Y_hat [1], cam [G, S, C] or None)."""

    @staticmethod
    def forward(ctx, x, idx, W1, Wv, bv, Wu, bu, w, b, Wc, bc, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, label, G, S,
                return_cam):
        N, Fin = x.shape
        L, D, C = W1.shape[0], Wv.shape[0], Wc.shape[0]
        R, D2 = G * S, 2 * D
        dev = x.device
        W1_, w_, b_, Wc_, bc_ = (_f32c(t) for t in (W1, w, b, Wc, bc))
        Wv2_, bv2_, Wu2_, bu2_, w2_, b2_, Wc2_, bc2_ = (_f32c(t) for t in (Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2))
        Wvu = torch.cat([Wv.detach(), Wu.detach()]).float().contiguous()
        bvu = torch.cat([bv.detach(), bu.detach()]).float().contiguous()
        xg = torch.empty(R, Fin, device=dev)
        for s in range(0, R, _GATHER_ROWS):
            e = min(R, s + _GATHER_ROWS)
            _lib.call("tm_gather_rows", F32, _p(x), Fin, _p(idx[s:e]), None, None, None, e - s, _p(xg[s:e]), _stream())
        h, Z = embed(xg, W1_, None, Wvu, bvu)           # dimreduction.fc1 has no bias
        p1, M, sub = torch.empty(G, S, device=dev), torch.empty(G, L, device=dev), torch.empty(G, C, device=dev)
        cam = torch.empty(G, S, C, device=dev) if return_cam else None
        Z2, p2, F = torch.empty(G, D2, device=dev), torch.empty(G, device=dev), torch.empty(L, device=dev)
        slide, yprob = torch.empty(1, C, device=dev), torch.empty(1, C, device=dev)
        yhat = torch.empty(1, dtype=torch.int64, device=dev)
        losses = torch.empty(2, device=dev) if label is not None else None
        _lib.call("tm_dtfd_fwd", _p(Z), _p(h), G, S, L, D, C, _p(w_), _p(b_), _p(Wc_), _p(bc_), _p(Wv2_), _p(bv2_),
                  _p(Wu2_), _p(bu2_), _p(w2_), _p(b2_), _p(Wc2_), _p(bc2_), _p(label), _p(p1), _p(M), _p(sub),
                  _p(cam), _p(Z2), _p(p2), _p(F), _p(slide), _p(losses), _p(yprob), _p(yhat), _stream())
        ctx.save_for_backward(xg, idx, W1_, Wvu, h, Z, p1, M, p2, Z2, F, sub, slide, label, w_, Wc_, Wv2_, Wu2_, w2_,
                              Wc2_)
        ctx.dims = (N, Fin, G, S, L, D, C)
        sub_loss, slide_loss = (losses[0], losses[1]) if label is not None else (None, None)
        ctx.mark_non_differentiable(*(t for t in (M, p1, p2, yprob, yhat, cam) if t is not None))
        ctx.set_materialize_grads(False)
        return sub, slide, sub_loss, slide_loss, M, p1, p2, yprob, yhat, cam

    @staticmethod
    def backward(ctx, dsub, dslide, gsub, gslide, *_unused):
        need = ctx.needs_input_grad
        need_t1, need_t2 = need[0] or any(need[2:11]), any(need[11:19])
        if all(g is None for g in (dsub, dslide, gsub, gslide)) or not (need_t1 or need_t2):
            return (None,) * 23
        (xg, idx, W1, Wvu, h, Z, p1, M, p2, Z2, F, sub, slide, label, w, Wc, Wv2, Wu2, w2, Wc2) = ctx.saved_tensors
        N, Fin, G, S, L, D, C = ctx.dims
        R, D2 = G * S, 2 * D
        dev = M.device
        dsub, dslide, gsub, gslide = (g.float().contiguous() if g is not None else None
                                      for g in (dsub, dslide, gsub, gslide))
        work = torch.empty(max(_lib.query("tm_dtfd_bwd_workspace", G, D, C), 4) // 4, device=dev)
        dZ = dh = dw = db = dWc = dbc = None
        if need_t1:
            dZ, dh = torch.empty(R, D2, device=dev), torch.empty(R, L, device=dev)
            dw, db = torch.empty(1, D, device=dev), torch.empty(1, device=dev)
            dWc, dbc = torch.empty(C, L, device=dev), torch.empty(C, device=dev)
        dWv2 = dbv2 = dWu2 = dbu2 = dw2 = db2 = dWc2 = dbc2 = None
        if need_t2:
            dWv2, dWu2 = torch.empty(D, L, device=dev), torch.empty(D, L, device=dev)
            dbv2, dbu2 = torch.empty(D, device=dev), torch.empty(D, device=dev)
            dw2, db2 = torch.empty(1, D, device=dev), torch.empty(1, device=dev)
            dWc2, dbc2 = torch.empty(C, L, device=dev), torch.empty(C, device=dev)
        _lib.call("tm_dtfd_bwd", _p(Z), _p(h), _p(p1), _p(M), _p(p2), _p(Z2), _p(F), _p(sub), _p(slide), _p(label),
                  G, S, L, D, C, _p(w), _p(Wc), _p(Wv2), _p(Wu2), _p(w2), _p(Wc2), _p(dsub), _p(dslide), _p(gsub),
                  _p(gslide), int(need_t1), int(need_t2), _p(work), _p(dZ), _p(dh), _p(dw), _p(db), _p(dWc), _p(dbc),
                  _p(dWv2), _p(dbv2), _p(dWu2), _p(dbu2), _p(dw2), _p(db2), _p(dWc2), _p(dbc2), _stream())
        dx = dW1 = dWvu = dbvu = None
        if need[0] or any(need[2:7]):
            # attention_V / attention_U, the ReLU, then dimreduction.fc1 (no bias)
            dxg, dW1, _, dWvu, dbvu = embed_bwd(dZ, dh, h, xg, W1, Wvu, Pool(dev), need_dx=need[0], need_dW1=need[2],
                                                need_db1=False)
            if need[0]:
                # zero-filled, then plain stores at the selected rows (the permutation makes them distinct)
                dx = torch.zeros(N, Fin, device=dev)
                _lib.call("tm_scatter_rows", _p(dxg), _p(idx), R, Fin, N, _p(dx), _stream())
        split = (lambda t, lo: t[lo * D:(lo + 1) * D]) if dWvu is not None else (lambda t, lo: None)
        return (dx, None, dW1, split(dWvu, 0), split(dbvu, 0), split(dWvu, 1), split(dbvu, 1), dw, db, dWc, dbc,
                dWv2, dbv2, dWu2, dbu2, dw2, db2, dWc2, dbc2, None, None, None, None)


def _check_bag(x):
    if not x.is_cuda:
        raise RuntimeError("DTFDMIL (HIP) needs a GPU tensor: there is no CPU path")
    if x.dim() == 3 and x.shape[0] == 1:        # [1, N, F]: the task's bag layout (x.squeeze(0), :183)
        x = x[0]
    if x.dim() != 2:
        raise ValueError(f"DTFDMIL: x must be [N, F] or [1, N, F], got {tuple(x.shape)}")
    return x.float().contiguous()               # x.float() (:176)


def pseudo_bags(N, bag_size, max_pseudo_bags):
    """G = min(max_pseudo_bags, N // bag_size) (:177-178)."""
    return min(int(max_pseudo_bags), int(N) // int(bag_size))


def dtfd_pool(x, perm, W1, Wv, bv, Wu, bu, w, b, Wc, bc, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, bag_size=120,
              max_pseudo_bags=8, label=None, return_cam=False):
    """The fused node on a ``[N, F]`` fp32 GPU bag.  ``perm``: a GPU int64 tensor of distinct row ids in
    ``[0, N)`` (the caller's contract; it is never read on the host); pseudo-bag ``g`` of
    ``G = min(max_pseudo_bags, N // bag_size)`` holds rows ``perm[g S : (g + 1) S]``.  ``W1`` is
    ``dimreduction.fc1.weight``; ``Wv, bv, Wu, bu, w, b`` the tier-1 gated attention; ``Wc, bc`` the tier-1
    classifier; the ``*2`` arguments the same of ``attCls``.  Returns device tensors only and never
    synchronises: ``(sub [G, C], slide [1, C], M [G, L], p1 [G, S], p2 [G])``, then with ``label`` (a GPU
    int64 tensor whose first element the kernel reads; outside ``[0, C)`` both losses are NaN)
    ``(sub_loss [], slide_loss [], Y_prob [1, C], Y_hat [1])``, then with ``return_cam``
    ``(cam [G, S, C],)``.  ``sub``, ``slide`` and the two losses are differentiable."""
    sub, slide, sub_loss, slide_loss, M, p1, p2, yprob, yhat, cam = _pool(
        x, perm, W1, Wv, bv, Wu, bu, w, b, Wc, bc, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, bag_size, max_pseudo_bags,
        label, return_cam)
    out = (sub, slide, M, p1, p2)
    if label is not None:
        out += (sub_loss, slide_loss, yprob, yhat)
    if return_cam:
        out += (cam,)
    return out


def _pool(x, perm, W1, Wv, bv, Wu, bu, w, b, Wc, bc, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, bag_size, max_pseudo_bags,
          label, return_cam):
    """``dtfd_pool``'s checks and node; returns the node's ten outputs (``_DtfdFn``), ``None`` where not asked for."""
    x = _check_bag(x)
    N, S = x.shape[0], int(bag_size)
    L, D, C = W1.shape[0], Wv.shape[0], Wc.shape[0]
    if L != M_DIM or W1.shape[1] != x.shape[1]:
        raise RuntimeError(f"DTFDMIL: m_dim must be {M_DIM} on the HIP path and fc1 must take the bag's width, got "
                           f"fc1.weight {tuple(W1.shape)} for bags {x.shape[1]} wide")
    if not (4 <= D <= MAX_D and D % 4 == 0):
        raise RuntimeError(f"DTFDMIL: D must be a multiple of 4, <= {MAX_D} on the HIP path, got {D}")
    if not 1 <= C <= MAX_CLASSES:
        raise RuntimeError(f"DTFDMIL: n_classes must be in [1, {MAX_CLASSES}] on the HIP path, got {C}")
    if not 1 <= S <= MAX_BAG_SIZE:
        raise RuntimeError(f"DTFDMIL: bag_size must be in [1, {MAX_BAG_SIZE}] on the HIP path, got {S}")
    G = pseudo_bags(N, S, max_pseudo_bags)
    if G < 1:
        raise RuntimeError(f"DTFDMIL: a bag of {N} instances holds no pseudo-bag of bag_size = {S} "
                           "(the reference fails on torch.cat of an empty list)")
    if G > MAX_PSEUDO_BAGS:
        raise RuntimeError(f"DTFDMIL: the number of pseudo-bags must be in [1, {MAX_PSEUDO_BAGS}] on the HIP path, "
                           f"got {G}")
    if not perm.is_cuda or perm.dtype != torch.int64 or perm.dim() != 1 or perm.numel() < G * S:
        raise RuntimeError(f"DTFDMIL: perm must be a 1-D int64 GPU tensor of at least G S = {G * S} row ids")
    if label is not None:
        label = device_label(label, "DTFDMIL")
    idx = perm.detach()[:G * S].contiguous()
    return _DtfdFn.apply(x, idx, W1, Wv, bv, Wu, bu, w, b, Wc, bc, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, label, G, S,
                         bool(return_cam))


_REFUSED = "is not on the MI355X path"


class Attention_Gated(nn.Module):
    """``DTFDMIL.py:14-45``: the parameter container of a gated attention branch (the arithmetic runs
    in ``dtfd_pool``)."""

    def __init__(self, features=512, D=128, K=1):
        super().__init__()
        if K != 1:
            raise NotImplementedError(f"DTFDMIL (HIP): Attention_Gated with K = {K} != 1 {_REFUSED}")
        self.L, self.D, self.K = features, D, K
        self.attention_V = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh())
        self.attention_U = nn.Sequential(nn.Linear(self.L, self.D), nn.Sigmoid())
        self.attention_weights = nn.Linear(self.D, self.K)

    def tensors(self):
        V, U, W = self.attention_V[0], self.attention_U[0], self.attention_weights
        return V.weight, V.bias, U.weight, U.bias, W.weight, W.bias


class Classifier_1fc(nn.Module):
    """``DTFDMIL.py:58-71``."""

    def __init__(self, n_channels, n_classes, droprate=0.0):
        super().__init__()
        if droprate != 0.0:
            raise NotImplementedError(f"DTFDMIL (HIP): Classifier_1fc with droprate = {droprate} != 0 {_REFUSED}")
        self.fc = nn.Linear(n_channels, n_classes)
        self.droprate = droprate


class residual_block(nn.Module):
    """``DTFDMIL.py:74-86``: parameters only; ``DimReduction`` refuses to stack it (``numLayer_Res > 0``)."""

    def __init__(self, nChn=512):
        super().__init__()
        self.block = nn.Sequential(nn.Linear(nChn, nChn, bias=False), nn.ReLU(inplace=True),
                                   nn.Linear(nChn, nChn, bias=False), nn.ReLU(inplace=True))


class DimReduction(nn.Module):
    """``DTFDMIL.py:89-109`` with ``numLayer_Res = 0``: ``Linear(n_channels, m_dim, bias=False)`` + ReLU."""

    def __init__(self, n_channels, m_dim=512, numLayer_Res=0):
        super().__init__()
        if numLayer_Res > 0:
            raise NotImplementedError(f"DTFDMIL (HIP): DimReduction with numLayer_Res = {numLayer_Res} > 0 {_REFUSED}")
        self.fc1 = nn.Linear(n_channels, m_dim, bias=False)
        self.relu1 = nn.ReLU(inplace=True)
        self.numRes = numLayer_Res
        self.resBlocks = nn.Sequential()


class Attention_with_Classifier(nn.Module):
    """``DTFDMIL.py:47-56``: tier 2."""

    def __init__(self, L=512, D=128, K=1, num_cls=2, droprate=0):
        super().__init__()
        self.attention = Attention_Gated(L, D, K)
        self.classifier = Classifier_1fc(L, num_cls, droprate)


class DTFDMIL(nn.Module):
    """The modules ``ModelInterface_DTFD`` builds at ``model_interface_dtfd.py:162-165`` and its
    ``forward`` (:174-224) on feature bags ``in_features`` wide (``self.out_features = 1024``, :110)."""

    def __init__(self, n_classes, in_features=1024, m_dim=512, bag_size=120, max_pseudo_bags=8):
        super().__init__()
        self.classifier = Classifier_1fc(n_channels=m_dim, n_classes=n_classes)
        self.attention = Attention_Gated(features=m_dim)
        self.dimreduction = DimReduction(n_channels=in_features, m_dim=m_dim)
        self.attCls = Attention_with_Classifier(L=m_dim, num_cls=n_classes)
        self.n_classes, self.in_features, self.m_dim = n_classes, in_features, m_dim
        self.bag_size, self.max_pseudo_bags = int(bag_size), int(max_pseudo_bags)

    def group_parameters(self):
        """The two optimizers' parameter lists (:166-169, 596-597)."""
        first = (list(self.classifier.parameters()) + list(self.attention.parameters())
                 + list(self.dimreduction.parameters()))
        return first, list(self.attCls.parameters())

    def _tensors(self):
        return ((self.dimreduction.fc1.weight,) + self.attention.tensors()
                + (self.classifier.fc.weight, self.classifier.fc.bias) + self.attCls.attention.tensors()
                + (self.attCls.classifier.fc.weight, self.attCls.classifier.fc.bias))

    def forward(self, x, bag_size=None, perm=None, label=None, return_cam=False):
        """-> ``(sub_predictions [G, C], slide_prediction [1, C], Y_prob [1, C], Y_hat [1])``; with a
        ``label`` or ``return_cam`` a fifth element, the dict of ``sub_loss`` / ``slide_loss`` (with a
        label), ``cam`` (with ``return_cam``), ``M``, ``p1`` and ``p2``.  ``perm=None`` draws
        ``torch.randperm(N)`` on the CPU default generator (one call, :186); a CPU ``perm`` is checked
        to be a permutation of ``range(N)``; a GPU int64 ``perm`` is taken as it is (no host work)."""
        S = int(self.bag_size if bag_size is None else bag_size)
        N = x.shape[-2] if x.dim() >= 2 else 0
        if N < S:
            raise RuntimeError(f"DTFDMIL: a bag of {N} instances holds no pseudo-bag of bag_size = {S} "
                               "(the reference fails on torch.cat of an empty list)")
        x = _check_bag(x)
        if perm is None:
            perm = torch.randperm(N)
        elif not perm.is_cuda:
            perm = perm.to(torch.int64).reshape(-1)
            if perm.numel() != N or not torch.equal(torch.sort(perm).values, torch.arange(N)):
                raise ValueError(f"DTFDMIL: perm must hold every row id of [0, {N}) once")
        perm = perm.to(x.device)
        dev_label = None
        if label is not None:
            dev_label = torch.as_tensor(label).to(device=x.device, dtype=torch.int64).reshape(-1)
        sub, slide, sub_loss, slide_loss, M, p1, p2, Y_prob, Y_hat, cam = _pool(
            x, perm, *self._tensors(), S, self.max_pseudo_bags, dev_label, return_cam)
        if dev_label is None and not return_cam:
            return sub, slide, Y_prob, Y_hat
        extras = {"M": M, "p1": p1, "p2": p2}
        if dev_label is not None:
            extras.update(sub_loss=sub_loss, slide_loss=slide_loss)
        if return_cam:
            extras["cam"] = cam
        return sub, slide, Y_prob, Y_hat, extras


class DTFDTask:
    """``ModelInterface_DTFD``'s steps and optimizers without Lightning (:227-279, 313-341, 594-601)."""

    def __init__(self, model):
        self.model = model
        self.n_classes = model.n_classes

    def _class_index(self, label, device):
        """A class index, or a one-hot row reduced by argmax (:244), as a device int64 [1]."""
        label = torch.as_tensor(label).to(device)
        if label.numel() > 1:
            label = torch.argmax(label.reshape(-1))
        return label.to(torch.int64).reshape(1)

    def training_step(self, batch, optimizer_idx=0):
        x, label = batch[0], batch[1]
        Y = self._class_index(label, x.device)
        _, _, Y_prob, Y_hat, extras = self.model(x, label=Y)
        total = (extras["sub_loss"] + extras["slide_loss"]) / 2
        return {"loss": total, "Y_prob": Y_prob.detach(), "Y_hat": Y_hat.detach(), "label": Y[0]}

    def validation_step(self, batch):
        x, label = batch[0], batch[1]
        Y = self._class_index(label, x.device)
        with torch.no_grad():
            _, slide, Y_prob, Y_hat, extras = self.model(x, label=Y)
        return {"val_sub_loss": extras["sub_loss"], "val_slide_loss": extras["slide_loss"], "logits": slide,
                "Y_prob": Y_prob, "Y_hat": Y_hat, "label": Y[0]}

    def configure_optimizers(self):
        first, second = self.model.group_parameters()
        optimizer0 = torch.optim.Adam(first, lr=1e-4, weight_decay=1e-2)
        optimizer1 = torch.optim.Adam(second, lr=1e-4, weight_decay=1e-2)
        scheduler0 = torch.optim.lr_scheduler.MultiStepLR(optimizer0, [100], gamma=0.2)
        scheduler1 = torch.optim.lr_scheduler.MultiStepLR(optimizer1, [100], gamma=0.2)
        return [optimizer0, optimizer1], [scheduler0, scheduler1]

    def optimization_step(self, batch, optimizers):
        """One batch of Lightning 1.x automatic optimization with two optimizers: per optimizer a fresh
        forward (a fresh ``randperm``) with the other group's ``requires_grad`` off (``toggle_optimizer``),
        the backward of ``total``, that optimizer's step and ``zero_grad(set_to_none=True)``.  Returns the
        two ``training_step`` dicts."""
        groups = self.model.group_parameters()
        outs = []
        for i, opt in enumerate(optimizers):
            other = groups[1 - i]
            flags = [p.requires_grad for p in other]
            for p in other:
                p.requires_grad_(False)
            try:
                out = self.training_step(batch, i)
                out["loss"].backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
            finally:
                for p, f in zip(other, flags):
                    p.requires_grad_(f)
            outs.append(out)
        return outs
