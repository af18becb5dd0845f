"""Torch restatement of the reference ``CLAM_MB`` (code/models/model_clam.py:195-268) for fp32 and
fp64 CPU runs, plus the helpers the CLAM fixtures and tests share.

``ClamMBRef`` is the reference's op sequence (``Linear`` + ``ReLU``, the gated attention branch, the
softmax over the instances, ``mm``, one ``Linear(L, 1)`` per class; for the instance evaluation
``index_select``, the class's instance classifier and the mean cross entropy) with the reference's
parameter names, so a state dict moves between the two with ``strict=True``.  Two differences, both
of the contract: it exposes the raw scores, and it takes the instance selection from the
``(score, index)`` order of the raw scores (``select``) instead of ``topk`` of the softmaxed ones
(the softmax is monotone; ``topk`` leaves the order of equal scores open).
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SIZES = {"small": [1024, 512, 256], "big": [1024, 512, 384]}


class _Gated(nn.Module):
    def __init__(self, L, D, n_classes):
        super().__init__()
        self.attention_a = nn.Sequential(nn.Linear(L, D), nn.Tanh())
        self.attention_b = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
        self.attention_c = nn.Linear(D, n_classes)

    def forward(self, x):
        return self.attention_c(self.attention_a(x).mul(self.attention_b(x))), x


def select(a, label, k, subtyping):
    """The contract's selection from raw scores ``a [K, N]`` (numpy): ``idx [K, 2k]`` int64.  Row
    ``label``: the k largest in descending order, then the k smallest in ascending order; with
    ``subtyping`` every other row: its k largest, then -1; otherwise -1.  Among equal scores the lower
    index comes first on both sides."""
    K, N = a.shape
    order = np.arange(N)
    out = np.full((K, 2 * k), -1, dtype=np.int64)
    for c in range(K):
        if c != label and not subtyping:
            continue
        out[c, :k] = np.lexsort((order, -a[c]))[:k]
        if c == label:
            out[c, k:] = np.lexsort((order, a[c]))[:k]
    return out


def targets_of(idx, label, k):
    """``inst_targets [K, 2k]``: 1 for the in-class largest, 0 for every other selected slot, -1 where
    nothing is selected."""
    t = np.where(idx >= 0, 0, -1).astype(np.int64)
    if 0 <= label < idx.shape[0]:
        t[label, :k] = 1
    return t


def extreme_gap(a, label, k, subtyping):
    """Smallest fp64 gap between neighbouring scores among the k + 1 extremes of every evaluated
    class and side (all N where N <= k)."""
    gap = np.inf
    for c, row in enumerate(np.asarray(a, dtype=np.float64)):
        if c != label and not subtyping:
            continue
        srt = np.sort(row)
        n = min(k + 1, srt.size)
        parts = [srt[-n:]] + ([srt[:n]] if c == label else [])
        for part in parts:
            if part.size > 1:
                gap = min(gap, float(np.diff(part).min()))
    return gap


class ClamMBRef(nn.Module):
    def __init__(self, gate=True, size_arg="small", dropout=False, k_sample=8, n_classes=2, subtyping=False):
        super().__init__()
        assert gate and not dropout
        size = SIZES[size_arg]
        self.attention_net = nn.Sequential(nn.Linear(size[0], size[1]), nn.ReLU(), _Gated(size[1], size[2], n_classes))
        self.classifiers = nn.ModuleList([nn.Linear(size[1], 1) for _ in range(n_classes)])
        self.instance_classifiers = nn.ModuleList([nn.Linear(size[1], 2) for _ in range(n_classes)])
        self.k_sample, self.n_classes, self.subtyping = k_sample, n_classes, subtyping

    def scores(self, x):
        """x [N, 1024] -> (A_raw [K, N], h [N, L])."""
        A, h = self.attention_net(x)
        return torch.transpose(A, 1, 0), h

    def forward(self, x, label=None, instance_eval=False):
        """-> dict(logits [1, K], A_raw, M, instance_loss, idx / inst_preds / inst_targets [K, 2k] numpy)."""
        A_raw, h = self.scores(x)
        A = F.softmax(A_raw, dim=1)
        out = {}
        if instance_eval:
            k, y = self.k_sample, int(label)
            idx = select(A_raw.detach().double().numpy(), y, k, self.subtyping)
            targets = targets_of(idx, y, k)
            preds = np.full_like(idx, -1)
            total = 0.0
            for c in range(self.n_classes):
                on = idx[c] >= 0
                if not on.any():
                    continue
                rows = torch.index_select(h, 0, torch.from_numpy(idx[c][on]))
                il = self.instance_classifiers[c](rows)
                total = total + F.cross_entropy(il, torch.from_numpy(targets[c][on]))
                preds[c][on] = torch.topk(il, 1, dim=1)[1].squeeze(1).numpy()
            if self.subtyping:
                total = total / self.n_classes
            out.update(instance_loss=total, idx=idx, inst_preds=preds, inst_targets=targets)
        M = torch.mm(A, h)
        logits = torch.stack([self.classifiers[c](M[c]) for c in range(self.n_classes)], dim=1)
        out.update(logits=logits, A_raw=A_raw, M=M)
        return out


def case_params_(model, name):
    """The fixtures' weights: ``deterministic_params_(seed=2021)``; the ``peaky`` case then scales
    ``attention_c.weight`` by 40 and sets ``attention_c.bias = [+95, -95]``: its scores lie near +-95,
    where an exp without the max shift overflows fp32, while the softmax inside a class stays soft."""
    from oracle.transmil_ref import deterministic_params_
    deterministic_params_(model, 2021)
    if name.endswith("peaky"):
        c = model.attention_net[2].attention_c
        with torch.no_grad():
            c.weight.mul_(40.0)
            c.bias.copy_(torch.tensor([95.0, -95.0], dtype=c.bias.dtype))
    return model


def case_input(N, seed):
    """Uniform [0, 1) fp32 bag [N, 1024] from numpy PCG64(seed)."""
    return np.random.default_rng(seed).random((N, 1024), dtype=np.float32)


def ref_model(name, case, dtype=torch.float64):
    K, N, size, k, subtyping, label = case
    return case_params_(ClamMBRef(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping), name).to(dtype).eval()


def fixture_cases():
    """The case table of tests/golden/make_golden_clam.py: name -> (K, N, size, k_sample, subtyping, label)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_clam.py")
    spec = importlib.util.spec_from_file_location("make_golden_clam", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return dict(mod.CASES)
