"""Torch restatement of the reference Chowder (code/models/Chowder.py:19-50), for fp32 and fp64
CPU runs, plus the helpers the Chowder fixtures and tests share.

The model below is the reference's op sequence (transpose, ``Conv1d(L, 1, 1)``, two ``topk``, ``cat``,
three ``Linear``, ``squeeze(0)``) without its ``x.float()``, so that it also runs in fp64.  It keeps
the reference's parameter names, so a state dict moves between the two with ``strict=True``.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn


class ChowderRef(nn.Module):
    def __init__(self, n_classes, features=512, r=5):
        super().__init__()
        self.L, self.n_classes, self.R = features, n_classes, r
        self.f1 = nn.Sequential(nn.Conv1d(self.L, 1, 1))
        self.f2 = nn.Sequential(nn.Linear(r * 2, 200), nn.Linear(200, 100), nn.Linear(100, self.n_classes))

    def scores(self, x):
        """[B, N, L] -> [B, 1, N]: the Conv1d on the transposed bag (:40-42)."""
        return self.f1(torch.transpose(x, 1, 2))

    def forward(self, x):
        s = self.scores(x)
        top = torch.topk(s, self.R).values
        bottom = torch.topk(s, self.R, largest=False).values
        cat_minmax = torch.cat((bottom, top), dim=2)
        return self.f2(cat_minmax).squeeze(0), None


def select(s, r):
    """The contract's selection of a [B, N] score array (numpy): ``idx [B, 2r]`` = the r smallest
    ascending, then the r largest descending, among equal scores the lower index first."""
    n = s.shape[1]
    order = np.arange(n)
    out = np.empty((s.shape[0], 2 * r), dtype=np.int64)
    for b in range(s.shape[0]):
        lo = np.lexsort((order, s[b]))[:r]
        hi = np.lexsort((order, -s[b]))[:r]
        out[b] = np.concatenate([lo, hi])
    return out


def rounding_bound(x, w, bias):
    """E[b, n] = L 2^-24 (sum_i |x_i w_i| + |bias|): a bound on |fl(x . w + bias) - exact| that holds for
    every fp32 summation order of the row (each of at most L additions and multiplications rounds
    once, relative 2^-24, and partial sums are bounded by the sum of magnitudes; second-order terms
    are far below the slack).  x [B, N, L], w [L], bias scalar; fp64 numpy in, [B, N] out."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    L = x.shape[-1]
    return L * 2.0 ** -24 * (np.abs(x * w).sum(-1) + abs(float(bias)))


def extreme_gap(s, r):
    """Smallest fp64 gap between neighbouring scores among the r + 1 smallest and among the r + 1
    largest scores of every bag (all of them when N <= r).  s [B, N]."""
    gap = np.inf
    for row in np.asarray(s, dtype=np.float64):
        srt = np.sort(row)
        k = min(r + 1, srt.size)
        for part in (srt[:k], srt[-k:]):
            if part.size > 1:
                gap = min(gap, float(np.diff(part).min()))
    return gap


def case_input(shape, seed):
    """Uniform [0, 1) fp32 input from numpy PCG64(seed)."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def bf16_round(a):
    """fp32 numpy -> the same values rounded to bf16 (round to nearest even), as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def fixture_cases():
    """The case table of tests/golden/make_golden_chowder.py: name -> (B, N, L, R, classes, bf16)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_chowder.py")
    spec = importlib.util.spec_from_file_location("make_golden_chowder", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return dict(mod.CASES)
