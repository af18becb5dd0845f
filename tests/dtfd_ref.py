"""Torch restatement of the reference's DTFD-MIL (``ModelInterface_DTFD.forward`` and its training step,
code/models/model_interface_dtfd.py:174-279, 594-601, on the blocks of code/models/DTFDMIL.py) for fp32
and fp64 CPU runs, plus the case table and the helpers the DTFD fixtures and tests share.

``DtfdRef`` is the reference's op sequence (``Linear`` + ``ReLU`` over all N rows, per pseudo-bag the
index by the permutation's slice, the gated attention, ``softmax``, the ``einsum`` weighting, the sum,
``Classifier_1fc`` and ``get_cam_1d``; then ``Attention_with_Classifier``) with the reference's
parameter names, so a state dict moves between the two with ``strict=True``.  Two differences, both of
the contract: the permutation is an argument (the reference draws it inside), and the pooled rows, the
two softmaxes and the CAMs are returned (the reference drops them).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

IN_FEATURES = 1024

# name -> (C, N, S = bag_size, cap = max_pseudo_bags, label)
CASES = {
    "dtfd_n1_s1": (2, 1, 1, 8, 1),                    # both softmaxes over one element
    "dtfd_n120_s120": (2, 120, 120, 8, 0),            # G = 1
    "dtfd_n239_s120": (2, 239, 120, 8, 1),            # 119 rows unused
    "dtfd_n30_s7": (2, 30, 7, 8, 0),                  # G = 4, S under a wave, 2 rows unused
    "dtfd_n130_s65_c5": (5, 130, 65, 8, 3),           # one row past a wave
    "dtfd_n600_s257": (2, 600, 257, 8, 1),            # past 256
    "dtfd_n960_s120_c3": (3, 960, 120, 8, 2),         # G = 8
    "dtfd_n2000_s120": (2, 2000, 120, 8, 0),          # the cap bites, 1040 rows unused
    "dtfd_n2048_s32_g64": (2, 2048, 32, 64, 1),       # non-default cap
    "dtfd_n960_s120_peaky": (2, 960, 120, 8, 1),      # tier-1 scores near +-90 (case_params_)
}

LOGIT_SCALE = 32.0
PEAKY_V_SCALE, PEAKY_W_SCALE = 20.0, 250.0


class _Gated(nn.Module):
    def __init__(self, L=512, D=128, K=1):
        super().__init__()
        self.attention_V = nn.Sequential(nn.Linear(L, D), nn.Tanh())
        self.attention_U = nn.Sequential(nn.Linear(L, D), nn.Sigmoid())
        self.attention_weights = nn.Linear(D, K)

    def forward(self, x):
        """x [n, L] -> the raw scores [K, n]."""
        return torch.transpose(self.attention_weights(self.attention_V(x) * self.attention_U(x)), 1, 0)


class _Classifier(nn.Module):
    def __init__(self, L, C):
        super().__init__()
        self.fc = nn.Linear(L, C)

    def forward(self, x):
        return self.fc(x)


class _DimReduction(nn.Module):
    def __init__(self, n_channels, m_dim):
        super().__init__()
        self.fc1 = nn.Linear(n_channels, m_dim, bias=False)

    def forward(self, x):
        return F.relu(self.fc1(x))


class _AttCls(nn.Module):
    def __init__(self, L, C):
        super().__init__()
        self.attention = _Gated(L)
        self.classifier = _Classifier(L, C)


class DtfdRef(nn.Module):
    def __init__(self, n_classes, in_features=IN_FEATURES, m_dim=512):
        super().__init__()
        self.classifier = _Classifier(m_dim, n_classes)
        self.attention = _Gated(m_dim)
        self.dimreduction = _DimReduction(in_features, m_dim)
        self.attCls = _AttCls(m_dim, n_classes)

    def group_parameters(self):
        first = (list(self.classifier.parameters()) + list(self.attention.parameters())
                 + list(self.dimreduction.parameters()))
        return first, list(self.attCls.parameters())

    def forward(self, x, perm, bag_size, cap=8, label=None):
        """x [N, F], perm int64 [N] -> dict(sub [G, C], slide [1, C], M [G, L], p1 [G, S], p2 [G], a1 [G, S]
        (the raw tier-1 scores), cam [G, S, C]; with ``label`` (an int) sub_loss, slide_loss, total)."""
        S = int(bag_size)
        G = min(int(cap), x.shape[0] // S)
        f = self.dimreduction(x)
        Ms, subs, p1s, a1s, cams = [], [], [], [], []
        for g in range(G):
            bag = f[perm[S * g:S * (g + 1)]]
            a = self.attention(bag)
            p = F.softmax(a, dim=1).squeeze(0)
            att = torch.einsum("ns,n->ns", bag, p)
            Mg = torch.sum(att, dim=0).unsqueeze(0)
            subs.append(self.classifier(Mg))
            cams.append(torch.einsum("gf,cf->gc", att, self.classifier.fc.weight))
            Ms.append(Mg)
            p1s.append(p)
            a1s.append(a.squeeze(0))
        M, sub = torch.cat(Ms, dim=0), torch.cat(subs, dim=0)
        p2 = F.softmax(self.attCls.attention(M), dim=1)
        slide = self.attCls.classifier(torch.mm(p2, M))
        out = dict(sub=sub, slide=slide, M=M, p1=torch.stack(p1s), p2=p2.squeeze(0), a1=torch.stack(a1s),
                   cam=torch.stack(cams))
        if label is not None:
            y = torch.tensor([int(label)])
            out["sub_loss"] = F.cross_entropy(sub, y.repeat(G))
            out["slide_loss"] = F.cross_entropy(slide, y)
            out["total"] = (out["sub_loss"] + out["slide_loss"]) / 2
        return out


def optimizers_for(model):
    """The reference's two Adam optimizers (:594-601)."""
    first, second = model.group_parameters()
    return [torch.optim.Adam(first, lr=1e-4, weight_decay=1e-2), torch.optim.Adam(second, lr=1e-4, weight_decay=1e-2)]


def optimization_step(model, x, label, perms, bag_size, cap, optimizers):
    """One batch of Lightning 1.x automatic optimization on the restatement: per optimizer a forward on
    ``perms[i]`` with the other group's ``requires_grad`` off, the backward of ``total``, the step and
    ``zero_grad``.  Returns the two totals."""
    groups = model.group_parameters()
    totals = []
    for i, opt in enumerate(optimizers):
        other = groups[1 - i]
        for p in other:
            p.requires_grad_(False)
        out = model(x, perms[i], bag_size, cap, label)
        out["total"].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        for p in other:
            p.requires_grad_(True)
        totals.append(float(out["total"].detach()))
    return totals


def case_params_(model, name):
    """The fixtures' weights: ``deterministic_params_(seed=2021)``, then both classifiers' weights times 32
    (with the default scale the logits are 0.1-0.3, and an absolute bar on them would be weak; so
    max |logits| >= 1 in every case).  The ``peaky`` case also scales ``attention.attention_V`` by 20
    (the tanh saturates) and ``attention.attention_weights.weight`` by 250: its tier-1 scores reach about
    +-90, where an exp without the max shift overflows fp32."""
    from oracle.transmil_ref import deterministic_params_
    deterministic_params_(model, 2021)
    with torch.no_grad():
        model.classifier.fc.weight.mul_(LOGIT_SCALE)
        model.attCls.classifier.fc.weight.mul_(LOGIT_SCALE)
        if name.endswith("peaky"):
            model.attention.attention_V[0].weight.mul_(PEAKY_V_SCALE)
            model.attention.attention_weights.weight.mul_(PEAKY_W_SCALE)
    return model


def case_input(N, seed):
    """Uniform [0, 1) fp32 bag [N, 1024] from numpy PCG64(seed)."""
    return np.random.default_rng(seed).random((N, IN_FEATURES), dtype=np.float32)


def case_perm(N, seed):
    """``torch.randperm(N)`` right after ``torch.manual_seed(seed)``: the reference's draw (:186)."""
    torch.manual_seed(seed)
    return torch.randperm(N)


def ref_model(name, dtype=torch.float64):
    return case_params_(DtfdRef(CASES[name][0]), name).to(dtype).eval()
