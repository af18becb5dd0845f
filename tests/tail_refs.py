"""Plain fp64 PyTorch restatements of the LayerNorm forward, the class-token head, the fused
cross-entropy, the PPEG fold and the GELU derivative (helpers of test_tail_kernels_gpu.py;
test_tail_refs_cpu.py checks them against autograd and the oracle PPEG).  No library code is
imported.  Not a conftest: imported by name."""
import math

import torch


# ----------------------------------------------------------------------------- LayerNorm forward
def ln_fwd_ref(x, gamma, beta, eps, S, n_pad, pad):
    """tm_layernorm_fwd in fp64: x [B*S, D] -> (y [B, n_pad, D], mean [B*S], rstd [B*S]).  Row pad + t
    of bag b is token t, rows 0..pad-1 are zero and rows pad + S.. (which the kernel leaves alone)
    are NaN."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    rows, D = x.shape
    B = rows // S
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = torch.full((B, n_pad, D), float("nan"), dtype=torch.float64)
    y[:, :pad] = 0.0
    y[:, pad:pad + S] = (((x - mean[:, None]) * rstd[:, None]) * gamma + beta).view(B, S, D)
    return y, mean, rstd


# ----------------------------------------------------------------------------- head
def head_ref(h, S, gamma, beta, eps, W, bias):
    """tm_head_fwd in fp64: h [B*S, D] (only row 0 of every bag is read) -> (logits [B, C] =
    LN(h[b*S]) W^T + bias, xhat [B, D], rstd [B])."""
    D = h.shape[-1]
    x = h.reshape(-1, S, D)[:, 0].double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1) + eps)
    xhat = (x - mean) * rstd[:, None]
    y = xhat * gamma.double() + beta.double()
    return y @ W.double().t() + bias.double(), xhat, rstd


def head_bwd_ref(dlogits, xhat, rstd, gamma, beta, W):
    """tm_head_bwd in fp64: (dW [C, D], dbias [C], dgamma [D], dbeta [D], dh_row0 [B, D]) from the
    forward's xhat / rstd:  y = xhat gamma + beta, dy = dlogits W,
    dh = rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat))."""
    dl, xhat, rstd, gamma, beta, W = (t.double() for t in (dlogits, xhat, rstd, gamma, beta, W))
    y = xhat * gamma + beta
    dW = dl.t() @ y
    dbias = dl.sum(0)
    dy = dl @ W
    dgamma = (dy * xhat).sum(0)
    dbeta = dy.sum(0)
    g = dy * gamma
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xhat).mean(-1, keepdim=True)
    dh = rstd[:, None] * (g - s1 - xhat * s2)
    return dW, dbias, dgamma, dbeta, dh


# ----------------------------------------------------------------------------- cross-entropy
def ce_ref(logits, label):
    """tm_ce_fwd in fp64: (loss = mean_b(logsumexp(l_b) - l_b[label_b]), prob = softmax, yhat = the
    FIRST index of the row maximum, stats_delta int32 [C, 2] = per-class (count, correct)).  A label
    outside [0, C) makes the loss NaN and is left out of stats_delta."""
    l = logits.double()
    B, C = l.shape
    m = l.max(-1, keepdim=True).values
    e = torch.exp(l - m)
    s = e.sum(-1, keepdim=True)
    prob = e / s
    lse = (m + torch.log(s))[:, 0]
    idx = torch.arange(C).expand(B, C)
    yhat = torch.where(l == m, idx, torch.full_like(idx, C)).min(-1).values
    terms = torch.full((B,), float("nan"), dtype=torch.float64)
    stats = torch.zeros(C, 2, dtype=torch.int32)
    for b, y in enumerate(label.tolist()):
        if 0 <= y < C:
            terms[b] = lse[b] - l[b, y]
            stats[y, 0] += 1
            stats[y, 1] += int(yhat[b].item() == y)
    return terms.sum() / B, prob, yhat, stats


def ce_dlogits_ref(prob, label, g, dlogits_in):
    """tm_ce_bwd / the first step of tm_head_ce_bwd in fp64: g (prob - one_hot(label)) / B
    (+ dlogits_in when it is not None)."""
    p = prob.double()
    B, C = p.shape
    onehot = torch.zeros(B, C, dtype=torch.float64)
    onehot[torch.arange(B), label] = 1.0
    d = float(g) * (p - onehot) / B
    return d if dlogits_in is None else d + dlogits_in.double()


# ----------------------------------------------------------------------------- PPEG fold
def ppeg_fold_ref(w7, b7, w5, b5, w3, b3):
    """tm_ppeg_fold / the fold of tm_step_prepare in fp64: the depthwise 7x7 + 5x5 + 3x3 + identity
    of PPEG as ONE 7x7 kernel, (wf [49, D] tap-major, bf [D]); w7 [D, 49] (or [D, 1, 7, 7]), w5
    [D, 25], w3 [D, 9].  The 5x5 sits at taps 1..5, the 3x3 at 2..4, the identity at (3, 3)."""
    D = w7.shape[0]
    k = w7.double().reshape(D, 7, 7).clone()
    k[:, 1:6, 1:6] += w5.double().reshape(D, 5, 5)
    k[:, 2:5, 2:5] += w3.double().reshape(D, 3, 3)
    k[:, 3, 3] += 1.0
    return k.reshape(D, 49).t().contiguous(), b7.double() + b5.double() + b3.double()


# ----------------------------------------------------------------------------- GELU
def gelu_grad_ref(x):
    """d/dx of the erf GELU x Phi(x) in fp64: Phi(x) + x phi(x)."""
    x = x.double()
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf
