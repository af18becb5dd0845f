"""Plain fp64 PyTorch restatements of the bf16 step's backward kernels (helpers of
test_backward_fused_gpu.py; test_kernel_refs_cpu.py checks them against autograd), and the host
restatement of the kernels' dropout hash.  Not a conftest: imported by name."""
import numpy as np
import torch

NL, DH, TAPS, HALF = 256, 64, 33, 16


# ----------------------------------------------------------------------------- dropout hash
def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h = (h * np.uint32(0x85EBCA6B)).astype(np.uint32)
    h ^= h >> np.uint32(13)
    h = (h * np.uint32(0xC2B2AE35)).astype(np.uint32)
    h ^= h >> np.uint32(16)
    return h


def dropout_keep(seed_dev_value, layer_seed, rows, cols, p):
    """Host restatement of common.h dropout_u01 / effective_seed (the kernels' hash): keep[row][col]
    for rows 0..rows-1.  The kernels compare the 24-bit uniform with the fp32 value of p."""
    seed = (int(seed_dev_value) * 0x9E3779B97F4A7C15 + int(layer_seed)) & (2 ** 64 - 1)
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    r = np.arange(rows, dtype=np.uint32)[:, None]
    c = np.arange(cols, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        h = _mix32(lo ^ _mix32((r * np.uint32(0x9E3779B1) + hi).astype(np.uint32)))
        h = _mix32(h ^ (c * np.uint32(0x7FEB352D)).astype(np.uint32))
    u = (h >> np.uint32(8)).astype(np.float64) / 16777216.0
    return u >= np.float64(np.float32(p))


def drop_scale_f32(p):
    """1 / (1 - p) as the entry points compute it (fp32)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)


# ----------------------------------------------------------------------------- layouts
def heads_to_cols(x, nh):
    """[B*nh, n, 64] -> [B, n, nh*64] (the column block of one of q / k / v in dqkv, or merged)."""
    nbh, n, dh = x.shape
    return x.view(nbh // nh, nh, n, dh).permute(0, 2, 1, 3).reshape(nbh // nh, n, nh * dh)


# ----------------------------------------------------------------------------- A3 backward
def a3_bwd_ref(ql, dw, k, v):
    """fp64: A = softmax(ql k^T) over the keys; dS = A (dw v^T - rowsum(dw o A v)); returns
    (lse, D, dk = dS^T ql, dv = A^T dw, dql = dS k): the backward of W = A v (SURVEY App. A eq. 3/9).
    One head at a time (the [256, n] matrices of 16 heads x 8448 keys do not have to coexist)."""
    ql, dw, k, v = (t.double() for t in (ql, dw, k, v))
    lse, d, dk, dv, dql = [], [], [], [], []
    for h in range(ql.shape[0]):
        s = ql[h] @ k[h].t()
        ls = torch.logsumexp(s, -1)
        a = torch.exp(s - ls[:, None])
        dd = (dw[h] * (a @ v[h])).sum(-1)
        ds = a * (dw[h] @ v[h].t() - dd[:, None])
        lse.append(ls)
        d.append(dd)
        dk.append(ds.t() @ ql[h])
        dv.append(a.t() @ dw[h])
        dql.append(ds @ k[h])
    return tuple(torch.stack(t) for t in (lse, d, dk, dv, dql))


def a3_fwd_ref(ql, k, v):
    """fp64 W = softmax(ql k^T) v, [B*nh, 256, 64], one head at a time."""
    ql, k, v = (t.double() for t in (ql, k, v))
    return torch.stack([torch.softmax(ql[h] @ k[h].t(), -1) @ v[h] for h in range(ql.shape[0])])


def a3_bwd_fused_ref(ql, dw, k, v, dv_conv, dv_lo, dv_hi, dkl, nh, base=None):
    """tm_nys_a3_bwd_fused in fp64: (k_cols, v_cols [B][n][nh*64], dql [B*nh][256][64]) with
    k_cols[b][t][h*64+d] = dK + dkl[bh][t // l] / l and v_cols = dV + (dv_conv[t] if dv_lo <= t <
    dv_hi else 0).  dv_conv outside the window is never read (it may be NaN).  ``base``: the
    a3_bwd_ref(ql, dw, k, v) tuple when the caller already has it."""
    n = k.shape[1]
    l = n // NL
    _, _, dk, dv, dql = a3_bwd_ref(ql, dw, k, v) if base is None else base
    kc = dk + dkl.double().repeat_interleave(l, dim=1) / l
    win = torch.zeros_like(dv)
    win[:, dv_lo:dv_hi] = dv_conv.double()[:, dv_lo:dv_hi]
    return heads_to_cols(kc, nh), heads_to_cols(dv + win, nh), dql


def slab_sum_f32(slabs, par=1):
    """The fp32 sum of [p][...] partial slabs as the flush launch orders it (gemm.hip
    multi_reduce_kernel): lane `sub` of `par` adds slabs sub, sub + par, ... in index order, then
    the lanes combine through an xor tree; par = 1 is the plain index-order sum."""
    x = slabs.float()
    parts = []
    for sub in range(par):
        s = torch.zeros_like(x[0])
        for z in range(sub, x.shape[0], par):
            s = s + x[z]
        parts.append(s)
    o = 1
    while o < par:
        parts = [parts[i] + parts[i ^ o] for i in range(par)]
        o <<= 1
    return parts[0]


def reduce_par(splits, count, bf16=True):
    """Lanes per output unit of the flush launch (gemm.hip push_reduce_entry, 16-B aligned slabs)."""
    units = count // 8 if bf16 and count % 8 == 0 else count // 4 if count % 4 == 0 else count
    par = 1
    while par < 64 and (splits + par - 1) // par > 24 and units * par * 2 <= 65536:
        par <<= 1
    return par


def assemble_q_ref(dq, dq_row, dql_total, nh, scale):
    """q part of dqkv: scale * (dq + dql_total[t // l] / l), dq zero outside row dq_row when
    dq_row >= 0; dql_total = dql + the sum of the A3 backward's slabs.  [B][n][nh*64] fp64."""
    dqd = dq.double()
    n = dqd.shape[1]
    l = n // NL
    if dq_row >= 0:
        keep = torch.zeros_like(dqd)
        keep[:, dq_row] = dqd[:, dq_row]
        dqd = keep
    return heads_to_cols(scale * (dqd + dql_total.double().repeat_interleave(l, dim=1) / l), nh)


# ----------------------------------------------------------------------------- class row (clsrow.hip)
def cls_a1_row_ref(q, v, kl, y, wconv, nh, r):
    """Row r of merged = softmax(q kl^T) y + conv33(v) for every bag: (merged_row [B, nh*64],
    lse_row [B*nh]); q / v [B*nh, n, 64], kl / y [B*nh, 256, 64], wconv [nh, 33].  Differentiable."""
    q, v, kl, y, wconv = (t.double() for t in (q, v, kl, y, wconv))
    nbh, n, dh = q.shape
    s = torch.einsum("hd,hjd->hj", q[:, r], kl)
    lse = torch.logsumexp(s, -1)
    o = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), y)
    w = wconv.view(nh, TAPS)[torch.arange(nbh) % nh]
    for tau in range(TAPS):
        t = r + tau - HALF
        if 0 <= t < n:
            o = o + w[:, tau, None] * v[:, t]
    return o.reshape(nbh // nh, nh * dh), lse


def cls_a1_row_bwd_ref(dmerged, q, v, kl, y, wconv, nh, r):
    """fp64 autograd through cls_a1_row_ref with the upstream row gradient dmerged [B, nh*64]:
    (dq_row [B*nh, 64], dkl, dy [B*nh, 256, 64], dv_window [B*nh, hi - lo, 64], dwconv [nh, 33]),
    the window rows [lo, hi) = [max(r-16, 0), min(r+17, n))."""
    ins = [t.double().detach().clone().requires_grad_() for t in (q, v, kl, y, wconv)]
    m, _ = cls_a1_row_ref(*ins, nh, r)
    gq, gv, gkl, gy, gw = torch.autograd.grad(m, ins, dmerged.double())
    n = q.shape[1]
    lo, hi = max(r - HALF, 0), min(r + HALF + 1, n)
    return gq[:, r], gkl, gy, gv[:, lo:hi], gw.view(nh, TAPS)


# ----------------------------------------------------------------------------- LayerNorm backward
def ln_bwd_seg_ref(dy, x, gamma, mean, rstd, S, pad, dx_accum, resid_cls_only, seg=None, seg_len=1, nseg=0):
    """tm_layernorm_bwd / tm_layernorm_bwd_seg in fp64: dy [B, n_pad, D] (row pad + t of bag b is
    token t), x / dx_accum [B*S, D], mean / rstd [B*S]; with seg [B, seg_rows, D]:
    dy_eff[b][t] = dy[b][pad+t] + seg[b][(pad+t)//seg_len] + (t==0)*seg[b][nseg].  Returns (dx, dgamma,
    dbeta), dx = LN'(dy_eff) + dx_accum, of which only the class rows (t = 0) are read (the others
    count as zero, whatever they hold) when resid_cls_only."""
    B, _, D = dy.shape
    g = dy[:, pad:pad + S].double()
    if seg is not None:
        idx = (pad + torch.arange(S)) // seg_len
        g = g + seg.double()[:, idx]
        g[:, 0] = g[:, 0] + seg.double()[:, nseg]
    xh = ((x.double() - mean.double()[:, None]) * rstd.double()[:, None]).view(B, S, D)
    dgamma = (g * xh).sum((0, 1))
    dbeta = g.sum((0, 1))
    gg = g * gamma.double()
    s1 = gg.mean(-1, keepdim=True)
    s2 = (gg * xh).mean(-1, keepdim=True)
    dx = rstd.double().view(B, S, 1) * (gg - s1 - xh * s2)
    acc = dx_accum.double().view(B, S, D)
    if resid_cls_only:
        dx[:, 0] = dx[:, 0] + acc[:, 0]
    else:
        dx = dx + acc
    return dx.reshape(B * S, D), dgamma, dbeta
