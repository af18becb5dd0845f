"""Restatement of exact softmax attention (code/models/_transformer.py:33-43) and of its backward as
the attention kernels compute it (transmil_deepgraft_amd/csrc/attention.hip), on CPU tensors.

q, k, v, dout: [B, H, n, dh].  ``dtype=torch.float64`` is the reference of the kernel tests;
``dtype=torch.float32`` is the plain fp32 torch evaluation of the same formulas, whose own error
against fp64 scales the fp32 bounds where the scores' fp32 resolution sets the error."""
import torch


def attn_fwd(q, k, v, scale, dtype=torch.float64):
    """out = softmax(q k^T scale) v  [B, H, n, dh],  lse = log sum_j exp(scale q.k_j)  [B, H, n]."""
    q, k, v = (t.to(dtype) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    out = (e / l) @ v
    return out, (m + torch.log(l)).squeeze(-1)


def attn_bwd(q, k, v, out, lse, dout, scale, dtype=torch.float64):
    """D = rowsum(dO o O), P = exp(S - lse), dV = P^T dO, dS = P o (dO V^T - D), dQ = scale dS K,
    dK = scale dS^T Q."""
    q, k, v, out, lse, dout = (t.to(dtype) for t in (q, k, v, out, lse, dout))
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse[..., None])
    d = (dout * out).sum(dim=-1, keepdim=True)
    dv = p.transpose(-1, -2) @ dout
    ds = p * (dout @ v.transpose(-1, -2) - d)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(-1, -2) @ q)
    return dq, dk, dv


def attn_plain(q, k, v, scale):
    """The model's formula, for autograd: softmax(q k^T scale) v."""
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v


def pack_qkv(q, k, v):
    """[B, H, n, dh] x 3 -> the packed to_qkv layout [B, n, 3*H*dh] (which-major, then head)."""
    B, H, n, dh = q.shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B, n, H * dh) for t in (q, k, v)], dim=-1).contiguous()


def unpack_qkv(x, H):
    """[B, n, 3*H*dh] -> three [B, H, n, dh]."""
    B, n, w = x.shape
    dh = w // (3 * H)
    return tuple(t.reshape(B, n, H, dh).permute(0, 2, 1, 3) for t in x.chunk(3, dim=-1))


def merge_heads(t):
    """[B, H, n, dh] -> [B, n, H*dh]."""
    B, H, n, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * dh).contiguous()


def split_heads(t, H):
    """[B, n, H*dh] -> [B, H, n, dh]."""
    B, n, w = t.shape
    return t.reshape(B, n, H, w // H).permute(0, 2, 1, 3)
