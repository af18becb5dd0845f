"""The embed path the gated-attention MIL models share (``models/CLAM.py``, ``dtfd.py``; the gate
layer's backward also ``models/AttMIL.py``): ``h = ReLU(x W1^T [+ b1])``, the stacked gate layer
``Z = h Wab^T + bab`` (``Wab = [Wa;Wb]``: the tanh branch's rows, then the sigmoid branch's) and their
backward, on the HIP GEMM (f32 MFMA) and the fp32 row passes.  fp32 throughout.  Every kernel is
deterministic and the launches that do not depend on each other write disjoint buffers, so the
order they are issued in here is not part of any result.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import F32
from .engine import _p, _stream, colsum, gemm, weight_grad


def _f32c(t):
    return t.detach().float().contiguous()


def device_label(label, who):
    """``label`` as the kernels read it: an int64 GPU tensor, flattened (never copied to the host)."""
    if not label.is_cuda or label.dtype != torch.int64:
        raise RuntimeError(f"{who}: label must be an int64 GPU tensor (it is read on the device)")
    return label.reshape(-1)


def embed(x, W1, b1, Wab, bab):
    """h [N, L] = ReLU(x W1^T + b1) (``b1`` None: no bias), Z [N, 2D] = h Wab^T + bab."""
    N, Fin = x.shape
    L, D2 = W1.shape[0], Wab.shape[0]
    h = torch.empty(N, L, device=x.device)
    gemm(x, W1, h, N, L, Fin, lda=Fin, ldb=Fin, ldc=L, dtype=F32, c_dtype=F32)
    if b1 is not None:
        _lib.call("tm_bias_act", F32, _p(h), _p(b1), N, L, 1, _stream())
    else:
        _lib.call("tm_relu", _p(h), N * L, _stream())
    Z = torch.empty(N, D2, device=x.device)
    gemm(h, Wab, Z, N, D2, L, lda=L, ldb=L, ldc=D2, dtype=F32, c_dtype=F32, bias=bab)
    return h, Z


def gate_layer_bwd(dZ, h, Wab, dh, pool, need_dh=True, need_params=True):
    """The gate layer's backward from dZ [N, 2D]: ``dh += dZ Wab`` in place (``need_dh``), and returns
    ``(dWab [2D, L] = dZ^T h, dbab [2D] = colsum(dZ))`` (``need_params``; else two None)."""
    N, D2 = dZ.shape
    L = h.shape[1]
    if need_dh:
        gemm(dZ, Wab, dh, N, L, D2, lda=D2, ldb=L, ldc=L, b_kn=1, dtype=F32, c_dtype=F32, accumulate=True)
    if not need_params:
        return None, None
    dWab = torch.empty(D2, L, device=dZ.device)
    weight_grad(dZ, h, dWab, D2, L, N, ldy=D2, ldx=L, dtype=F32, work_pool=pool)
    dbab = torch.empty(D2, device=dZ.device)
    colsum(dZ, N, D2, D2, F32, dbab, pool)
    return dWab, dbab


def embed_bwd(dZ, dh, h, x, W1, Wab, pool, need_dx, need_dW1, need_db1, need_gate=True):
    """``embed``'s backward from dZ [N, 2D] and the pooling's own dh [N, L] (overwritten: the gate
    layer's share is added, then the ReLU is taken back).  Returns ``(dx, dW1, db1, dWab, dbab)``, None
    where the flag is off (``need_gate``: the last two); with the first three off dh is left as it is."""
    N, Fin = x.shape
    L = h.shape[1]
    need_dh = need_dx or need_dW1 or need_db1
    dWab, dbab = gate_layer_bwd(dZ, h, Wab, dh, pool, need_dh, need_gate)
    dx = dW1 = db1 = None
    if need_dh:
        _lib.call("tm_relu_bwd", _p(dh), _p(h), N * L, _stream())
    if need_dW1:
        dW1 = torch.empty(L, Fin, device=dZ.device)
        weight_grad(dh, x, dW1, L, Fin, N, ldy=L, ldx=Fin, dtype=F32, work_pool=pool)
    if need_db1:
        db1 = torch.empty(L, device=dZ.device)
        colsum(dh, N, L, L, F32, db1, pool)
    if need_dx:
        dx = torch.empty(N, Fin, device=dZ.device)
        gemm(dh, W1, dx, N, Fin, L, lda=L, ldb=Fin, ldc=Fin, b_kn=1, dtype=F32, c_dtype=F32)
    return dx, dW1, db1, dWab, dbab
