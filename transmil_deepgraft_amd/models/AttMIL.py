"""Drop-in ``models/AttMIL.py`` (code/models/AttMIL.py:20-110): gated attention MIL pooling
(Ilse et al. 2018) on the MI355X HIP kernels.

Same constructor, parameter names and ``forward(x) -> logits``.  The forward is
``_fc1`` (HIP GEMM Linear+GELU, Dropout, HIP LayerNorm, ...), then one fused pooling node:
``Z = H [Wv;Wu]^T + [bv;bu]`` on the HIP GEMM (f32 MFMA) and ``tm_attmil_fwd`` (scores
``w . tanh(Zv) sigmoid(Zu) + b``, softmax over the N instances, ``M = p H``, the classifier);
the backward is ``tm_attmil_bwd`` plus three GEMM/colsum launches.  That is the fp32 compute mode,
the default of a directly constructed model.

``set_compute_dtype(torch.bfloat16)`` (what ``config.build_model`` selects for ``precision: 16``)
keeps the fp32 master parameters and runs the ``_fc1`` Linears and the gate layer on the bf16 MFMA
GEMM with fp32 accumulation: the bag and those layers' weights are rounded to bf16 (one cast launch for
the weights; a bf16 bag is read as it is), the GELU pre-activations are kept in bf16, LayerNorm takes
fp32 input and statistics and writes bf16, ``H`` and ``Z`` are produced, saved and read in bf16 by
the typed pooling kernels (``tm_attmil_pool_fwd`` / ``_bwd``: fp32 arithmetic, scores, softmax
statistics, ``M``, logits and parameter gradients), and the backward products take bf16 operands
with fp32 outputs.  In that mode everything after the Dropout is one autograd node, so forward hooks on
``_fc1``'s LayerNorm / last Linear do not fire.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import BF16, F32
from ..engine import LN_EPS, Pool, _p, _stream, gemm, weight_grad
from ..gated import gate_layer_bwd


class _GatedPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, wvu, bvu, w, b, wc, bc):
        N, L = H.shape
        D2, C = wvu.shape[0], wc.shape[0]
        D = D2 // 2
        dev = H.device
        Hc = H.contiguous()
        Z = torch.empty(N, D2, device=dev)
        gemm(Hc, wvu.contiguous(), Z, N, D2, L, lda=L, ldb=L, ldc=D2, dtype=F32, c_dtype=F32, bias=bvu.contiguous())
        work = torch.empty(_lib.query("tm_attmil_fwd_workspace", N, L) // 4, device=dev)
        a, p = torch.empty(N, device=dev), torch.empty(N, device=dev)
        M = torch.empty(L, device=dev)
        logits = torch.empty(1, C, device=dev)
        _lib.call("tm_attmil_fwd", _p(Z), _p(Hc), _p(w.contiguous()), _p(b.contiguous()), _p(wc.contiguous()),
                  _p(bc.contiguous()), N, L, D, C, _p(work), _p(a), _p(p), _p(M), _p(logits), _stream())
        ctx.save_for_backward(Hc, Z, wvu, w, p, M, wc)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        H, Z, wvu, w, p, M, wc = ctx.saved_tensors
        N, L = H.shape
        D2, C = wvu.shape[0], wc.shape[0]
        D = D2 // 2
        dev = H.device
        work = torch.empty(_lib.query("tm_attmil_bwd_workspace", N, L, D) // 4, device=dev)
        dZ, dH = torch.empty(N, D2, device=dev), torch.empty(N, L, device=dev)
        dM, dw, db = torch.empty(L, device=dev), torch.empty(1, D, device=dev), torch.empty(1, device=dev)
        dwc, dbc = torch.empty(C, L, device=dev), torch.empty(C, device=dev)
        _lib.call("tm_attmil_bwd", _p(Z), _p(H), _p(w.contiguous()), _p(p), _p(M), _p(wc.contiguous()),
                  _p(dlogits.float().contiguous()), N, L, D, C, _p(work), _p(dZ), _p(dH), _p(dM), _p(dw), _p(db),
                  _p(dwc), _p(dbc), _stream())
        dwvu, dbvu = gate_layer_bwd(dZ, H, wvu.contiguous(), dH, Pool(dev))
        return dH, dwvu, dbvu, dw, db, dwc, dbc


class _TailBf16Fn(torch.autograd.Function):
    """bf16 mode, everything after ``_fc1``'s Dropout as one node: LayerNorm (fp32 in, bf16 out), the
    2048 branch's second Linear + GELU (bf16 out, pre-activation bf16), the gate layer (``Z`` bf16) and the
    typed pooling.  ``w1t`` / ``wvut``: the bf16 copies of ``w1`` and of ``[Vw; Uw]``; ``w1`` None: the
    1024 branch (``H`` is the LayerNorm output).  No bf16 tensor crosses the node's boundary, so autograd
    never rounds a gradient."""

    @staticmethod
    def forward(ctx, y0, lnw, lnb, eps, w1, b1, w1t, Vw, Vb, Uw, Ub, wvut, w, b, wc, bc):
        N, Fm = y0.shape
        dev = y0.device
        st = _stream()
        bf = torch.bfloat16
        y0 = y0.contiguous()
        xln = torch.empty(N, Fm, dtype=bf, device=dev)
        mean, rstd = torch.empty(N, device=dev), torch.empty(N, device=dev)
        _lib.call("tm_layernorm_fwd", _p(y0), _p(lnw), _p(lnb), C.c_float(eps), N, Fm, N, N, 0, BF16, _p(xln),
                  _p(mean), _p(rstd), st)
        pre1 = None
        if w1 is not None:
            L = w1.shape[0]
            H = torch.empty(N, L, dtype=bf, device=dev)
            pre1 = torch.empty(N, L, dtype=bf, device=dev)
            gemm(xln, w1t, H, N, L, Fm, lda=Fm, ldb=Fm, ldc=L, dtype=BF16, c_dtype=BF16, bias=b1, gelu=True, pre=pre1,
                 ld_pre=L, pre_bf16=True)
        else:
            L, H = Fm, xln
        D2, Cn = wvut.shape[0], wc.shape[0]
        D = D2 // 2
        Z = torch.empty(N, D2, dtype=bf, device=dev)
        gemm(H, wvut, Z, N, D2, L, lda=L, ldb=L, ldc=D2, dtype=BF16, c_dtype=BF16, bias=torch.cat([Vb, Ub]))
        work = torch.empty(_lib.query("tm_attmil_pool_fwd_workspace", N, L) // 4, device=dev)
        a, stats, M = torch.empty(N, device=dev), torch.empty(4, device=dev), torch.empty(L, device=dev)
        logits = torch.empty(1, Cn, device=dev)
        wq, wcq = w.contiguous(), wc.contiguous()
        _lib.call("tm_attmil_pool_fwd", BF16, _p(Z), _p(H), _p(wq), _p(b.contiguous()), _p(wcq),
                  _p(bc.contiguous()), N, L, D, Cn, _p(work), _p(a), _p(stats), _p(M), _p(logits), st)
        ctx.save_for_backward(y0, lnw, mean, rstd, xln, w1t, pre1, H, Z, wvut, wq, a, stats, M, wcq)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        y0, lnw, mean, rstd, xln, w1t, pre1, H, Z, wvut, w, a, stats, M, wc = ctx.saved_tensors
        N, Fm = y0.shape
        L, D2, Cn = H.shape[1], Z.shape[1], wc.shape[0]
        D = D2 // 2
        dev = y0.device
        st = _stream()
        bf = torch.bfloat16
        pool = Pool(dev)
        work = torch.empty(_lib.query("tm_attmil_pool_bwd_workspace", N, L, D) // 4, device=dev)
        dZ, dH = torch.empty(N, D2, dtype=bf, device=dev), torch.empty(N, L, device=dev)
        dw, db = torch.empty(1, D, device=dev), torch.empty(1, device=dev)
        dwc, dbc = torch.empty(Cn, L, device=dev), torch.empty(Cn, device=dev)
        _lib.call("tm_attmil_pool_bwd", BF16, _p(Z), _p(H), _p(w), _p(a), _p(stats), _p(M), _p(wc),
                  _p(dlogits.float().contiguous()), N, L, D, Cn, _p(work), _p(dZ), _p(dH), _p(dw), _p(db), _p(dwc),
                  _p(dbc), st)
        # the gate layer: dH += dZ [Wv;Wu], d[Wv;Wu] = dZ^T H, d[bv;bu] = colsum(dZ)
        gemm(dZ, wvut, dH, N, L, D2, lda=D2, ldb=L, ldc=L, b_kn=1, dtype=BF16, c_dtype=F32, accumulate=True)
        dwvu, dbvu = torch.empty(D2, L, device=dev), torch.empty(D2, device=dev)
        weight_grad(dZ, H, dwvu, D2, L, N, ldy=D2, ldx=L, dtype=BF16, work_pool=pool, bias_out=dbvu)
        dw1 = db1 = None
        dln = dH
        if w1t is not None:
            dpre1 = torch.empty(N, L, dtype=bf, device=dev)
            _lib.call("tm_gelu_bwd_pre", BF16, _p(dH), _p(pre1), N * L, _p(dpre1), st)
            dln = torch.empty(N, Fm, device=dev)
            gemm(dpre1, w1t, dln, N, Fm, L, lda=L, ldb=Fm, ldc=Fm, b_kn=1, dtype=BF16, c_dtype=F32)
            dw1, db1 = torch.empty(L, Fm, device=dev), torch.empty(L, device=dev)
            weight_grad(dpre1, xln, dw1, L, Fm, N, ldy=L, ldx=Fm, dtype=BF16, work_pool=pool, bias_out=db1)
        dy0 = torch.zeros(N, Fm, device=dev)
        dlnw, dlnb = torch.empty_like(lnw), torch.empty_like(lnw)
        rpb = 64
        lwork = torch.empty(_lib.query("tm_layernorm_bwd_workspace", N, Fm, rpb) // 4, device=dev)
        _lib.call("tm_layernorm_bwd", _p(dln), F32, _p(y0), _p(lnw), _p(mean), _p(rstd), N, Fm, N, N, 0, rpb, 0,
                  _p(dy0), _p(lwork), _p(dlnw), _p(dlnb), C.c_void_p(0), st)
        return (dy0, dlnw, dlnb, None, dw1, db1, None, dwvu[:D], dbvu[:D], dwvu[D:], dbvu[D:], None, dw, db, dwc,
                dbc)


class AttMIL(nn.Module):
    """``code/models/AttMIL.py:20-110``.  ``feature_extractor_part2`` is constructed (state_dict)
    but unused, as in the reference; ``in_features`` other than 2048 / 1024 leave ``_fc1``
    undefined there too (the forward then fails the same way)."""

    def __init__(self, n_classes, in_features=2048, out_features=512):
        super().__init__()
        self.L, self.D, self.K = out_features, 128, 1
        self.n_classes = n_classes
        if in_features == 2048:                                     # :55-59
            self._fc1 = nn.Sequential(nn.Linear(in_features, in_features // 2), nn.GELU(), nn.Dropout(p=0.6),
                                      ops.LayerNorm(in_features // 2),
                                      nn.Linear(in_features // 2, out_features), nn.GELU())
        elif in_features == 1024:                                   # :60-63
            self._fc1 = nn.Sequential(nn.Linear(in_features, out_features), nn.GELU(), nn.Dropout(p=0.6),
                                      ops.LayerNorm(out_features))
        self.feature_extractor_part2 = nn.Sequential(nn.Linear(in_features, self.L), nn.ReLU())
        self.attention_V = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh())
        self.attention_U = nn.Sequential(nn.Linear(self.L, self.D), nn.Sigmoid())
        self.attention_weights = nn.Linear(self.D, self.K)
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, self.n_classes))
        self.compute_dtype = torch.float32

    def set_compute_dtype(self, dtype: torch.dtype):
        """torch.float32 (the default: fp32 MFMA, the reference's arithmetic) or torch.bfloat16 (bf16
        GEMM operands, ``H`` / ``Z`` in bf16; see the module docstring).  Touches neither the GPU nor
        the library."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"AttMIL: compute dtype must be torch.bfloat16 or torch.float32, got {dtype}")
        self.compute_dtype = dtype
        return self

    def _embed(self, x):
        """_fc1 on the HIP ops: x [1, N, F] -> H [1, N, L]."""
        f = self._fc1
        h = ops.linear_gelu(f[0], x)
        h = f[2](h)
        h = f[3](h)
        if len(f) == 6:
            h = ops.linear_gelu(f[4], h)
        return h

    def forward(self, x):
        x = x.squeeze()                                             # :93
        if not x.is_cuda:
            raise RuntimeError("AttMIL (HIP) needs a GPU tensor: there is no CPU path")
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError(f"AttMIL pools one bag: x.squeeze() must be [N, F], got {tuple(x.shape)}")
        if self.compute_dtype == torch.bfloat16:
            return self._forward_bf16(x)
        h = self._embed(x.float()[None])[0]                         # :94
        V, U = self.attention_V[0], self.attention_U[0]
        return _GatedPoolFn.apply(h, torch.cat([V.weight, U.weight]), torch.cat([V.bias, U.bias]),
                                  self.attention_weights.weight, self.attention_weights.bias,
                                  self.classifier[0].weight, self.classifier[0].bias)

    def _forward_bf16(self, x):
        """x [N, F] (bf16: read as it is; else cast once) -> logits [1, C] in the bf16 compute mode."""
        f = self._fc1
        V, U = self.attention_V[0], self.attention_U[0]
        two = len(f) == 6
        wvut = torch.empty(2 * self.D, self.L, dtype=torch.bfloat16, device=x.device)
        srcs = [f[0].weight, V.weight, U.weight] + ([f[4].weight] if two else [])
        dsts = [torch.empty(f[0].weight.shape, dtype=torch.bfloat16, device=x.device), wvut[:self.D], wvut[self.D:]]
        if two:
            dsts.append(torch.empty(f[4].weight.shape, dtype=torch.bfloat16, device=x.device))
        ops.cast_bf16_many(srcs, dsts)                              # one launch for all weight operands
        y0 = ops.linear_gelu_bf16(f[0], x, dsts[0])
        y0 = f[2](y0)                                               # torch's Dropout, as in fp32 mode
        ln = f[3]
        w1, b1, w1t = (f[4].weight, f[4].bias, dsts[3]) if two else (None, None, None)
        return _TailBf16Fn.apply(y0, ln.weight, ln.bias, getattr(ln, "eps", LN_EPS), w1, b1, w1t, V.weight, V.bias,
                                 U.weight, U.bias, wvut, self.attention_weights.weight,
                                 self.attention_weights.bias, self.classifier[0].weight, self.classifier[0].bias)
