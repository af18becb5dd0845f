"""The fp64 restatements of tests/kernel_refs.py against fp64 autograd of the oracle pieces or of a
direct dense formulation (CPU only): all agree to 1e-10."""
import numpy as np
import pytest
import torch

import kernel_refs as R

TOL = 1e-10


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


# ----------------------------------------------------------------------------- dropout hash
def _u01_scalar(seed, row, col):
    """common.h dropout_u01, one element at a time in Python integers."""
    M = 0xFFFFFFFF

    def mix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M
        h ^= h >> 16
        return h
    h = mix((seed & M) ^ mix((row * 0x9E3779B1 + (seed >> 32)) & M))
    h = mix(h ^ ((col * 0x7FEB352D) & M))
    return float(np.float32(h >> 8) * np.float32(1.0 / 16777216.0))


def test_dropout_keep_is_the_scalar_hash():
    ctr, layer = 5, 0x1234ABCD9876
    seed = (ctr * 0x9E3779B97F4A7C15 + layer) & (2 ** 64 - 1)
    keep = R.dropout_keep(ctr, layer, 300, 40, 0.7)
    p32 = float(np.float32(0.7))
    for row, col in [(0, 0), (1, 0), (0, 1), (77, 39), (299, 17), (154, 3), (255, 31)]:
        assert keep[row, col] == (_u01_scalar(seed, row, col) >= p32)
    assert abs(keep.mean() - 0.3) < 0.02
    # seed_ptr = NULL is effective_seed = seed: counter 0
    assert np.array_equal(R.dropout_keep(0, seed, 300, 40, 0.7), keep)


# ----------------------------------------------------------------------------- A3 backward
@pytest.mark.parametrize("nbh,nh,n,lo,hi", [(2, 2, 768, 0, 768), (4, 2, 512, 150, 183), (2, 1, 256, 238, 256)])
def test_a3_bwd_fused_ref_is_autograd_of_the_attention_and_the_landmark_means(nbh, nh, n, lo, hi):
    """W = softmax(ql k^T) v with upstream dw; k also enters through the landmark means k~ (App. A
    eq. 2) with upstream dkl, v also through a conv output whose gradient w.r.t. v is dv_conv inside
    the window and zero outside: autograd of  sum(W dw) + sum(mean_l(k) dkl) + sum(v[lo:hi] dv_conv)."""
    from test_kernels_gpu import _a3_bwd_ref
    g = _gen(n + nbh)
    l = n // 256
    ql, dw = _randn(g, nbh, 256, 64, scale=0.3), _randn(g, nbh, 256, 64, scale=0.1)
    k, v = _randn(g, nbh, n, 64, scale=0.3), _randn(g, nbh, n, 64)
    dkl, dvc = _randn(g, nbh, 256, 64), _randn(g, nbh, n, 64)
    qa, ka, va = (t.clone().requires_grad_() for t in (ql, k, v))
    w = torch.softmax(qa @ ka.transpose(1, 2), -1) @ va
    loss = (w * dw).sum() + (ka.view(nbh, 256, l, 64).mean(2) * dkl).sum() + (va[:, lo:hi] * dvc[:, lo:hi]).sum()
    loss.backward()
    dvc_nan = dvc.clone()
    dvc_nan[:, :lo] = float("nan")
    dvc_nan[:, hi:] = float("nan")
    kc, vc, dql = R.a3_bwd_fused_ref(ql, dw, k, v, dvc_nan, lo, hi, dkl, nh)
    assert _rel(kc, R.heads_to_cols(ka.grad, nh)) < TOL
    assert _rel(vc, R.heads_to_cols(va.grad, nh)) < TOL
    assert _rel(dql, qa.grad) < TOL
    # and the per-head loop equals the batched restatement the unfused kernel's test uses
    for a, b in zip(R.a3_bwd_ref(ql, dw, k, v), _a3_bwd_ref(ql, dw, k, v)):
        assert _rel(a, b) < TOL


def test_heads_to_cols_is_the_dqkv_column_layout():
    x = torch.arange(4 * 3 * 64, dtype=torch.float64).view(4, 3, 64)       # 2 bags x 2 heads, 3 rows
    c = R.heads_to_cols(x, 2)
    assert c.shape == (2, 3, 128)
    for b in range(2):
        for h in range(2):
            assert torch.equal(c[b, :, h * 64:(h + 1) * 64], x[b * 2 + h])


def test_slab_sum_orders():
    g = _gen(3)
    s = torch.randn(33, 64, generator=g).bfloat16()
    plain = R.slab_sum_f32(s)
    acc = torch.zeros(64)
    for z in range(33):
        acc = acc + s[z].float()
    assert torch.equal(plain, acc)
    ev, od = torch.zeros(64), torch.zeros(64)
    for z in range(0, 33, 2):
        ev = ev + s[z].float()
    for z in range(1, 33, 2):
        od = od + s[z].float()
    assert torch.equal(R.slab_sum_f32(s, 2), ev + od)
    assert _rel(R.slab_sum_f32(s, 4), s.double().sum(0)) < 1e-6
    assert R.reduce_par(24, 2 * 256 * 64) == 1 and R.reduce_par(32, 8 * 256 * 64) == 2
    assert R.reduce_par(33, 16 * 256 * 64) == 2 and R.reduce_par(16, 4099) == 1


def test_assemble_q_ref_is_the_chain_rule_of_the_landmark_means():
    """q enters through its rows (gradient dq, only row r non-zero) and through q~ = mean_l(q)
    (gradient dql_total); the q columns are scale * dL/dq because the stored q is scale * (x Wq)."""
    g = _gen(9)
    nbh, nh, n, r, scale = 4, 2, 768, 300, 0.125
    l = n // 256
    dq, dqt = _randn(g, nbh, n, 64), _randn(g, nbh, 256, 64)
    q = _randn(g, nbh, n, 64).requires_grad_()
    loss = (q[:, r] * dq[:, r]).sum() + (q.view(nbh, 256, l, 64).mean(2) * dqt).sum()
    loss.backward()
    dq_nan = torch.full_like(dq, float("nan"))
    dq_nan[:, r] = dq[:, r]
    assert _rel(R.assemble_q_ref(dq_nan, r, dqt, nh, scale), scale * R.heads_to_cols(q.grad, nh)) < TOL
    loss2 = (q * dq).sum() + (q.view(nbh, 256, l, 64).mean(2) * dqt).sum()
    q.grad = None
    loss2.backward()
    assert _rel(R.assemble_q_ref(dq, -1, dqt, nh, scale), scale * R.heads_to_cols(q.grad, nh)) < TOL


# ----------------------------------------------------------------------------- class row
@pytest.mark.parametrize("B,n,r", [(1, 256, 254), (2, 512, 0), (2, 512, 5), (3, 512, 300)])
def test_cls_a1_row_ref_is_row_r_of_the_dense_a1(B, n, r):
    from test_kernels_gpu import _a1_ref
    nh = 2
    nbh = B * nh
    g = _gen(n + r)
    q, v = _randn(g, nbh, n, 64, scale=0.3), _randn(g, nbh, n, 64)
    kl, y = _randn(g, nbh, 256, 64, scale=0.3), _randn(g, nbh, 256, 64)
    wconv = _randn(g, nh, 33, scale=0.1)
    dm = _randn(g, B, nh * 64, scale=0.1)
    m_ref, lse_ref = _a1_ref(q, v, kl, y, wconv, nh)
    m, lse = R.cls_a1_row_ref(q, v, kl, y, wconv, nh, r)
    assert _rel(m, m_ref[:, r]) < TOL and _rel(lse, lse_ref[:, r]) < TOL
    # backward: autograd of the dense formulation with a one-row upstream gradient
    ins = [t.clone().requires_grad_() for t in (q, v, kl, y, wconv)]
    md, _ = _a1_ref(*ins, nh)
    up = torch.zeros_like(md)
    up[:, r] = dm
    gq, gv, gkl, gy, gw = torch.autograd.grad(md, ins, up)
    dq_row, dkl, dy, dvw, dwc = R.cls_a1_row_bwd_ref(dm, q, v, kl, y, wconv, nh, r)
    lo, hi = max(r - 16, 0), min(r + 17, n)
    assert dvw.shape[1] == hi - lo
    assert _rel(dq_row, gq[:, r]) < TOL and _rel(dkl, gkl) < TOL and _rel(dy, gy) < TOL
    assert _rel(dvw, gv[:, lo:hi]) < TOL and _rel(dwc, gw.view(nh, 33)) < TOL
    # the dense gradient is zero outside row r of dq and outside the window of dv
    gq[:, r] = 0
    gv[:, lo:hi] = 0
    assert gq.abs().max() == 0 and gv.abs().max() == 0


def test_cls_a1_row_ref_is_the_oracle_attention_row():
    """Through oracle/nystrom_ref.py: with Y = Z (A3 v) the class row of (attn1 @ Y + res_conv(v))
    of the oracle's forward equals the restatement (heads merged as 'b n (h d)')."""
    from oracle.nystrom_ref import NystromAttention
    torch.manual_seed(2)
    att = NystromAttention(dim=128, dim_head=64, heads=2, num_landmarks=256, pinv_iterations=6, residual=True).double()
    g = _gen(4)
    nh, n, r = 2, 512, 37
    q, v = _randn(g, nh, n, 64, scale=0.3), _randn(g, nh, n, 64)
    kl, y = _randn(g, nh, 256, 64, scale=0.3), _randn(g, nh, 256, 64)
    wconv = att.res_conv.weight.detach().view(nh, 33)
    dense = torch.softmax(q @ kl.transpose(1, 2), -1) @ y + att.res_conv(v[None])[0]
    m, _ = R.cls_a1_row_ref(q, v, kl, y, wconv, nh, r)
    assert _rel(m, dense[:, r].reshape(1, nh * 64)) < TOL


# ----------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("B,S,n,pad,seg_len", [(2, 77, 256, 179, 1), (1, 130, 1280, 1150, 5)])
@pytest.mark.parametrize("resid_cls_only", [0, 1])
@pytest.mark.parametrize("use_seg", [False, True])
def test_ln_bwd_seg_ref_is_autograd_of_layer_norm(B, S, n, pad, seg_len, resid_cls_only, use_seg):
    D, nseg, seg_rows = 64, 256, 288
    g = _gen(S + pad)
    x = _randn(g, B * S, D).requires_grad_()
    gamma, beta = (_randn(g, D, scale=0.3) + 1).requires_grad_(), _randn(g, D).requires_grad_()
    dy = _randn(g, B, n, D)
    dy_nan = dy.clone()
    dy_nan[:, :pad] = float("nan")                  # pad rows are not read
    seg = _randn(g, B, seg_rows, D) if use_seg else None
    acc = _randn(g, B * S, D)
    up = dy[:, pad:].clone()
    if use_seg:
        for t in range(S):
            up[:, t] += seg[:, (pad + t) // seg_len]
        up[:, 0] += seg[:, nseg]
    y = torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5)
    y.backward(up.reshape(B * S, D))
    xd = x.detach()
    mean = xd.mean(-1)
    rstd = 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-5)
    want = x.grad.clone().view(B, S, D)
    accv = acc.view(B, S, D)
    acc_in = acc.clone()
    if resid_cls_only:
        want[:, 0] += accv[:, 0]
        acc_in.view(B, S, D)[:, 1:] = float("nan")   # written without being read
    else:
        want += accv
    dx, dg, db = R.ln_bwd_seg_ref(dy_nan, xd, gamma.detach(), mean, rstd, S, pad, acc_in, resid_cls_only,
                                  seg=seg, seg_len=seg_len, nseg=nseg)
    assert torch.isfinite(dx).all()
    assert _rel(dx, want.reshape(B * S, D)) < TOL
    assert _rel(dg, gamma.grad) < TOL and _rel(db, beta.grad) < TOL


def test_ln_bwd_ref_is_the_oracle_translayer_norm():
    """The TransLayer's pre-norm of oracle/transmil_ref.py: x + f(norm(x)) with a linear f; the
    input gradient is the residual gradient plus LN'(dy), as the kernel accumulates it."""
    from oracle.transmil_ref import TransLayer
    torch.manual_seed(1)
    norm = TransLayer(dim=512).norm.double()
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.2, 0.2)
    g = _gen(6)
    B, S, D, pad = 2, 9, 512, 3
    x = _randn(g, B * S, D).requires_grad_()
    a = _randn(g, D, D, scale=0.05)
    gy = _randn(g, B * S, D)
    out = x + norm(x) @ a
    out.backward(gy)
    dy = torch.full((B, S + pad, D), float("nan"), dtype=torch.float64)
    dy[:, pad:] = (gy @ a.t()).view(B, S, D)
    xd = x.detach()
    mean, rstd = xd.mean(-1), 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + norm.eps)
    dx, dg, db = R.ln_bwd_seg_ref(dy, xd, norm.weight.detach(), mean, rstd, S, pad, gy, 0)
    assert _rel(dx, x.grad) < TOL and _rel(dg, norm.weight.grad) < TOL and _rel(db, norm.bias.grad) < TOL
