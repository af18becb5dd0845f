"""TransMIL out_features 256 / 384 on the MI355X: the tm_nysg_* kernels (dim_head 32 / 48, 128 / 192
landmarks) against fp64 torch evaluations of the same formulas, NystromAttention against the fp64
oracle, and the whole model (fp32 parity mode, the two reference fixtures, bf16 mode, return_attn,
hooks, the training task).

Kernel bounds are the ones the (64, 256) fp32 kernels are held to in test_kernels_gpu.py
(_F32_CASES, test_landmarks_segment_means, test_pinv_fwd_bwd_fp32_exact_path) and
test_pinv_split_gpu.py (the fp32 A2 at 1e-6, the peaky chain at 1e-3).  tm_nysg_mm and
tm_nysg_assemble_dqkv have no fp32 case there: their bound is 4x the error of the fp32 torch
evaluation of the same formula against the fp64 one on the same inputs (measured on the CPU, the
figures beside the bounds), the headroom for a different summation order."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from golden_util import load, bag_input
from kernel_refs import a3_bwd_ref, heads_to_cols

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOS = [(32, 128), (48, 192)]
NBH, NH = 16, 8            # 2 bags x 8 heads: the chain's global maxima couple the bags
TAPS, HALF = 33, 16


def _L():
    from transmil_deepgraft_amd import _lib
    return _lib


def _ps():
    from transmil_deepgraft_amd.engine import _p, _stream
    return _p, _stream


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _absmax(a, b):
    return (a.double() - b.double()).abs().max().item()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum((i + 1) * 1009 * int(k) for i, k in enumerate(key)))


def _dev(*ts):
    return tuple(t.float().to(DEV).contiguous() for t in ts)


def _check(figs, bounds):
    """figs {output: (got, fp64 ref, "rel" | "abs")}; every figure printed before any assertion."""
    errs = {}
    for name, (got, ref, kind) in figs.items():
        assert torch.isfinite(got).all(), name
        errs[name] = _rel(got, ref) if kind == "rel" else _absmax(got, ref)
    print(" ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert set(errs) == set(bounds)
    for name, err in errs.items():
        assert err < bounds[name], (name, err, bounds[name])


def _cases():
    return [(dh, nl, f * nl) for dh, nl in GEOS for f in (1, 2, 5)]   # l = 1 (one token per segment), 2, 5


# ----------------------------------------------------------------------------- fp64 restatements
def _conv(v, wconv, nh):
    """conv33 residual per head: out[bh][t] = sum_tau w[bh % nh][tau] v[bh][t + tau - 16]."""
    nbh, n, _ = v.shape
    vp = torch.nn.functional.pad(v, (0, 0, HALF, HALF))
    w = wconv[torch.arange(nbh) % nh]
    return sum(w[:, tau, None, None] * vp[:, tau:tau + n] for tau in range(TAPS))


def _cols_to_heads(x, nh):
    """[B, n, nh*dh] -> [B*nh, n, dh]."""
    B, n, inner = x.shape
    return x.view(B, n, nh, inner // nh).permute(0, 2, 1, 3).reshape(B * nh, n, inner // nh)


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dh,nl,n", _cases())
def test_landmarks(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(1, dh, n)
    q, k = torch.randn(NBH, n, dh, generator=g), torch.randn(NBH, n, dh, generator=g)
    l = n // nl
    ql, kl = _nan(NBH, nl, dh), _nan(NBH, nl, dh)
    qd, kd = _dev(q, k)
    L.call("tm_nysg_landmarks", dh, nl, p(qd), p(kd), NBH, n, p(ql), p(kl), st())
    torch.cuda.synchronize()
    _check({"ql": (ql.cpu(), q.double().view(NBH, nl, l, dh).mean(2), "abs"),
            "kl": (kl.cpu(), k.double().view(NBH, nl, l, dh).mean(2), "abs")}, {"ql": 1e-5, "kl": 1e-5})


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_a3_fwd(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(2, dh, n)
    ql = torch.randn(NBH, nl, dh, generator=g) * 0.4
    k = torch.randn(NBH, n, dh, generator=g) * 0.4
    v = torch.randn(NBH, n, dh, generator=g)
    s = ql.double() @ k.double().transpose(1, 2)
    w, lse = _nan(NBH, nl, dh), _nan(NBH, nl)
    work = torch.empty(L.query("tm_nysg_a3_workspace", dh, nl, NBH, n) // 4 + 16, device=DEV)
    qd, kd, vd = _dev(ql, k, v)
    L.call("tm_nysg_a3_fwd", dh, nl, p(qd), p(kd), p(vd), NBH, n, p(work), p(w), p(lse), st())
    torch.cuda.synchronize()
    _check({"w": (w.cpu(), torch.softmax(s, -1) @ v.double(), "rel"), "lse3": (lse.cpu(), torch.logsumexp(s, -1), "abs")},
           {"w": 6.00e-6, "lse3": 3.45e-6})


@pytest.mark.parametrize("dh,nl", GEOS)
def test_sim2_softmax(dh, nl):
    L, (p, st) = _L(), _ps()
    g = _gen(3, dh)
    ql = torch.randn(NBH, nl, dh, generator=g) * 0.2
    kl = torch.randn(NBH, nl, dh, generator=g) * 0.2
    a2 = _nan(NBH, nl, nl)
    qd, kd = _dev(ql, kl)
    L.call("tm_nysg_sim2_softmax", dh, nl, p(qd), p(kd), NBH, p(a2), st())
    torch.cuda.synchronize()
    exact = torch.softmax(ql.double() @ kl.double().transpose(1, 2), -1)
    _check({"a2": (a2.cpu(), exact, "rel")}, {"a2": 1e-6})
    assert torch.allclose(a2.cpu().double().sum(-1), torch.ones(NBH, nl, dtype=torch.float64), atol=1e-5)


def _chain(dh, nl, s64, gz):
    """Z_6 = pinv(softmax(s)) and dL/ds through tm_nysg_pinv_fwd / _bwd / softmax_bwd_rows."""
    L, (p, st) = _L(), _ps()
    X = torch.softmax(s64.detach(), -1).float().to(DEV).contiguous()
    mat = NBH * nl * nl
    saved = torch.full((L.query("tm_nysg_pinv_saved_floats", dh, nl, NBH, 6),), float("nan"), device=DEV)
    L.call("tm_nysg_pinv_fwd", dh, nl, p(X), NBH, 6, p(saved), st())
    z = saved[6 * mat:7 * mat].view(NBH, nl, nl).clone()
    work = torch.full((L.query("tm_nysg_pinv_bwd_workspace_floats", dh, nl, NBH),), float("nan"), device=DEV)
    dz = gz.float().to(DEV).contiguous()
    dX, ds = _nan(NBH, nl, nl), _nan(NBH, nl, nl)
    L.call("tm_nysg_pinv_bwd", dh, nl, p(X), NBH, 6, p(saved), p(dz), p(work), p(dX), st())
    L.call("tm_nysg_softmax_bwd_rows", dh, nl, p(X), p(dX), p(ds), NBH * nl, st())
    torch.cuda.synchronize()
    return z.cpu(), ds.cpu()


@pytest.mark.parametrize("dh,nl", GEOS)
def test_pinv_chain_fwd_bwd(dh, nl):
    """As test_pinv_fwd_bwd_fp32_exact_path: Z and dL/ds (dL/dA2 itself carries the tie-dependent
    row-constant term the softmax backward annihilates); 16 heads = 2 bags under one global max."""
    from oracle.nystrom_ref import moore_penrose_iter_pinv
    g = _gen(4, dh)
    s64 = (torch.randn(NBH, nl, nl, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    z_ref = moore_penrose_iter_pinv(torch.softmax(s64, -1), 6)
    gz = torch.randn(NBH, nl, nl, generator=g, dtype=torch.float64) * 1e-3
    z_ref.backward(gz)
    z, ds = _chain(dh, nl, s64, gz)
    _check({"z": (z, z_ref.detach(), "rel"), "ds": (ds, s64.grad, "rel")}, {"z": 2e-4, "ds": 2e-3})


@pytest.mark.parametrize("dh,nl", GEOS)
def test_pinv_chain_peaky(dh, nl):
    """Sharpened attention (q x 8, as make_golden_r2.py's peaky case): A2 from landmark logits with
    q~ scaled by 8; Z within the 1e-3 the existing peaky chain case allows, dL/ds finite (printed)."""
    from oracle.nystrom_ref import moore_penrose_iter_pinv
    g = _gen(5, dh)
    ql = torch.randn(NBH, nl, dh, generator=g, dtype=torch.float64) * 0.2 * 8.0
    kl = torch.randn(NBH, nl, dh, generator=g, dtype=torch.float64) * 0.2
    s64 = (ql @ kl.transpose(1, 2)).requires_grad_()
    z_ref = moore_penrose_iter_pinv(torch.softmax(s64, -1), 6)
    gz = torch.randn(NBH, nl, nl, generator=g, dtype=torch.float64) * 1e-3
    z_ref.backward(gz)
    z, ds = _chain(dh, nl, s64, gz)
    print(f"ds={_rel(ds, s64.grad):.3e}")
    assert torch.isfinite(ds).all()
    _check({"z": (z, z_ref.detach(), "rel")}, {"z": 1e-3})


def _mm_inputs(dh, nl, ta):
    g = _gen(6, dh, ta)
    A = torch.randn(NBH, nl, nl, generator=g) * 0.1
    Bm = torch.randn(NBH, nl, dh, generator=g)
    E1 = torch.randn(NBH, nl, dh, generator=g)
    return A, Bm, E1


def _mm_eval(A, Bm, E1, ta, e1, dtype):
    A, Bm, E1 = (t.to(dtype) for t in (A, Bm, E1))
    return (A.transpose(1, 2) if ta else A) @ Bm + e1 * E1


# (dh, ta) -> (bound with the addend, bound without): 4 x the fp32 torch evaluation's error against
# fp64 on the same inputs, measured on the CPU (relative to the largest entry):
#   (32, 0) 3.920e-7 / 4.163e-7   (32, 1) 5.063e-7 / 5.336e-7
#   (48, 0) 4.005e-7 / 3.896e-7   (48, 1) 4.446e-7 / 5.283e-7
_MM_BOUND = {(32, 0): (1.568e-6, 1.665e-6), (32, 1): (2.025e-6, 2.134e-6),
             (48, 0): (1.602e-6, 1.558e-6), (48, 1): (1.778e-6, 2.113e-6)}


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("dh,nl", GEOS)
def test_mm(dh, nl, ta):
    """C = op(A) B + e1 E1 (Y = Z W, dW = Z^T dY, dq~, dk~), in place on E1 as the engine's dk~ update."""
    L, (p, st) = _L(), _ps()
    A, Bm, E1 = _mm_inputs(dh, nl, ta)
    ref = _mm_eval(A, Bm, E1, ta, 0.5, torch.float64)
    print(f"fp32 torch: {_rel(_mm_eval(A, Bm, E1, ta, 0.5, torch.float32), ref):.3e}")
    Ad, Bd, Ed = _dev(A, Bm, E1)
    out = _nan(NBH, nl, dh)
    L.call("tm_nysg_mm", dh, nl, p(Ad), ta, p(Bd), p(Ed), C.c_float(0.5), p(out), NBH, st())
    L.call("tm_nysg_mm", dh, nl, p(Ad), ta, p(Bd), p(Ed), C.c_float(0.5), p(Ed), NBH, st())   # C = E1
    plain = _nan(NBH, nl, dh)
    L.call("tm_nysg_mm", dh, nl, p(Ad), ta, p(Bd), None, C.c_float(0.0), p(plain), NBH, st())
    torch.cuda.synchronize()
    assert torch.equal(out, Ed)
    _check({"c": (out.cpu(), ref, "rel"), "plain": (plain.cpu(), _mm_eval(A, Bm, E1, ta, 0.0, torch.float64), "rel")},
           {"c": _MM_BOUND[(dh, ta)][0], "plain": _MM_BOUND[(dh, ta)][1]})


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_a1_fwd(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(7, dh, n)
    q = torch.randn(NBH, n, dh, generator=g) * 0.3
    v = torch.randn(NBH, n, dh, generator=g)
    kl = torch.randn(NBH, nl, dh, generator=g) * 0.3
    y = torch.randn(NBH, nl, dh, generator=g)
    wconv = torch.randn(NH, TAPS, generator=g) * 0.1
    s = q.double() @ kl.double().transpose(1, 2)
    o = torch.softmax(s, -1) @ y.double() + _conv(v.double(), wconv.double(), NH)
    merged, lse = _nan(NBH // NH, n, NH * dh), _nan(NBH, n)
    qd, vd, kd, yd, wd = _dev(q, v, kl, y, wconv)
    L.call("tm_nysg_a1_fwd", dh, nl, p(qd), p(vd), p(kd), p(yd), p(wd), NBH, NH, n, p(merged), p(lse), st())
    torch.cuda.synchronize()
    _check({"merged": (merged.cpu(), heads_to_cols(o, NH), "rel"), "lse1": (lse.cpu(), torch.logsumexp(s, -1), "abs")},
           {"merged": 1.08e-6, "lse1": 3.61e-6})


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_conv_bwd(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(8, dh, n)
    nbags = NBH // NH
    dO = torch.randn(nbags, n, NH * dh, generator=g) * 0.5
    O = torch.randn(nbags, n, NH * dh, generator=g)
    v = torch.randn(NBH, n, dh, generator=g)
    wconv = torch.randn(NH, TAPS, generator=g) * 0.1
    v64, w64 = v.double().requires_grad_(), wconv.double().requires_grad_()
    conv = _conv(v64, w64, NH)
    dOh = _cols_to_heads(dO.double(), NH)
    ref_dv, ref_dw = torch.autograd.grad(conv, (v64, w64), dOh)
    ref_d1 = (dOh * (_cols_to_heads(O.double(), NH) - conv.detach())).sum(-1)
    dv, d1, dw = _nan(NBH, n, dh), _nan(NBH, n), _nan(NH * TAPS)
    work = torch.empty(L.query("tm_nysg_conv_bwd_workspace", dh, nl, nbags, NH, n) // 4 + 16, device=DEV)
    dOd, Od, vd, wd = _dev(dO, O, v, wconv)
    L.call("tm_nysg_conv_bwd", dh, nl, p(dOd), p(Od), p(vd), p(wd), NBH, NH, n, p(dv), p(d1), p(work), p(dw), None,
           st())
    torch.cuda.synchronize()
    _check({"dv": (dv.cpu(), ref_dv, "rel"), "d1": (d1.cpu(), ref_d1, "abs"), "dw": (dw.cpu().view(NH, TAPS), ref_dw, "rel")},
           {"dv": 8.81e-7, "d1": 9.79e-6, "dw": 9.98e-7})


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_a1_bwd(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(9, dh, n)
    q = torch.randn(NBH, n, dh, generator=g) * 0.3
    kl = torch.randn(NBH, nl, dh, generator=g) * 0.3
    y = torch.randn(NBH, nl, dh, generator=g)
    dm = torch.randn(NBH // NH, n, NH * dh, generator=g) * 0.1
    d1 = torch.randn(NBH, n, generator=g) * 0.05
    s = q.double() @ kl.double().transpose(1, 2)
    lse = torch.logsumexp(s, -1).float()                    # a consistent softmax
    pr = torch.exp(s - lse.double()[..., None])
    dOh = _cols_to_heads(dm.double(), NH)
    dS = pr * (dOh @ y.double().transpose(1, 2) - d1.double()[..., None])
    dq, dkl, dy = _nan(NBH, n, dh), _nan(NBH, nl, dh), _nan(NBH, nl, dh)
    work = torch.empty(L.query("tm_nysg_a1_bwd_workspace", dh, nl, NBH, n) // 4 + 16, device=DEV)
    qd, kd, yd, dmd, lsed, d1d = _dev(q, kl, y, dm, lse, d1)
    L.call("tm_nysg_a1_bwd", dh, nl, p(qd), p(dmd), p(kd), p(yd), p(lsed), p(d1d), NBH, NH, n, p(dq), p(work), p(dkl),
           p(dy), None, st())
    torch.cuda.synchronize()
    _check({"dq": (dq.cpu(), dS @ kl.double(), "rel"), "dkl": (dkl.cpu(), dS.transpose(1, 2) @ q.double(), "rel"),
            "dy": (dy.cpu(), pr.transpose(1, 2) @ dOh, "rel")}, {"dq": 2.78e-6, "dkl": 3.03e-6, "dy": 3.29e-6})


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_a3_bwd(dh, nl, n):
    L, (p, st) = _L(), _ps()
    g = _gen(10, dh, n)
    ql = torch.randn(NBH, nl, dh, generator=g) * 0.3
    dw = torch.randn(NBH, nl, dh, generator=g) * 0.1
    k = torch.randn(NBH, n, dh, generator=g) * 0.3
    v = torch.randn(NBH, n, dh, generator=g)
    lse, _, ref_dk, ref_dv, ref_dql = a3_bwd_ref(ql, dw, k, v)
    w = torch.softmax(ql.double() @ k.double().transpose(1, 2), -1) @ v.double()
    dv0 = torch.randn(NBH, n, dh, generator=g) * 0.1       # the conv backward's dv, accumulated into (+=)
    dk, dql = _nan(NBH, n, dh), _nan(NBH, nl, dh)
    work = torch.empty(L.query("tm_nysg_a3_bwd_workspace", dh, nl, NBH, n) // 4 + 16, device=DEV)
    qd, dwd, wd, kd, vd, lsed, dv = _dev(ql, dw, w, k, v, lse, dv0)
    L.call("tm_nysg_a3_bwd", dh, nl, p(qd), p(dwd), p(wd), p(kd), p(vd), p(lsed), NBH, n, p(dk), p(dv), p(work), p(dql),
           None, st())
    torch.cuda.synchronize()
    _check({"dk": (dk.cpu(), ref_dk, "rel"), "dv": (dv.cpu(), ref_dv + dv0.double(), "rel"), "dql": (dql.cpu(), ref_dql, "rel")},
           {"dk": 3.16e-6, "dv": 3.24e-6, "dql": 2.08e-6})


def _assemble_eval(dq, dql, dk, dkl, dv, l, scale, dtype):
    dq, dql, dk, dkl, dv = (t.to(dtype) for t in (dq, dql, dk, dkl, dv))
    inv_l = torch.tensor(1.0 / l, dtype=dtype) if dtype == torch.float64 else torch.tensor(1.0, dtype=dtype) / l
    qp = scale * (dq + dql.repeat_interleave(l, dim=1) * inv_l)
    kp = dk + dkl.repeat_interleave(l, dim=1) * inv_l
    return torch.cat([heads_to_cols(t, NH) for t in (qp, kp, dv)], dim=-1)


# 4 x the fp32 torch evaluation's error against fp64 (CPU, relative to the largest entry): measured
# 3.703e-8, 4.602e-8, 4.823e-8 at (32, 128) and 3.766e-8, 4.470e-8, 4.479e-8 at (48, 192) for
# n = nl, 2 nl, 5 nl; the bound is 4 x the smallest
_ASSEMBLE_BOUND = 1.48e-7


@pytest.mark.parametrize("dh,nl,n", _cases())
def test_assemble_dqkv(dh, nl, n):
    L, (p, st) = _L(), _ps()
    from transmil_deepgraft_amd._lib import F32, BF16
    g = _gen(11, dh, n)
    dq, dk, dv = (torch.randn(NBH, n, dh, generator=g) for _ in range(3))
    dql, dkl = (torch.randn(NBH, nl, dh, generator=g) for _ in range(2))
    l, scale, nbags = n // nl, dh ** -0.5, NBH // NH
    ref = _assemble_eval(dq, dql, dk, dkl, dv, l, scale, torch.float64)
    print(f"fp32 torch: {_rel(_assemble_eval(dq, dql, dk, dkl, dv, l, np.float32(scale).item(), torch.float32), ref):.3e}")
    ins = _dev(dq, dql, dk, dkl, dv)
    o32 = _nan(nbags, n, 3 * NH * dh)
    o16 = torch.zeros(nbags, n, 3 * NH * dh, dtype=torch.bfloat16, device=DEV)
    L.call("tm_nysg_assemble_dqkv", dh, nl, F32, *(p(t) for t in ins), nbags, NH, n, C.c_float(scale), p(o32), st())
    L.call("tm_nysg_assemble_dqkv", dh, nl, BF16, *(p(t) for t in ins), nbags, NH, n, C.c_float(scale), p(o16), st())
    torch.cuda.synchronize()
    _check({"dqkv": (o32.cpu(), ref, "rel")}, {"dqkv": _ASSEMBLE_BOUND})
    assert torch.equal(o16.cpu(), o32.cpu().to(torch.bfloat16))      # the same values, rounded once


# ----------------------------------------------------------------------------- NystromAttention module
@pytest.mark.parametrize("dim,dh,nl,S,B", [(256, 32, 128, 1, 1), (256, 32, 128, 128, 1), (256, 32, 128, 129, 1),
                                           (256, 32, 128, 500, 1), (256, 32, 128, 300, 2),
                                           (384, 48, 192, 1, 1), (384, 48, 192, 192, 1), (384, 48, 192, 193, 1),
                                           (384, 48, 192, 500, 1), (384, 48, 192, 300, 2)])
def test_nystrom_attention_fp32_vs_oracle(dim, dh, nl, S, B):
    """Forward and backward against oracle.nystrom_ref in fp64, eval mode; the tolerances of the
    (64, 256) standalone test (output 1e-4, gradients 1e-3, relative to each tensor's largest entry)."""
    from oracle.nystrom_ref import NystromAttention as Ref
    from transmil_deepgraft_amd.nystrom_attention import NystromAttention
    torch.manual_seed(S + dim)
    ref = Ref(dim=dim, dim_head=dh, heads=8, num_landmarks=nl, pinv_iterations=6, residual=True).double().eval()
    with torch.no_grad():
        ref.res_conv.weight.mul_(3.0)
    ours = NystromAttention(dim=dim, dim_head=dh, heads=8, num_landmarks=nl, pinv_iterations=6,
                            residual=True).to(DEV).eval()
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.compute_dtype = torch.float32
    x = torch.randn(B, S, dim, dtype=torch.float64)
    xr = x.clone().requires_grad_()
    out_ref = ref(xr)
    gy = torch.randn_like(out_ref)
    out_ref.backward(gy)
    xo = x.float().to(DEV).requires_grad_()
    out = ours(xo)
    out.backward(gy.float().to(DEV))
    errs = {"out": _rel(out.detach().cpu(), out_ref), "dx": _rel(xo.grad.cpu(), xr.grad)}
    for (n1, p1), (_, p2) in zip(ours.named_parameters(), ref.named_parameters()):
        errs[n1] = _rel(p1.grad.cpu(), p2.grad)
    print(" ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert errs.pop("out") < 1e-4
    assert all(e < 1e-3 for e in errs.values()), errs


# ----------------------------------------------------------------------------- whole model
def _pair(ncls, feat, out, dtype=torch.float32):
    from oracle.transmil_ref import TransMIL as Ref, deterministic_params_
    from transmil_deepgraft_amd.models import TransMIL
    torch.manual_seed(0)
    ref = deterministic_params_(Ref(ncls, feat, out), 2021).double().eval()
    ours = TransMIL(ncls, feat, out).to(DEV).eval()
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.set_compute_dtype(dtype)
    return ref, ours


def _ref64(ref, x, **kw):
    from oracle.transmil_ref import TransLayer
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self
    TransLayer.compute_attn = bool(kw.get("return_attn", False))
    try:
        return ref(x.double(), **kw)
    finally:
        torch.Tensor.float = orig
        TransLayer.compute_attn = True


def _ours_forward_backward(ours, x, label, ncls):
    logits = ours(x.float().to(DEV))
    y = torch.tensor([label] * x.shape[0], device=DEV)
    loss = torch.nn.CrossEntropyLoss()(logits, torch.nn.functional.one_hot(y, ncls).float())
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().cpu(), {n: p.grad.detach().cpu() for n, p in ours.named_parameters()}


def _grad_errors(go, gr):
    return {n: ((go[n].double() - torch.as_tensor(g).double()).abs().max()
                / torch.as_tensor(g).double().abs().max().clamp_min(1e-12)).item() for n, g in gr.items()}


@pytest.mark.parametrize("ncls,feat,out,N,B", [(2, 2048, 256, 300, 1), (3, 2048, 384, 300, 2), (5, 384, 384, 257, 1),
                                               (2, 2048, 256, 20, 3), (3, 384, 384, 1, 1), (2, 256, 256, 127, 1),
                                               (3, 384, 384, 1024, 2)])
def test_transmil_fp32_logits_and_grads(ncls, feat, out, N, B):
    """The harness and bounds of test_parity_gpu.test_transmil_fp32_logits_and_grads: logits within
    1e-4 of the fp64 oracle, equal argmax, every gradient within 2e-3 of its largest entry."""
    ref, ours = _pair(ncls, feat, out)
    x = torch.from_numpy(bag_input(N, feat, 2021 + 1000 + N, B))
    lr = _ref64(ref, x)
    y = torch.tensor([1] * B)
    torch.nn.CrossEntropyLoss()(lr, torch.nn.functional.one_hot(y, ncls).double()).backward()
    gr = {n: p.grad.detach() for n, p in ref.named_parameters()}
    lo, go = _ours_forward_backward(ours, x, 1, ncls)
    errs = _grad_errors(go, gr)
    print(f"logits={(lo.double() - lr.detach()).abs().max().item():.3e} grads_max={max(errs.values()):.3e}")
    np.testing.assert_allclose(lo.numpy(), lr.detach().numpy(), rtol=0, atol=1e-4)
    assert torch.equal(lo.argmax(1), lr.argmax(1))
    bad = [(n, e) for n, e in errs.items() if e > 2e-3]
    assert not bad, bad


FIXTURES = ["dims256_fc2048_n300", "dims384_c3_n300_b2"]


def _fixture_pair(name, dtype):
    fx = load(name)
    meta = json.loads(str(fx["meta"]))
    _, ours = _pair(meta["n_classes"], meta["feat"], meta["out"], dtype)
    x = torch.from_numpy(bag_input(meta["n"], meta["feat"], 2021 + 1000 + meta["n"], meta["batch"]))
    return fx, meta, ours, x


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_reference_fixtures_fp32(name):
    """The reference's own code/models/TransMIL.py (make_golden_dims.py): logits within 1e-4 of the
    fixture's fp64 logits, equal argmax, the small gradients within 2e-3."""
    fx, meta, ours, x = _fixture_pair(name, torch.float32)
    lo, go = _ours_forward_backward(ours, x, meta["label"], meta["n_classes"])
    gr = {k[len("grad."):-len(".f64")]: v for k, v in fx.items() if k.startswith("grad.") and k.endswith(".f64")}
    assert set(gr) == {"cls_token", "norm.weight", "norm.bias", "_fc.weight", "_fc.bias"}
    errs = _grad_errors(go, gr)
    print(f"logits={np.abs(lo.numpy() - fx['logits.f64']).max():.3e} grads_max={max(errs.values()):.3e}")
    np.testing.assert_allclose(lo.numpy(), fx["logits.f64"], rtol=0, atol=1e-4)
    assert (lo.numpy().argmax(1) == fx["logits.f64"].argmax(1)).all()
    bad = [(n, e) for n, e in errs.items() if e > 2e-3]
    assert not bad, bad


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_mode_close_to_reference(name):
    """bf16 mode (bf16 projections, fp32 core): logits within 5e-2 of the fixture's fp64 logits,
    equal argmax (margins 1.82 and 0.67); one train-mode backward with every gradient finite and
    non-zero."""
    fx, meta, ours, x = _fixture_pair(name, torch.bfloat16)
    with torch.no_grad():
        lo = ours(x.to(DEV)).cpu().numpy()
    print(f"logits={np.abs(lo - fx['logits.f64']).max():.3e}")
    np.testing.assert_allclose(lo, fx["logits.f64"], rtol=0, atol=5e-2)
    assert (lo.argmax(1) == fx["logits.f64"].argmax(1)).all()
    ours.train()
    y = torch.full((meta["batch"],), meta["label"], device=DEV)
    loss = torch.nn.CrossEntropyLoss()(ours(x.to(DEV)), torch.nn.functional.one_hot(y, meta["n_classes"]).float())
    loss.backward()
    for n, p in ours.named_parameters():
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n


@pytest.mark.parametrize("ncls,feat,out,N", [(2, 2048, 256, 300), (3, 384, 384, 300)])
def test_return_attn_rows(ncls, feat, out, N):
    """(logits, (AttentionMap, padding)) with the reference's literal padding 256 - S % 256; rows 0,
    the class-token row (-S) % m and n - 1 through tm_nysg_attn_row (no n x n matrix) against the
    oracle's full product, at the tolerance of test_attention_map_rows_match_the_full_product."""
    from transmil_deepgraft_amd.nystrom_attention import AttentionMap
    ref, ours = _pair(ncls, feat, out)
    x = torch.from_numpy(bag_input(N, feat, 2021 + 1000 + N))
    with torch.no_grad():
        lr, (ar, pr) = _ref64(ref, x, return_attn=True)
        lo, (attn, pad) = ours(x.to(DEV), return_attn=True)
    G = int(np.ceil(np.sqrt(N)))
    S, m = G * G + 1, out // 2
    n = -(-S // m) * m
    assert isinstance(attn, AttentionMap) and pad == pr == 256 - S % 256
    assert tuple(attn.shape) == tuple(ar.shape) == (1, 8, n, n)
    rows = [0, (-S) % m, n - 1]
    got = [attn[0, :, r, :].cpu().double() for r in rows]
    assert attn._full is None                                 # no n x n matrix so far
    assert torch.equal(attn.row(rows[1])[0].cpu().double(), got[1])
    full = attn.full().cpu().double()
    errs = {}
    for r, g in zip(rows, got):
        assert g.shape == (8, n)
        errs[f"oracle{r}"] = ((g - ar[0, :, r, :]).abs().max() / ar[0, :, r, :].abs().max()).item()
        errs[f"full{r}"] = ((g - full[0, :, r, :]).abs().max() / full[0, :, r, :].abs().max()).item()
    print(" ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert all(e < 1e-5 for e in errs.values()), errs


def test_norm_hook_sees_the_narrow_width():
    _, ours = _pair(2, 2048, 256)
    seen = []
    h = ours.norm.register_forward_hook(lambda _m, _i, o: seen.append(tuple(o.shape)))
    try:
        with torch.no_grad():
            ours(torch.from_numpy(bag_input(300, 2048, 5, 2)).to(DEV))
    finally:
        h.remove()
    assert seen == [(2, 18 * 18 + 1, 256)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_task_step(dtype):
    """TransMILTask.training_step at out_features 384 (forward_ce declines: forward + the task's own
    CE), eager: a finite loss equal to CE of forward under the same dropout seed, and one optimizer
    step moves every parameter."""
    from transmil_deepgraft_amd.interface import TransMILTask
    _, model = _pair(3, 2048, 384, dtype)
    model.train()
    task = TransMILTask(model)
    opt = task.configure_optimizers()[0][0]
    x = torch.from_numpy(bag_input(300, 2048, 11, 2)).to(DEV)
    label = torch.tensor([1, 2], device=DEV)
    assert model.forward_ce(x, label) is None
    counters = [m._dropout_counter for m in (model.layer1.attn, model.layer2.attn)]
    start = [c.clone() for c in counters]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss = task.training_step((x, label, None))
    assert loss.shape == (1,) and torch.isfinite(loss).all()
    for c, s in zip(counters, start):
        c.copy_(s)
    with torch.no_grad():
        ce = torch.nn.CrossEntropyLoss()(model(x), torch.nn.functional.one_hot(label, 3).float())
    assert abs(loss.item() - ce.item()) < 1e-6 * max(1.0, abs(ce.item()))
    task.backward(loss)
    opt.step()
    torch.cuda.synchronize()
    same = [n for n, p in model.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not same, same
