"""Softmax attention (attention.hip) without a GPU: the fp64 restatement the kernel tests compare
with equals autograd, the C entry points refuse bad arguments before touching a pointer, and the
backward's workspace is linear in n."""
import ctypes as C

import pytest
import torch

import attention_refs as A


def test_restatement_backward_equals_autograd():
    g = torch.Generator().manual_seed(5)
    B, H, n, dh, scale = 2, 3, 37, 64, 0.125
    q, k, v, dout = (torch.randn(B, H, n, dh, generator=g, dtype=torch.float64) for _ in range(4))
    q = q * 4
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ref = A.attn_plain(*leaves, scale)
    ref.backward(dout)
    out, lse = A.attn_fwd(q, k, v, scale)
    dq, dk, dv = A.attn_bwd(q, k, v, out, lse, dout, scale)
    errs = {"out": (out - ref.detach()).abs().max().item()}
    for name, got, leaf in zip(("dq", "dk", "dv"), (dq, dk, dv), leaves):
        errs[name] = (got - leaf.grad).abs().max().item()
    lse_ref = torch.logsumexp((q @ k.transpose(-1, -2)) * scale, dim=-1)
    errs["lse"] = (lse - lse_ref).abs().max().item()
    print("[measured] restatement vs fp64 autograd, max abs:", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


def _fwd(B, H, n, stride):
    from transmil_deepgraft_amd import _lib
    _lib.call("tm_attn_fwd", _lib.F32, None, None, None, B, H, n, stride, C.c_float(0.125), None, None, None)


def _bwd(B, H, n, stride):
    from transmil_deepgraft_amd import _lib
    _lib.call("tm_attn_bwd", _lib.F32, None, None, None, None, None, None, B, H, n, stride, C.c_float(0.125),
              None, None, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("args, msg", [
    ((1, 8, 0, 1536), "n must be positive"),
    ((1, 0, 5, 1536), "H must be positive"),
    ((1, 8, 5, 511), "row_stride must be at least H\\*64"),
    ((1, 8, 5, 1538), "row_stride must be a multiple of 4"),
], ids=["n0", "H0", "stride_small", "stride_mod4"])
def test_bad_arguments_are_refused_before_any_pointer_is_touched(call, args, msg):
    from transmil_deepgraft_amd import _lib
    with pytest.raises(RuntimeError, match=msg):
        call(*args)
    assert _lib.last_error()
    # well-formed sizes with null pointers: refused too, still without dereferencing anything
    with pytest.raises(RuntimeError, match="null pointer"):
        call(1, 8, 5, 1536)


@pytest.mark.parametrize("n", [1025, 8193])
def test_backward_workspace_is_linear_in_n(n):
    from transmil_deepgraft_amd import _lib
    B, H = 1, 8
    w1 = _lib.query("tm_attn_bwd_workspace", B, H, n)
    w2 = _lib.query("tm_attn_bwd_workspace", B, H, 2 * n)
    print(f"[measured] tm_attn_bwd_workspace(1, 8, {n}) = {w1} B, (1, 8, {2 * n}) = {w2} B")
    assert w1 >= B * H * n * 4          # at least the D rows
    assert w2 <= 2 * w1 + 4096
