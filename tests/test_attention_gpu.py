"""The softmax-attention kernels (attention.hip) on the MI355X through the C ABI with the packed
to_qkv layout (row_stride = 3*H*64), against the fp64 restatement of tests/attention_refs.py.

Operands are bf16-representable as the kernel reads them (randn, q times its multiplier, then
rounded), so the TM_BF16 bounds measure the kernel's arithmetic (bf16 P and dS, fp32 accumulation)
and not the rounding of its inputs; dout is an operand of the backward and is rounded likewise.
Every test prints the figures it then asserts on (pytest -s shows them)."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_refs as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = 7.0
SCALE = 0.125
DH = 64

SHAPES = [(1, 8, 1), (1, 8, 2), (2, 8, 63), (1, 8, 64), (3, 8, 65), (1, 1, 129), (2, 8, 201), (1, 8, 1025),
          (1, 8, 2049)]
MULTS = [1, 8, 24]
MODES = [torch.float32, torch.bfloat16]
# the compute modes TransformerMIL runs on the HIP attention (the attention section)
WIRED = [torch.float32, torch.bfloat16]

# (project bound fp32, bound bf16) per quantity; fp32 also admits 4x the fp32 torch evaluation's error
BOUNDS = {"out": (1e-5, 2e-2), "lse": (1e-4, 1e-3), "dq": (1e-4, 2e-2), "dk": (1e-4, 2e-2), "dv": (1e-4, 2e-2)}


def _lib():
    from transmil_deepgraft_amd import _lib
    return _lib


def _stream():
    from transmil_deepgraft_amd.engine import _stream
    return _stream()


def _tt(dtype):
    return _lib().BF16 if dtype == torch.bfloat16 else _lib().F32


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _abs(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _report(name, value):
    print(f"[measured] {name} = {value:.3e}" if isinstance(value, float) else f"[measured] {name} = {value}")


def _bound(what, dtype, e32=None):
    f32, b16 = BOUNDS[what]
    if dtype == torch.bfloat16:
        return b16
    return max(f32, 4 * e32) if e32 is not None else f32


def _smax(q, k):
    return ((q.double() @ k.double().transpose(-1, -2)) * SCALE).max().item()


def _operands(B, H, n, mult):
    """q (times mult), k, v, dout from a CPU generator seeded per case.  At mult = 24 and n >= 63 the
    case is the one whose largest scaled score is above 100 (exp overflows fp32 from 88.7): the
    first of the case's seeds that gives it (the small one-head shapes need a second draw)."""
    for draw in range(16):
        g = torch.Generator().manual_seed(1000000 * draw + 100000 * mult + 100 * n + 10 * B + H)

        def rnd(m=1):
            return (torch.randn(B, H, n, DH, generator=g) * m).bfloat16().float()
        q, k, v, dout = rnd(mult), rnd(), rnd(), rnd()
        if not (mult == 24 and n >= 63) or _smax(q, k) > 100.0:
            return q, k, v, dout
    raise AssertionError(f"no draw of case {(B, H, n, mult)} reaches a scaled score above 100")


@functools.lru_cache(maxsize=None)
def _case(B, H, n, mult):
    """Operands, the fp64 reference and the fp32 torch evaluation's own error, computed once."""
    q, k, v, dout = _operands(B, H, n, mult)
    out, lse = A.attn_fwd(q, k, v, SCALE)
    dq, dk, dv = A.attn_bwd(q, k, v, out, lse, dout, SCALE)
    ref = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)
    o32, l32 = A.attn_fwd(q, k, v, SCALE, torch.float32)
    g32 = A.attn_bwd(q, k, v, o32, l32, dout, SCALE, torch.float32)
    e32 = {"out": _rel(o32, out), "lse": _abs(l32, lse)}
    for name, got in zip(("dq", "dk", "dv"), g32):
        e32[name] = _rel(got, ref[name]) if n > 1 or name == "dv" else 0.0
    return SimpleNamespace(B=B, H=H, n=n, q=q, k=k, v=v, dout=dout, ref=ref, e32=e32,
                           smax=_smax(q, k))


def _guarded(rows, width, fill=NAN):
    """[rows, width] filled with `fill`, with a sentinel guard row behind it in the same allocation."""
    buf = torch.full(((rows + 1) * width,), SENTINEL, device=DEV)
    buf[:rows * width] = fill
    return buf, buf[:rows * width].view(rows, width), buf[rows * width:]


def _run(q, k, v, dout, dtype):
    """tm_attn_fwd + tm_attn_bwd on [B, H, n, 64] CPU operands; outputs NaN-prefilled and guarded."""
    from transmil_deepgraft_amd.engine import _p
    lib = _lib()
    B, H, n, _ = q.shape
    inner = H * DH
    qkv = A.pack_qkv(q, k, v).to(DEV)
    do = A.merge_heads(dout).to(DEV)
    ob, out, og = _guarded(B * n, inner)
    lb, lse, lg = _guarded(B * H, n)
    gb, dqkv, gg = _guarded(B * n, 3 * inner)
    ptr = [C.c_void_p(qkv.data_ptr() + i * inner * 4) for i in range(3)]
    lib.call("tm_attn_fwd", _tt(dtype), *ptr, B, H, n, 3 * inner, C.c_float(SCALE), _p(out), _p(lse), _stream())
    wbytes = lib.query("tm_attn_bwd_workspace", B, H, n)
    wb, work, wg = _guarded(1, wbytes // 4)
    lib.call("tm_attn_bwd", _tt(dtype), *ptr, _p(out), _p(lse), _p(do), B, H, n, 3 * inner, C.c_float(SCALE),
             _p(work), _p(dqkv), _stream())
    torch.cuda.synchronize()
    guards_ok = all(bool((g == SENTINEL).all()) for g in (og, lg, gg, wg))
    dq, dk, dv = A.unpack_qkv(dqkv.view(B, n, 3 * inner).cpu(), H)
    return SimpleNamespace(out=A.split_heads(out.view(B, n, inner).cpu(), H), lse=lse.view(B, H, n).cpu(), dq=dq,
                           dk=dk, dv=dv, raw=(out.clone(), lse.clone(), dqkv.clone()), guards_ok=guards_ok)


# ============================================================================= a, b. against fp64; writes
@pytest.mark.parametrize("dtype", MODES, ids=_name)
@pytest.mark.parametrize("mult", MULTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_H%d_n%d" % s)
def test_kernels_against_fp64(shape, mult, dtype):
    B, H, n = shape
    c = _case(B, H, n, mult)
    if mult == 24 and n >= 63:
        assert c.smax > 100.0, c.smax                       # exp overflows fp32 without the running max
    got = _run(c.q, c.k, c.v, c.dout, dtype)
    tag = f"{_name(dtype)} B{B} H{H} n{n} x{mult}"
    _report(f"{tag} max scaled score", c.smax)
    # b. every output element written and finite, nothing written behind the outputs
    for t in got.raw:
        assert bool(torch.isfinite(t).all()), tag
    assert got.guards_ok, tag
    errs, bounds = {}, {}
    for what in ("out", "lse", "dq", "dk", "dv"):
        if n == 1 and what in ("dq", "dk"):
            continue
        errs[what] = _abs(getattr(got, what), c.ref[what]) if what == "lse" else _rel(getattr(got, what), c.ref[what])
        bounds[what] = _bound(what, dtype, c.e32[what])
    for what in errs:
        _report(f"{tag} {what} err", errs[what])
        _report(f"{tag} {what} bound (fp32 torch evaluation: {c.e32[what]:.3e})", bounds[what])
    if n == 1:
        # one key: P = 1, so out = v, dv = dout and dq = dk = 0 exactly in the reference
        e_ov, e_dv = _rel(got.out, c.v), _rel(got.dv, c.dout)
        zq = got.dq.abs().max().item() / c.dout.abs().max().item()
        zk = got.dk.abs().max().item() / c.dout.abs().max().item()
        for name, val in (("out vs v", e_ov), ("dv vs dout", e_dv), ("max|dq|/max|dout|", zq),
                          ("max|dk|/max|dout|", zk)):
            _report(f"{tag} {name}", val)
        assert e_ov <= _bound("out", dtype) and e_dv <= _bound("out", dtype), tag
        assert zq <= 1e-5 and zk <= 1e-5, tag
    for what in errs:
        assert errs[what] <= bounds[what], f"{tag} {what}: {errs[what]:.3e} > {bounds[what]:.3e}"


# ============================================================================= c. reproducibility
@pytest.mark.parametrize("dtype", MODES, ids=_name)
@pytest.mark.parametrize("shape", [(2, 8, 201), (1, 8, 2049)], ids=lambda s: "B%d_H%d_n%d" % s)
def test_two_calls_are_bitwise_equal(shape, dtype):
    c = _case(*shape, 8)
    a = _run(c.q, c.k, c.v, c.dout, dtype)
    b = _run(c.q, c.k, c.v, c.dout, dtype)
    same = [torch.equal(x, y) for x, y in zip(a.raw, b.raw)]
    _report(f"{_name(dtype)} {shape} out / lse / dqkv bitwise equal over two calls", same)
    assert all(same)


# ============================================================================= d. the user's shape
def _sdpa_path(qkv, heads, dt):
    """The attention core as the model ran it before the HIP kernels: reshape, transpose, cast, SDPA."""
    import torch.nn.functional as F
    b, n, _ = qkv.shape
    q, k, v = (t.reshape(b, n, heads, -1).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(q.to(dt), k.to(dt), v.to(dt), scale=SCALE).float()
    return o.transpose(1, 2).reshape(b, n, -1)


@pytest.mark.parametrize("dtype", MODES, ids=_name)
def test_user_shape_agrees_with_sdpa_in_linear_memory(dtype):
    from transmil_deepgraft_amd import ops
    B, H, n = 1, 8, 8193
    q, k, v, dout = _operands(B, H, n, 1)
    qkv = A.pack_qkv(q, k, v).to(DEV).requires_grad_(True)
    do = A.merge_heads(dout).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.attention(qkv, H, SCALE, dtype)
    out.backward(do)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = B * H * n * n * 4 // 2
    _report(f"{_name(dtype)} (1, 8, 8193) peak memory over forward + backward [bytes]", peak)
    _report("half of one fp32 score matrix [bytes]", limit)
    assert peak < limit
    g_ours, qkv.grad = qkv.grad, None
    ref = _sdpa_path(qkv, H, dtype)
    ref.backward(do)
    torch.cuda.synchronize()
    tol = {what: 2 * _bound(what, dtype) for what in ("out", "dq", "dk", "dv")}
    errs = {"out": _rel(out.detach(), ref.detach())}
    for what, a, b in zip(("dq", "dk", "dv"), g_ours.chunk(3, dim=-1), qkv.grad.chunk(3, dim=-1)):
        errs[what] = _rel(a, b)
    for what in errs:
        _report(f"{_name(dtype)} (1, 8, 8193) {what} vs SDPA", errs[what])
    for what in errs:
        assert errs[what] <= tol[what], (what, errs[what], tol[what])


# ============================================================================= e. ops.attention under autograd
@pytest.mark.parametrize("dtype", MODES, ids=_name)
def test_ops_attention_autograd(dtype):
    from transmil_deepgraft_amd import ops
    B, H, n = 2, 8, 65
    q, k, v, w = _operands(B, H, n, 1)
    qkv = A.pack_qkv(q, k, v).to(DEV).requires_grad_(True)
    out = ops.attention(qkv, H, SCALE, dtype)
    assert out.shape == (B, n, H * DH) and out.dtype == torch.float32
    (out * A.merge_heads(w).to(DEV)).sum().backward()
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    ref = A.attn_plain(*leaves, SCALE)
    (ref * w.double()).sum().backward()
    errs = {"out": _rel(A.split_heads(out.detach().cpu(), H), ref.detach())}
    for what, got, leaf in zip(("dq", "dk", "dv"), A.unpack_qkv(qkv.grad.cpu(), H), leaves):
        errs[what] = _rel(got, leaf.grad)
    for what in errs:
        _report(f"{_name(dtype)} ops.attention B2 n65 {what} vs fp64 autograd", errs[what])
    for what in errs:
        assert errs[what] <= _bound(what, dtype), (what, errs[what])


# ============================================================================= f. wiring
@pytest.mark.parametrize("dtype", WIRED, ids=_name)
def test_transformermil_runs_without_sdpa(dtype, monkeypatch):
    import torch.nn.functional as F
    from golden_util import load, sibling_input
    from test_siblings_gpu import _loss, _ours

    def refuse(*a, **k):
        raise AssertionError("TransformerMIL called torch's scaled_dot_product_attention")
    monkeypatch.setattr(F, "scaled_dot_product_attention", refuse)
    name = "transformermil768_n200_b2"
    fx = load(name)
    ref, ours = _ours(name, dtype)
    x = torch.from_numpy(sibling_input(name))
    lo = ours(x.to(DEV))
    atol = 2e-4 if dtype == torch.float32 else 6e-2
    err = float(np.abs(lo.detach().cpu().numpy() - fx["logits"]).max())
    _report(f"{_name(dtype)} {name} max |logits - fixture| (atol {atol:g})", err)
    assert err <= atol
    _loss(lo, lo.shape[1]).backward()
    # the parameters the reference's own backward reaches
    _loss(ref(x), lo.shape[1]).backward()
    reached = 0
    for (pname, pr), po in zip(ref.named_parameters(), ours.parameters()):
        if pr.grad is None:
            continue
        reached += 1
        assert po.grad is not None and bool(torch.isfinite(po.grad).all()), pname
    _report(f"{_name(dtype)} {name} parameters with a finite gradient", reached)
    assert reached > 0
