"""Every field of the stage kernel's job descriptor (pinv_split.hip SJob, read once at kernel
entry), at the smallest chains where a wrong or stale field shows: iters = 1 (the F level built on
X^T with alpha_cpow), iters = 2 (the k = 1 Z_0 level, the c2 / c3 side outputs, the k = 0 backward
jobs, the two-term level, the DOT launch), head counts 1, 8 and 9 (9: not a multiple of 8), and
the step's own shape (8 heads, 6 iterations).  tm_pinv_fwd_split, tm_pinv_fwd_split_a3 and
tm_pinv_bwd_split against the exact-fp32 chain (tm_pinv_fwd / tm_pinv_bwd, prec 0) on the same
softmax-row inputs, with the bounds test_pinv_split_gpu.py uses for Z and the softmax-side gradient
(5e-4, 4e-3); two calls give identical bytes."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAT = 65536
A3_N = 512   # keys of the A3 partials the _a3 entry point combines beside the last level

CASES = [(nbh, iters) for nbh in (1, 8, 9) for iters in (1, 2)] + [(8, 6)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _api():
    from transmil_deepgraft_amd import _lib
    from transmil_deepgraft_amd.engine import _p, _stream
    return _lib, _p, _stream


def _split(x):
    _lib, _p, _stream = _api()
    y = torch.empty(2 * x.numel(), dtype=torch.bfloat16, device=DEV)
    _lib.call("tm_split_f32", _p(x), _p(y), x.numel(), _stream())
    return y


@functools.lru_cache(maxsize=None)
def _inputs(nbh, iters):
    g = torch.Generator().manual_seed(1000 * iters + nbh)
    X = torch.softmax(torch.randn(nbh, 256, 256, generator=g) * 0.3, dim=-1).to(DEV).contiguous()
    gz = (torch.randn(nbh, 256, 256, generator=g) * 1e-3).to(DEV).contiguous()
    return X, gz


@functools.lru_cache(maxsize=None)
def _fp32_chain(nbh, iters):
    """Z_iters and dL/ds of the exact-fp32 chain: computed once per case, never written again."""
    _lib, _p, _stream = _api()
    X, gz = _inputs(nbh, iters)
    saved = torch.empty(_lib.query("tm_pinv_saved_floats", nbh, iters), device=DEV)
    _lib.call("tm_pinv_fwd", _p(X), nbh, iters, 0, _p(saved), _stream())
    z = saved[iters * nbh * MAT:(iters + 1) * nbh * MAT].view(nbh, 256, 256).clone()
    work = torch.empty(_lib.query("tm_pinv_bwd_workspace_floats", nbh), device=DEV)
    dX = torch.empty(nbh, 256, 256, device=DEV)
    _lib.call("tm_pinv_bwd", _p(X), nbh, iters, 0, _p(saved), _p(gz.clone()), _p(work), _p(dX), _stream())
    ds = torch.empty_like(dX)
    _lib.call("tm_softmax_bwd_rows256", _p(X), _p(dX), _p(ds), nbh * 256, _stream())
    torch.cuda.synchronize()
    return z.cpu(), ds.cpu()


def _run_split(X, Xs, gz, nbh, iters, a3=None):
    """(saved, ds) of the split chain; a3 = (work, parts, w, lse): through tm_pinv_fwd_split_a3."""
    _lib, _p, _stream = _api()
    saved = torch.full((_lib.query("tm_pinv_split_saved_floats", nbh, iters),), float("nan"), device=DEV)
    if a3 is None:
        _lib.call("tm_pinv_fwd_split", _p(X), _p(Xs), nbh, iters, _p(saved), _stream())
    else:
        work3, parts, w, lse = a3
        _lib.call("tm_pinv_fwd_split_a3", _p(X), _p(Xs), nbh, iters, _p(saved), _p(work3), parts, _p(w), _p(lse),
                  _stream())
    work = torch.full((_lib.query("tm_pinv_bwd_split_workspace_floats", nbh),), float("nan"), device=DEV)
    _lib.call("tm_split_f32", _p(gz), _p(work), gz.numel(), _stream())
    ds = torch.full((nbh, 256, 256), float("nan"), device=DEV)
    _lib.call("tm_pinv_bwd_split", _p(X), _p(Xs), nbh, iters, _p(saved), _p(work), 1, _p(ds), _stream())
    torch.cuda.synchronize()
    return saved, ds


@pytest.mark.parametrize("nbh,iters", CASES)
def test_stage_descriptor_chain_vs_fp32(nbh, iters):
    _lib, _p, _stream = _api()
    from transmil_deepgraft_amd._lib import BF16
    X, gz = _inputs(nbh, iters)
    z_ref, ds_ref = _fp32_chain(nbh, iters)
    Xs = _split(X)
    zn = nbh * MAT

    saved, ds = _run_split(X, Xs, gz, nbh, iters)
    z = saved[:zn].view(nbh, 256, 256)
    assert torch.isfinite(saved).all() and torch.isfinite(ds).all()   # every saved slot was written
    ez, eds = _rel(z.cpu(), z_ref), _rel(ds.cpu(), ds_ref)
    print(f"nbh {nbh} iters {iters}: rel |Z - Z_fp32| {ez:.3e}, rel |ds - ds_fp32| {eds:.3e}")
    assert ez < 5e-4
    assert eds < 4e-3

    # the same calls again: identical bytes, in every saved matrix and in the gradient
    saved2, ds2 = _run_split(X, Xs, gz, nbh, iters)
    assert torch.equal(saved.view(torch.int32), saved2.view(torch.int32))
    assert torch.equal(ds.view(torch.int32), ds2.view(torch.int32))

    # the A3 combine row beside the last level: the chain's bytes do not move, W and lse3 are the
    # separate combine launch's
    g = torch.Generator().manual_seed(7 + nbh)
    ql = (torch.randn(nbh, 256, 64, generator=g) * 0.4).to(DEV)
    k = (torch.randn(nbh, A3_N, 64, generator=g) * 0.4).to(torch.bfloat16).to(DEV)
    v = torch.randn(nbh, A3_N, 64, generator=g).to(torch.bfloat16).to(DEV)
    work3 = torch.empty(_lib.query("tm_nys_a3_workspace", nbh, A3_N) // 4 + 16, device=DEV)
    w_ref = torch.full((nbh, 256, 64), float("nan"), device=DEV)
    lse_ref = torch.full((nbh, 256), float("nan"), device=DEV)
    _lib.call("tm_nys_a3_fwd", BF16, _p(ql), _p(k), _p(v), nbh, A3_N, _p(work3), _p(w_ref), _p(lse_ref), _stream())
    _lib.call("tm_nys_a3_fwd", BF16, _p(ql), _p(k), _p(v), nbh, A3_N, _p(work3), _p(None), _p(None), _stream())
    w, lse = torch.full_like(w_ref, float("nan")), torch.full_like(lse_ref, float("nan"))
    saved3, ds3 = _run_split(X, Xs, gz, nbh, iters, a3=(work3, _lib.query("tm_nys_a3_partials", nbh, A3_N), w, lse))
    assert torch.equal(w, w_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(saved.view(torch.int32), saved3.view(torch.int32))
    assert torch.equal(ds.view(torch.int32), ds3.view(torch.int32))
