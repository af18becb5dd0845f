"""Kernel-level checks of the bf16 training step's backward on the MI355X: the fused A3 backward,
the class-row kernels (clsrow.hip), the dropout mask shared by four kernels, the LayerNorm backward
in the step's form and the bf16 slab reduce, each called through the C ABI as engine.py calls it and
compared with the fp64 restatements of tests/kernel_refs.py (or bit for bit with a second kernel
path).  Every test prints the figures it then asserts on (pytest -s shows them)."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = 7.0


def _lib():
    from transmil_deepgraft_amd import _lib
    return _lib


def _eng():
    from transmil_deepgraft_amd.engine import _p, _stream
    return _p, _stream


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _report(name, value):
    print(f"[measured] {name} = {value:.3e}" if isinstance(value, float) else f"[measured] {name} = {value}")


def _tt(dtype):
    from transmil_deepgraft_amd._lib import BF16, F32
    return BF16 if dtype == torch.bfloat16 else F32


def _ulp_bf16(x):
    return torch.exp2(torch.floor(torch.log2(x.float().abs().clamp_min(1e-30))) - 7)


def _ulp_f32(x):
    return torch.exp2(torch.floor(torch.log2(x.float().abs().clamp_min(1e-30))) - 23)


def _dev(*ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


class _Queue:
    """A caller-owned tm_reduce_queue for one call (the engine's deferred form)."""

    def __enter__(self):
        self.h = C.c_void_p(_lib().lib().tm_reduce_queue_create())
        assert self.h
        return self

    def pending(self):
        return _lib().lib().tm_reduce_queue_pending(self.h)

    def flush(self):
        _, _stream = _eng()
        _lib().call("tm_reduce_flush", self.h, _stream())

    def __exit__(self, *exc):
        _lib().lib().tm_reduce_queue_destroy(self.h)
        return False


# ============================================================================= a. tm_nys_a3_bwd_fused
@functools.lru_cache(maxsize=2)
def _a3_case(nbh, n):
    """Operands (scaled as test_a3_bwd_bf16_even_split) and their fp64 backward, shared by the
    windows of one shape; dk~ and the conv dv are scaled to the size of dK and dV so that neither
    term of the epilogue's sums hides the other."""
    nh = 2 if nbh == 2 else 8
    l = n // 256
    g = torch.Generator(device="cpu").manual_seed(n * 3 + nbh)
    ql = (torch.randn(nbh, 256, 64, generator=g) * 0.3).to(torch.bfloat16)
    dw = (torch.randn(nbh, 256, 64, generator=g) * 0.1).to(torch.bfloat16)
    k = (torch.randn(nbh, n, 64, generator=g) * 0.3).to(torch.bfloat16)
    v = torch.randn(nbh, n, 64, generator=g).to(torch.bfloat16)
    base = R.a3_bwd_ref(ql, dw, k, v)
    lse, d, dk, dv, _ = base
    dkl = torch.randn(nbh, 256, 64, generator=g) * (l * dk.abs().max().item() / 4)
    dvc = (torch.randn(nbh, n, 64, generator=g) * (dv.abs().max().item() / 4)).to(torch.bfloat16)
    # D as the [2][nbh][256] partials over the two 32-column halves (tm_bmm_job.Rd of dW = Z^T dY)
    prod = dw.double() * R.a3_fwd_ref(ql, k, v)
    dparts = torch.stack([prod[..., :32].sum(-1), prod[..., 32:].sum(-1)])
    assert torch.allclose(dparts.sum(0), d)
    dev = _dev(ql, dw, k, v, lse.float(), dparts.float(), dkl)
    return SimpleNamespace(nh=nh, l=l, ql=ql, dw=dw, k=k, v=v, base=base, dkl=dkl, dvc=dvc, dev=dev)


A3_CASES = [
    (8, 256, 0, 256), (8, 256, 0, 17), (8, 256, 238, 256),           # l = 1
    (2, 768, 0, 768), (2, 768, 0, 17), (2, 768, 150, 183),           # l = 3, nbh < 8, one unit per workgroup
    (8, 1280, 0, 1280), (8, 1280, 0, 17), (8, 1280, 150, 183),       # l = 5, 40 units over 32 workgroups
    (8, 8448, 0, 8448), (8, 8448, 0, 17), (8, 8448, 150, 183),       # l = 33, the 9-wave form
    (16, 8448, 0, 8448),                                             # ceil(units / 8) workgroups
]


@pytest.mark.parametrize("nbh,n,lo,hi", A3_CASES)
def test_a3_bwd_fused_key_side_and_slabs(nbh, n, lo, hi):
    """tm_nys_a3_bwd_fused with dql = NULL and dql != NULL: dv_conv NaN outside [lo, hi), dqkv
    prefilled with 7, the workspace with NaN.
      - q columns keep the sentinel, every k / v element is finite (no read outside the window);
      - against tm_nys_a3_bwd(BF16) on the same operands (the same attn_bwd_bf16_kernel instance, so
        identical accumulators): v columns == bf16(unfused dv) bitwise, the bf16 slabs left in work
        == bf16(the unfused fp32 slabs) bitwise, and the k columns against
        want = bf16(unfused dk + p32), p32 = fp32(dk~[t // l] * fp32(1 / l)), all in fp32:
        "within one bf16 ulp" held at l = 1 (0 ulp) and l = 3 (1 ulp) but not at l >= 5 (2 ulps at 8
        heads, 10 at 16 x 8448 measured).  The differing operation: the epilogue's
        `*sk + ak * il` (nystrom_bf16.h, the fused branch of attn_bwd_bf16_kernel) is compiled with
        fp contraction on, so it is fma(dk~, 1/l, dK): the product is not rounded to fp32 first.
        That moves the fp32 sum by up to half an fp32 ulp OF THE PRODUCT, which is many ulps of the
        sum where dK and dk~ / l cancel.  Derived bound (not a loosening to a looser constant):
        |fused - want| <= ulp_bf16(m) + ulp_f32(m) + ulp_f32(p32) / 2, m = max(|fused|, |want|)
        (the two fp32 roundings of the sums, the product's rounding, then the bf16 roundings).  The
        count of elements equal to neither bf16(sum with p32) nor bf16(fma) is printed;
      - dql != NULL: dql == the fp32 sum of those bf16 slabs in the flush launch's order, bitwise.
        That order is the index order up to 24 slabs; with more (32 / 33 slabs here at n >= 1280,
        8 / 16 heads) gemm.hip push_reduce_entry gives each output two lanes, which add the even
        and the odd slabs in index order and then each other (R.slab_sum_f32 / R.reduce_par
        restate it) -- read from the code, so the claim stays bitwise;
      - against fp64 on the same bf16-rounded operands: k columns, v columns and the slab sum
        within 2e-2 of the reference's largest entry (test_a3_bwd_bf16_even_split's bound).
    Measured on the MI355X (max over the 13 cases x 2 dql forms): k columns up to 10 bf16 ulps from
    want but at most 0.99998 of the derived bound, and every element equal to bf16 of the separately
    rounded sum or of the fma (count of neither: 0, asserted); against fp64 3.7e-3 (k), 3.7e-3 (v),
    5.6e-3 (slab sum); every bitwise claim held."""
    L = _lib()
    _p, _stream = _eng()
    from transmil_deepgraft_amd._lib import BF16
    c = _a3_case(nbh, n)
    nh, l, B = c.nh, c.l, nbh // c.nh
    qd, wd, kd, vd, lsed, dd, dkld = c.dev
    dvc = c.dvc.clone()
    dvc[:, :lo] = NAN
    dvc[:, hi:] = NAN
    dvcd = dvc.to(DEV)
    ref_k, ref_v, ref_dql = R.a3_bwd_fused_ref(c.ql, c.dw, c.k, c.v, dvc, lo, hi, c.dkl, nh, base=c.base)
    ws = L.query("tm_nys_a3_bwd_workspace", nbh, n) // 4
    slabs = L.query("tm_nys_a3_bwd_slabs", nbh, n)
    cnt = nbh * 256 * 64
    assert slabs * cnt <= ws
    # the unfused launch: dk (=), dv (+=, preset to the window), fp32 slabs left in work
    dk_u = torch.full((nbh, n, 64), NAN, device=DEV)
    dv_u = torch.zeros(nbh, n, 64, device=DEV)
    dv_u[:, lo:hi] = dvcd[:, lo:hi].float()
    work_u = torch.full((ws,), NAN, device=DEV)
    dql_u = torch.full((nbh, 256, 64), NAN, device=DEV)
    L.call("tm_nys_a3_bwd", BF16, _p(qd), _p(wd), _p(kd), _p(vd), _p(lsed), _p(dd), nbh, nh, n, _p(dk_u), _p(dv_u),
           _p(work_u), _p(dql_u), 0, None, _stream())
    torch.cuda.synchronize()
    slab_u = work_u[:slabs * cnt].view(slabs, nbh, 256, 64).cpu()
    assert torch.isfinite(slab_u).all()
    want_slab = slab_u.to(torch.bfloat16)
    want_v = R.heads_to_cols(dv_u.cpu(), nh).to(torch.bfloat16)
    inv_l = torch.tensor(float(np.float32(1.0) / np.float32(l)))
    p32 = c.dkl.repeat_interleave(l, dim=1) * inv_l
    want_k = R.heads_to_cols(dk_u.cpu() + p32, nh).to(torch.bfloat16)
    fma_k = R.heads_to_cols((dk_u.cpu().double() + c.dkl.repeat_interleave(l, dim=1).double() * inv_l.double()).float(),
                            nh).to(torch.bfloat16)
    p32 = R.heads_to_cols(p32, nh)
    inner = nh * 64
    for use_dql in (False, True):
        dqkv = torch.full((B, n, 3 * inner), SENTINEL, dtype=torch.bfloat16, device=DEV)
        work = torch.full((ws,), NAN, device=DEV)
        dql = torch.full((nbh, 256, 64), NAN, device=DEV) if use_dql else None
        L.call("tm_nys_a3_bwd_fused", _p(qd), _p(wd), _p(kd), _p(vd), _p(lsed), _p(dd), nbh, nh, n, _p(dvcd), lo, hi,
               _p(dkld), _p(work), _p(dql), _p(dqkv), None, _stream())
        torch.cuda.synchronize()
        out = dqkv.cpu()
        got_q, got_k, got_v = out[..., :inner], out[..., inner:2 * inner], out[..., 2 * inner:]
        assert (got_q == SENTINEL).all()
        assert torch.isfinite(got_k.float()).all() and torch.isfinite(got_v.float()).all()
        # fused against unfused
        assert torch.equal(got_v, want_v)
        m = torch.maximum(got_k.float().abs(), want_k.float().abs())
        diff = (got_k.float() - want_k.float()).abs()
        bound = _ulp_bf16(m) + _ulp_f32(m) + 0.5 * _ulp_f32(p32)
        neither = ((got_k != want_k) & (got_k != fma_k)).sum().item()
        _report(f"a3 fused k vs unfused (max bf16 ulps, max diff / bound, neither sum nor fma) {nbh, n, lo, hi, use_dql}",
                ((diff / _ulp_bf16(m)).max().item(), (diff / bound).max().item(), neither))
        assert (diff <= bound).all()
        assert neither == 0
        got_slab = work.view(torch.bfloat16)[:slabs * cnt].view(slabs, nbh, 256, 64).cpu()
        assert torch.equal(got_slab, want_slab)
        if use_dql:
            assert torch.equal(dql.cpu(), R.slab_sum_f32(want_slab, R.reduce_par(slabs, cnt)))
        # against fp64
        ek, ev, eq = _rel(got_k, ref_k), _rel(got_v, ref_v), _rel(got_slab.double().sum(0), ref_dql)
        _report(f"a3 fused vs fp64 (k, v, slab sum) {nbh, n, lo, hi, use_dql}", (ek, ev, eq))
        assert ek < 2e-2 and ev < 2e-2 and eq < 2e-2


# ============================================================================= b. class-row A1 row
CLS_CASES = [(1, 256, 254), (2, 1024, 0), (2, 1024, 5), (1, 8448, 166), (3, 512, 300)]


@functools.lru_cache(maxsize=2)
def _cls_row_run(B, n, r, dtype):
    """Operands (scaled as test_a1_fwd_bf16_kernels), the forward and the backward launch with the
    forward's lse1, and the fp64 references on the same T-rounded operands."""
    L = _lib()
    _p, _stream = _eng()
    nh, code = 8, _tt(dtype)
    nbh = B * nh
    g = torch.Generator(device="cpu").manual_seed(n + 31 * r + B)
    q = (torch.randn(nbh, n, 64, generator=g) * 0.3).to(dtype)
    v = torch.randn(nbh, n, 64, generator=g).to(dtype)
    kl = (torch.randn(nbh, 256, 64, generator=g) * 0.3).to(dtype)
    y = torch.randn(nbh, 256, 64, generator=g).to(dtype)
    wconv = torch.randn(nh, 33, generator=g) * 0.1
    dm = (torch.randn(B, nh * 64, generator=g) * 0.1).to(dtype)
    ref_m, ref_lse = R.cls_a1_row_ref(q, v, kl, y, wconv, nh, r)
    ref_bwd = R.cls_a1_row_bwd_ref(dm, q, v, kl, y, wconv, nh, r)
    qd, vd, kld, yd, wd, dmd = _dev(q, v, kl, y, wconv, dm)
    merged = torch.full((B, n, nh * 64), SENTINEL, dtype=dtype, device=DEV)
    lse1 = torch.full((nbh, n), SENTINEL, device=DEV)
    L.call("tm_cls_a1_row_fwd", code, _p(qd), _p(vd), _p(kld), _p(yd), _p(wd), nbh, nh, n, r, _p(merged), _p(lse1),
           _stream())
    dq = torch.full((nbh, n, 64), NAN, device=DEV)
    dv = torch.full((nbh, n, 64), NAN, dtype=dtype, device=DEV)
    dkl = torch.full((nbh, 256, 64), NAN, device=DEV)
    dy = torch.full((nbh, 256, 64), NAN, device=DEV)
    dwconv = torch.full((nh, 33), NAN, device=DEV)
    L.call("tm_cls_a1_row_bwd", code, _p(dmd), _p(qd), _p(vd), _p(kld), _p(yd), _p(lse1), _p(wd), B, nh, n, r, _p(dq),
           _p(dkl), _p(dy), _p(dv), _p(dwconv), _stream())
    torch.cuda.synchronize()
    return SimpleNamespace(nh=nh, nbh=nbh, v=v, vd=vd, ref_m=ref_m, ref_lse=ref_lse, ref_bwd=ref_bwd, merged=merged,
                           lse1=lse1, dq=dq, dv=dv, dkl=dkl, dy=dy, dwconv=dwconv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,n,r", CLS_CASES)
def test_cls_a1_row_fwd_bwd(B, n, r, dtype):
    """tm_cls_a1_row_fwd / tm_cls_a1_row_bwd against fp64 on the same T-rounded operands.
    Forward (merged, lse1 prefilled with 7): only merged[b][r] and lse1[bh][r] change; lse within
    1e-4 absolute; the merged row within 1e-5 (fp32) / 4e-3 (bf16: fp32 sums, one bf16 rounding, the
    bound of test_conv_bwd_bf16_mfma) of the fp64 row's largest entry.
    Backward (lse1 of the forward; dq, dv prefilled with NaN): exactly row r of dq and rows
    [max(r-16, 0), min(r+17, n)) of dv are finite afterwards, and all of those are (the engine hands
    both buffers over uninitialised in the bf16 mode); dq row, dk~, dY, dwconv (fp32 sums, fp32 out)
    within 1e-5, the dv window within 1e-5 / 4e-3.
    Measured on the MI355X (max over the cases): lse 7.2e-7; merged row 1.0e-7 (fp32) / 3.3e-3
    (bf16); dq 6.6e-7, dk~ 9.1e-7, dY 6.6e-7, dwconv 1.0e-7; dv window 4.5e-8 (fp32) / 3.5e-3 (bf16)."""
    c = _cls_row_run(B, n, r, dtype)
    nh, nbh = c.nh, c.nbh
    tol_t = 1e-5 if dtype == torch.float32 else 4e-3
    merged, lse1 = c.merged.cpu().float(), c.lse1.cpu()
    row, lrow = merged[:, r].clone(), lse1[:, r].clone()
    merged[:, r] = SENTINEL
    lse1[:, r] = SENTINEL
    assert (merged == SENTINEL).all() and (lse1 == SENTINEL).all()
    e_lse, e_m = (lrow.double() - c.ref_lse).abs().max().item(), _rel(row, c.ref_m)
    _report(f"cls fwd (lse abs, merged rel) {B, n, r, dtype}", (e_lse, e_m))
    assert e_lse < 1e-4
    assert e_m < tol_t
    # backward: the written rows
    lo, hi = max(r - 16, 0), min(r + 17, n)
    fq = torch.isfinite(c.dq.cpu()).all(-1)                 # [nbh, n]
    fv = torch.isfinite(c.dv.cpu().float())
    want_q = torch.zeros(nbh, n, dtype=torch.bool)
    want_q[:, r] = True
    want_v = torch.zeros(nbh, n, 64, dtype=torch.bool)
    want_v[:, lo:hi] = True
    assert torch.equal(fq, want_q) and torch.isfinite(c.dq[:, r]).all()
    assert torch.equal(fv, want_v)
    rq, rkl, ry, rvw, rw = c.ref_bwd
    errs = (_rel(c.dq[:, r], rq), _rel(c.dkl, rkl), _rel(c.dy, ry), _rel(c.dwconv, rw), _rel(c.dv[:, lo:hi], rvw))
    _report(f"cls bwd (dq, dkl, dy, dwconv, dv) {B, n, r, dtype}", errs)
    assert all(e < 1e-5 for e in errs[:4]), errs
    assert errs[4] < tol_t, errs


# ============================================================================= c. class-row chain
@pytest.mark.parametrize("B,n,r", [(1, 256, 254), (2, 1024, 5)])
def test_cls_row_chain_into_fused_a3_and_assemble_q(B, n, r):
    """The bf16 class-row path of engine.nystrom_core_backward (_core_backward_bf16): the dv window and dq row of
    tm_cls_a1_row_bwd (NaN everywhere else, as the pool's uninitialised buffers may be) feed
    tm_nys_a3_bwd_fused(dv_lo, dv_hi, dql = NULL) and tm_nys_assemble_q_slab(dq_row = r).  The
    whole dqkv (prefilled with NaN) is finite and each third within 2e-2 of the fp64 chain
    (cls_a1_row_bwd_ref -> a3_bwd_fused_ref -> assemble_q_ref) relative to that third's largest entry.
    Measured on the MI355X (max over the two cases): q 4.3e-3, k 3.1e-3, v 4.6e-3."""
    L = _lib()
    _p, _stream = _eng()
    from transmil_deepgraft_amd._lib import BF16
    c = _cls_row_run(B, n, r, torch.bfloat16)
    nh, nbh, scale = c.nh, c.nbh, 0.125
    lo, hi = max(r - 16, 0), min(r + 17, n)
    g = torch.Generator(device="cpu").manual_seed(5 * n + r)
    ql = (torch.randn(nbh, 256, 64, generator=g) * 0.3).to(torch.bfloat16)
    dw = (torch.randn(nbh, 256, 64, generator=g) * 0.1).to(torch.bfloat16)
    k = (torch.randn(nbh, n, 64, generator=g) * 0.3).to(torch.bfloat16)
    dql = torch.randn(nbh, 256, 64, generator=g) * 0.01
    base = R.a3_bwd_ref(ql, dw, k, c.v)
    prod = dw.double() * R.a3_fwd_ref(ql, k, c.v)
    dparts = torch.stack([prod[..., :32].sum(-1), prod[..., 32:].sum(-1)]).float()
    qd, wd, kd, lsed, dd, dqld = _dev(ql, dw, k, base[0].float(), dparts, dql)
    inner = nh * 64
    dqkv = torch.full((B, n, 3 * inner), NAN, dtype=torch.bfloat16, device=DEV)
    work = torch.full((L.query("tm_nys_a3_bwd_workspace", nbh, n) // 4,), NAN, device=DEV)
    L.call("tm_nys_a3_bwd_fused", _p(qd), _p(wd), _p(kd), _p(c.vd), _p(lsed), _p(dd), nbh, nh, n, _p(c.dv), lo, hi,
           _p(c.dkl), _p(work), None, _p(dqkv), None, _stream())
    slabs = L.query("tm_nys_a3_bwd_slabs", nbh, n)
    L.call("tm_nys_assemble_q_slab", BF16, _p(c.dq), r, _p(dqld), _p(work), slabs, B, nh, n, C.c_float(scale),
           _p(dqkv), _stream())
    torch.cuda.synchronize()
    out = dqkv.cpu().float()
    assert torch.isfinite(out).all()
    rq, rkl, _, rvw, _ = c.ref_bwd
    dvc = torch.full((nbh, n, 64), NAN, dtype=torch.float64)
    dvc[:, lo:hi] = rvw
    ref_k, ref_v, ref_dql3 = R.a3_bwd_fused_ref(ql, dw, k, c.v, dvc, lo, hi, rkl, nh, base=base)
    dq = torch.full((nbh, n, 64), NAN, dtype=torch.float64)
    dq[:, r] = rq
    ref_q = R.assemble_q_ref(dq, r, dql.double() + ref_dql3, nh, scale)
    errs = (_rel(out[..., :inner], ref_q), _rel(out[..., inner:2 * inner], ref_k), _rel(out[..., 2 * inner:], ref_v))
    _report(f"cls chain dqkv (q, k, v) {B, n, r}", errs)
    assert all(e < 2e-2 for e in errs), errs


# ============================================================================= d. dropout mask, class-row to_out
DROP_SHAPES = [(77, 256, 179), (1025, 1280, 255)]
SEED, COUNTER = 0x5DEECE66D1234567, 3


def _seed_args(use_ptr):
    """(seed_ptr tensor or None, the counter value dropout_keep takes)."""
    if use_ptr:
        return torch.tensor([COUNTER], dtype=torch.int64, device=DEV), COUNTER
    return None, 0


@pytest.mark.parametrize("use_ptr", [False, True])
@pytest.mark.parametrize("S,n,pad", DROP_SHAPES)
def test_dropout_mask_is_one_function_of_seed_row_column(S, n, pad, use_ptr):
    """p = 0.7, B = 2, D = 512, a non-zero seed, seed_ptr NULL or a device counter: the mask is
    dropout_keep(seed, row b*S + i, column) in
      - tm_dropout_bwd_pad (fp32, bf16): out[b][pad+i][c] == T(dH[b*S+i][c] * fp32(1/0.3)) where kept,
        0 elsewhere, pad rows exactly 0 (bitwise);
      - the GEMM epilogue with the front-pad row map (n, pad, S, 0, 0, 0), M = B*n, N = K = 512,
        fp32 and bf16 operands: the non-zero pattern of out - resid is that mask exactly (positive
        operands: every kept product is >= 1; integer residuals: the subtraction is exact to well
        below that), the kept values within 1e-5 / 8e-3 of fp64 (the bounds of the neighbouring GEMM
        tests);
    and tm_pad_rows is the exact T-rounded copy with zero pad rows.
    Measured on the MI355X: every mask and copy bitwise; kept GEMM values 1.5e-6 (fp32) / 5.6e-7 (bf16
    operands: exact products, fp32 sums and output)."""
    L = _lib()
    _p, _stream = _eng()
    from transmil_deepgraft_amd.engine import gemm
    from transmil_deepgraft_amd._lib import F32
    B, D, p = 2, 512, 0.7
    sp, ctr = _seed_args(use_ptr)
    keep = torch.from_numpy(R.dropout_keep(ctr, SEED, B * S, D, p))
    assert abs(keep.double().mean().item() - 0.3) < 0.01
    g = torch.Generator(device="cpu").manual_seed(S)
    dH = torch.randn(B * S, D, generator=g)
    scale = torch.tensor(float(R.drop_scale_f32(p)))
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((B, n, D), NAN, dtype=dtype, device=DEV)
        L.call("tm_dropout_bwd_pad", _tt(dtype), _p(dH.to(DEV)), B, S, n, pad, D, C.c_float(p), C.c_uint64(SEED), _p(sp),
               _p(out), _stream())
        y = torch.full((B, n, D), NAN, dtype=dtype, device=DEV)
        L.call("tm_pad_rows", _tt(dtype), _p(dH.to(DEV)), B, S, n, pad, D, _p(y), _stream())
        torch.cuda.synchronize()
        want = torch.zeros(B, n, D)
        want[:, pad:] = torch.where(keep, dH * scale, torch.zeros(())).view(B, S, D)
        assert torch.equal(out.cpu(), want.to(dtype))
        want_y = torch.zeros(B, n, D)
        want_y[:, pad:] = dH.view(B, S, D)
        assert torch.equal(y.cpu(), want_y.to(dtype))
        # GEMM epilogue, rows mapped m = b*n + t -> b*S + t - pad (t < pad not stored)
        A = (torch.rand(B * n, D, generator=g) * 0.5 + 0.25).to(dtype)
        W = (torch.rand(D, D, generator=g) * 0.05 + 0.025).to(dtype)
        Rs = torch.randint(-4, 5, (B * S, D), generator=g).float()
        res = torch.full((B * S, D), NAN, device=DEV)
        gemm(A.to(DEV), W.to(DEV), res, B * n, D, D, lda=D, ldb=D, ldc=D, dtype=_tt(dtype), c_dtype=F32, drop_p=p,
             seed=SEED, seed_ptr=sp, resid=Rs.to(DEV), rowmap=(n, pad, S, 0, 0, 0))
        torch.cuda.synchronize()
        o = res.cpu() - Rs
        assert torch.isfinite(o).all()
        assert torch.equal(o != 0, keep)
        full = (A.double() @ W.double().t()).view(B, n, D)[:, pad:].reshape(B * S, D) / 0.3
        assert full.min() > 1.0
        e = _rel(o[keep], full[keep])
        _report(f"gemm dropout kept values {S, use_ptr, dtype}", e)
        assert e < (1e-5 if dtype == torch.float32 else 8e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dropout_bwd_pad_and_pad_rows_leave_the_tail_rows_alone(dtype):
    """(B, S, n_pad, pad, D) = (2, 7, 16, 5, 64), p = 0.7: four rows per bag past pad + S, which have
    no input row.  The input holds exactly B * S rows and the outputs one extra row, prefilled with 7.
    Data and pad rows as in test_dropout_mask_is_one_function_of_seed_row_column (bitwise); the tail
    rows and the extra row keep the sentinel.  Both kernels used to launch n_pad rows per bag and
    filled the tail from the next bag's rows (past the input, for the last bag)."""
    L = _lib()
    _p, _stream = _eng()
    B, S, n, pad, D, p = 2, 7, 16, 5, 64, 0.7
    sp, ctr = _seed_args(True)
    keep = torch.from_numpy(R.dropout_keep(ctr, SEED, B * S, D, p))
    dH = torch.randn(B * S, D, generator=torch.Generator(device="cpu").manual_seed(S))
    dHd = dH.to(DEV)
    scale = torch.tensor(float(R.drop_scale_f32(p)))
    out = torch.full((B * n + 1, D), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_dropout_bwd_pad", _tt(dtype), _p(dHd), B, S, n, pad, D, C.c_float(p), C.c_uint64(SEED), _p(sp), _p(out),
           _stream())
    y = torch.full((B * n + 1, D), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_pad_rows", _tt(dtype), _p(dHd), B, S, n, pad, D, _p(y), _stream())
    torch.cuda.synchronize()
    want = torch.full((B * n + 1, D), SENTINEL)
    want_y = want.clone()
    want[:-1].view(B, n, D)[:, :pad] = 0.0
    want[:-1].view(B, n, D)[:, pad:pad + S] = torch.where(keep, dH * scale, torch.zeros(())).view(B, S, D)
    want_y[:-1].view(B, n, D)[:, :pad] = 0.0
    want_y[:-1].view(B, n, D)[:, pad:pad + S] = dH.view(B, S, D)
    assert torch.equal(out.cpu(), want.to(dtype))
    assert torch.equal(y.cpu(), want_y.to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.0, 0.7])
@pytest.mark.parametrize("use_ptr", [False, True])
@pytest.mark.parametrize("S,n,pad", DROP_SHAPES)
def test_cls_out_fwd_bwd_against_fp64_with_the_same_mask(S, n, pad, use_ptr, p, dtype):
    """tm_cls_out_fwd: H3[b*S] = H2[b*S] + keep / 0.3 * (merged[b][r] Wo^T + bo) within 1e-5 of fp64
    (T-rounded merged / Wo, fp32 sums, fp32 out), every other row of H3 keeps its sentinel.
    tm_cls_out_bwd (dH NaN outside the class rows: nothing else is read; outputs prefilled with
    NaN): dout[b] = T(keep * fp32(1/0.3) * dH[b*S]) as the kernel and tm_dropout_bwd_pad round it, then
    dWo = sum_b dout[b] (x) merged[b][r], dbo = sum_b dout[b] within 1e-5, dmerged = T(dout Wo) within
    1e-5 (fp32) / 4e-3 (bf16).  keep = dropout_keep(seed, b*S, c), the mask of the dense epilogue.
    Measured on the MI355X (max over the cases): H3 rows 1.5e-7, dWo 7.1e-8, dbo 4.3e-8, dmerged
    7e-8 (fp32) / 2.3e-3 (bf16)."""
    L = _lib()
    _p, _stream = _eng()
    B, D, r, code = 2, 512, pad, _tt(dtype)
    sp, ctr = _seed_args(use_ptr)
    keep = torch.from_numpy(R.dropout_keep(ctr, SEED, B * S, D, 0.7)).view(B, S, D)[:, 0] if p > 0 else \
        torch.ones(B, D, dtype=torch.bool)
    g = torch.Generator(device="cpu").manual_seed(S + 1)
    merged = torch.randn(B, n, D, generator=g).to(dtype)
    wo = (torch.randn(D, D, generator=g) * 0.05).to(dtype)
    bo = torch.randn(D, generator=g) * 0.1
    H2 = torch.randn(B * S, D, generator=g)
    dH = torch.full((B, S, D), NAN)
    dH[:, 0] = torch.randn(B, D, generator=g)
    md, wod, bod, H2d, dHd = _dev(merged, wo, bo, H2, dH.view(B * S, D))
    H3 = torch.full((B * S, D), SENTINEL, device=DEV)
    L.call("tm_cls_out_fwd", code, _p(md), _p(wod), _p(bod), _p(H2d), B, n, r, S, D, C.c_float(p), C.c_uint64(SEED),
           _p(sp), _p(H3), _stream())
    dwo = torch.full((D, D), NAN, device=DEV)
    dbo = torch.full((D,), NAN, device=DEV)
    dmerged = torch.full((B, D), NAN, dtype=dtype, device=DEV)
    L.call("tm_cls_out_bwd", code, _p(dHd), _p(md), _p(wod), B, n, r, S, D, C.c_float(p), C.c_uint64(SEED), _p(sp),
           _p(dwo), _p(dbo), _p(dmerged), _stream())
    torch.cuda.synchronize()
    inv = 1.0 / 0.3 if p > 0 else 1.0
    mr = merged[:, r].double()
    want = H2.view(B, S, D)[:, 0].double() + keep.double() * inv * (mr @ wo.double().t() + bo.double())
    got = H3.cpu().view(B, S, D)
    assert (got[:, 1:] == SENTINEL).all()
    e_f = _rel(got[:, 0], want)
    scale = torch.tensor(float(R.drop_scale_f32(p)))
    dout = torch.where(keep, dH[:, 0] * scale, torch.zeros(())).to(dtype).double()          # [B, D]
    errs = (_rel(dwo, dout.t() @ mr), _rel(dbo, dout.sum(0)), _rel(dmerged, dout @ wo.double()))
    _report(f"cls_out fwd, bwd (dwo, dbo, dmerged) {S, use_ptr, p, dtype}", (e_f,) + errs)
    assert e_f < 1e-5
    assert errs[0] < 1e-5 and errs[1] < 1e-5, errs
    assert errs[2] < (1e-5 if dtype == torch.float32 else 4e-3), errs


# ============================================================================= e. LayerNorm backward
LN_CASES = [(2, 77, 256, 179), (1, 1025, 1280, 255)]
RPB = 16      # engine._LN_BWD_RPB


def _ln_operands(B, S, n, pad, dtype, with_seg):
    D = 512
    g = torch.Generator(device="cpu").manual_seed(S + n)
    x = torch.randn(B * S, D, generator=g) * 1.5 + 0.3
    gamma = torch.rand(D, generator=g) + 0.5
    mean = x.double().mean(-1).float()
    rstd = (1.0 / torch.sqrt(x.double().var(-1, unbiased=False) + 1e-5)).float()
    dy = torch.randn(B, n, D, generator=g).to(dtype)
    dy[:, :pad] = NAN                                   # pad rows of dy are never read
    acc = torch.randn(B * S, D, generator=g)
    seg = None
    if with_seg:                                         # every row distinct: a wrong segment index cannot cancel
        seg = torch.randn(B, 288, D, generator=g) + torch.arange(288).view(1, 288, 1) * 0.01
    return D, x, gamma, mean, rstd, dy, acc, seg


def _ln_run(entry, B, S, n, pad, dtype, resid, ops, queued):
    L = _lib()
    _p, _stream = _eng()
    D, x, gamma, mean, rstd, dy, acc, seg = ops
    acc_in = acc.clone()
    if resid:
        acc_in.view(B, S, D)[:, 1:] = NAN               # written without being read
    xd, gd, md, rd, dyd, dx = _dev(x, gamma, mean, rstd, dy, acc_in)
    work = torch.full((L.query("tm_layernorm_bwd_workspace", B * S, D, RPB) // 4,), NAN, device=DEV)
    dg = torch.full((D,), NAN, device=DEV)
    db = torch.full((D,), NAN, device=DEV)

    def launch(rq):
        if entry == "tm_layernorm_bwd":
            L.call(entry, _p(dyd), _tt(dtype), _p(xd), _p(gd), _p(md), _p(rd), B * S, D, S, n, pad, RPB, resid, _p(dx),
                   _p(work), _p(dg), _p(db), rq, _stream())
        else:
            segd = seg.to(DEV)
            L.call(entry, _p(dyd), _tt(dtype), _p(xd), _p(gd), _p(md), _p(rd), B * S, D, S, n, pad, RPB, resid,
                   _p(segd), n // 256, 256, 288, _p(dx), _p(work), _p(dg), _p(db), rq, _stream())
    if queued:
        with _Queue() as q:
            launch(q.h)
            assert q.pending() == 2
            q.flush()
            torch.cuda.synchronize()
    else:
        launch(None)
        torch.cuda.synchronize()
    return dx.cpu(), dg.cpu(), db.cpu(), acc_in


def _ln_check(entry, B, S, n, pad, dtype, resid, with_seg):
    ops = _ln_operands(B, S, n, pad, dtype, with_seg)
    D, x, gamma, mean, rstd, dy, acc, seg = ops
    now = _ln_run(entry, B, S, n, pad, dtype, resid, ops, queued=False)
    later = _ln_run(entry, B, S, n, pad, dtype, resid, ops, queued=True)
    for a, b in zip(now[:3], later[:3]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    ref = R.ln_bwd_seg_ref(dy, x, gamma, mean, rstd, S, pad, now[3], resid, seg=seg, seg_len=n // 256, nseg=256)
    errs = tuple(_rel(a, b) for a, b in zip(now[:3], ref))
    _report(f"{entry} (dx, dgamma, dbeta) {B, S, dtype, resid}", errs)
    assert all(e < 1e-4 for e in errs), errs


@pytest.mark.parametrize("resid_cls_only", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,S,n,pad", LN_CASES)
def test_layernorm_bwd_step_form(B, S, n, pad, dtype, resid_cls_only):
    """tm_layernorm_bwd as the step calls it: D = 512, 16 rows per block (bags straddle a block at
    S = 77), dy in bf16 / fp32 read from the front-padded layout (its pad rows NaN: never read),
    resid_cls_only 0 / 1 (1: the non-class rows of dx_accum hold NaN on entry and come out finite:
    written without being read).  The immediate reduce and a caller-owned queue flushed afterwards
    give the same bits; dx, dgamma, dbeta within 1e-4 of fp64 (test_layernorm_fwd_bwd's bound).
    The same-bits check failed at S = 1025 (65 blocks) before tm_splitk_reduce was fixed: with more
    than 24 partials the flush launch sums each output on several lanes, the immediate fp32 launch
    summed them on one, in another order; the immediate call now takes the flush's form there.
    Measured on the MI355X (max over the cases): dx 9.3e-8, dgamma 1.5e-7, dbeta 1.3e-7."""
    _ln_check("tm_layernorm_bwd", B, S, n, pad, dtype, resid_cls_only, False)


@pytest.mark.parametrize("resid_cls_only", [0, 1])
@pytest.mark.parametrize("B,S,n,pad", LN_CASES)
def test_layernorm_bwd_seg_step_form(B, S, n, pad, resid_cls_only):
    """tm_layernorm_bwd_seg (bf16 dy) with seg_add [B][288][512], nseg = 256, seg_len = n / 256 = 1 / 5,
    every seg_add row distinct: dy_eff[b][t] = dy[b][pad+t] + seg[b][(pad+t) // seg_len] + (t == 0)
    seg[b][256]; the same checks as test_layernorm_bwd_step_form.
    Measured on the MI355X (max over the cases): dx 1.2e-7, dgamma 1.6e-7, dbeta 1.3e-7."""
    _ln_check("tm_layernorm_bwd_seg", B, S, n, pad, torch.bfloat16, resid_cls_only, True)


# ============================================================================= f. tm_splitk_reduce_bf16
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("count", [4096, 4099])
@pytest.mark.parametrize("splits", [1, 5, 16])
def test_splitk_reduce_bf16_is_the_index_order_fp32_sum(splits, count, accumulate, alpha):
    """out (= / +=) alpha * sum_z slab[z] over bf16 slabs: the fp32 index-order sum computed in
    PyTorch, bitwise for alpha = 1, within one fp32 ulp for alpha = 0.5 (alpha * s + out may be one
    fma); count = 4099 takes the element-by-element form, 4096 the 16-B one; the immediate launch and
    a caller-owned queue flushed afterwards give the same bits.
    Measured on the MI355X: bitwise in every case, alpha = 0.5 included (0 ulp)."""
    L = _lib()
    _p, _stream = _eng()
    g = torch.Generator(device="cpu").manual_seed(splits * 7 + count)
    slab = torch.randn(splits, count, generator=g).to(torch.bfloat16)
    base = torch.randn(count, generator=g)
    s = R.slab_sum_f32(slab) * alpha
    want = s + base if accumulate else s
    slabd = slab.to(DEV)
    outs = []
    for queued in (False, True):
        out = base.clone().to(DEV) if accumulate else torch.full((count,), NAN, device=DEV)
        if queued:
            with _Queue() as q:
                L.call("tm_splitk_reduce_bf16", _p(slabd), _p(out), splits, count, C.c_float(alpha), accumulate, q.h,
                       _stream())
                assert q.pending() == 1
                q.flush()
                torch.cuda.synchronize()
        else:
            L.call("tm_splitk_reduce_bf16", _p(slabd), _p(out), splits, count, C.c_float(alpha), accumulate, None,
                   _stream())
            torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    if alpha == 1.0:
        assert torch.equal(outs[0], want)
    else:
        ulps = ((outs[0] - want).abs() / torch.maximum(_ulp_f32(want), _ulp_f32(outs[0]))).max().item()
        _report(f"splitk_reduce_bf16 alpha 0.5 [fp32 ulp] {splits, count, accumulate}", ulps)
        assert ulps <= 1.0


# ============================================================================= g. tm_splitk_reduce (fp32 slabs)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("count", [4096, 4099])
@pytest.mark.parametrize("splits", [1, 5, 16, 33])
def test_splitk_reduce_f32_is_the_index_order_fp32_sum(splits, count, accumulate, alpha):
    """out (= / +=) alpha * sum_z slab[z] over fp32 slabs, bit for bit the fp32 sum in the order
    kernel_refs.slab_sum_f32 restates (index order; 33 splits exceed one unrolled group of loads and
    give every output two lanes, reduce_par); count = 4099 takes the element-by-element form, 4096 the
    16-B one of the flush launch.  alpha = 0.5 scales exactly, so alpha * s + out rounds once whether
    or not it is one fma: bitwise there too.  The immediate launch and a caller-owned queue flushed
    afterwards give the same bits."""
    L = _lib()
    _p, _stream = _eng()
    g = torch.Generator(device="cpu").manual_seed(splits * 11 + count)
    slab = torch.randn(splits, count, generator=g)
    base = torch.randn(count, generator=g)
    s = R.slab_sum_f32(slab, R.reduce_par(splits, count, bf16=False)) * alpha
    want = s + base if accumulate else s
    slabd = slab.to(DEV)
    for queued in (False, True):
        out = base.clone().to(DEV) if accumulate else torch.full((count,), NAN, device=DEV)
        if queued:
            with _Queue() as q:
                L.call("tm_splitk_reduce", _p(slabd), _p(out), splits, count, C.c_float(alpha), accumulate, q.h,
                       _stream())
                assert q.pending() == 1
                q.flush()
                torch.cuda.synchronize()
        else:
            L.call("tm_splitk_reduce", _p(slabd), _p(out), splits, count, C.c_float(alpha), accumulate, None,
                   _stream())
            torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), ("queued" if queued else "immediate")
