"""tm_gemm (csrc/gemm.hip) against fp64 on every dispatch path, operand layout and epilogue: one
parametrised test over the table of tests/gemm_cases.py (the smallest shapes that reach each path;
test_gemm_cases_cpu.py proves the table's coverage and the reference without a GPU).

Every case
  * fails, not skips, if the product dispatch would not take the path the case names on this device
    (the 160-row cases build their row count from the CU count);
  * gives every output buffer a guard (leading-dimension padding, two extra rows, the rows a row map
    does not write), pre-filled with NaN -- or, under `accumulate`, with finite values that double as
    the addend -- and requires every contract element finite and every other element unchanged bit for
    bit; the operands' own padding is NaN, so a read past a row shows as well;
  * compares per element: |got - ref| <= 1e-5 max|ref| + r |ref|, r = 0 for fp32 stores and 2^-8 for a
    value stored once as bf16 (output, pre_bf16, bf16 slabs).  Dropout cases compare against the
    reference masked by the host restatement of the hash.
The measured max(err / bound) of every case is printed (DESIGN.md lists the worst per kernel).
"""
import ctypes as C
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gemm_cases as G  # noqa: E402
from gemm_cases import CASES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_PTRS = ("bias", "pre", "resid", "colsum", "seed_ptr")


def _mods():
    from transmil_deepgraft_amd import _lib, engine
    return _lib, engine


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _gemm_args(L, a, ptrs):
    g = L.GemmArgs()
    for k, v in a.items():
        if k not in _PTRS:
            setattr(g, k, v)
    for k in _PTRS:
        t = ptrs.get(k)
        setattr(g, k, t.data_ptr() if t is not None else None)
    return g


def _check(name, got, fill, ref, mask, r):
    """contract elements finite and inside the bound, everything else still the fill; returns max(err / bound)"""
    got = got.cpu()
    assert torch.isfinite(got[mask].float()).all(), f"{name}: a contract element is not finite (unwritten?)"
    assert torch.equal(_bits(got)[~mask], _bits(fill)[~mask]), f"{name}: an element outside the contract was written"
    err = (got.double() - ref).abs()[mask]
    bnd = G.bound(ref, mask, r)[mask]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    return ratio, bool((err <= bnd).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_tm_gemm_against_fp64(case):
    L, engine = _mods()
    cu = engine.cu_count()
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    b = G.build(case, gen, cu)
    a = b.args
    assert G.expected_path(a, cu) == (case.path, case.kind), "the dispatch would not take the path this case names"
    if case.m_cu:
        t128, t160 = G.tile_counts(a)
        assert t128 > cu and t160 <= cu, (a["M"], t128, t160, cu)
    refs = G.reference(case, b)

    A, B = b.A.to(DEV), b.B.to(DEV)
    bufs = {"C": b.C.to(DEV)}
    ptrs = {}
    for k in ("pre", "colsum"):
        if getattr(b, k) is not None:
            bufs[k] = ptrs[k] = getattr(b, k).to(DEV)
    for k, t in (("bias", b.bias), ("resid", b.resid), ("seed_ptr", b.seed_dev)):
        if t is not None:
            ptrs[k] = t.to(DEV)
    g = _gemm_args(L, a, ptrs)
    L.call("tm_gemm", C.c_void_p(A.data_ptr() + case.a_off * A.element_size()), C.c_void_p(B.data_ptr()),
           C.c_void_p(bufs["C"].data_ptr()), C.byref(g), engine._stream())
    torch.cuda.synchronize()

    fills = {"C": b.C, "pre": b.pre, "colsum": b.colsum}
    ok, worst = True, {}
    for k, (ref, mask, r) in refs.items():
        worst[k], inside = _check(f"{case.name}/{k}", bufs[k], fills[k], ref, mask, r)
        ok = ok and inside
    print(f"[measured] {case.name}: max(err / bound) " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert ok, worst


# ----------------------------------------------------------------------------- host side, no launch
def _plain_call(L, M, N, K, **over):
    """A bf16 ring-shaped call with a NaN-filled C; returns (rc, C tensor)"""
    _, engine = _mods()
    A = torch.zeros(max(M, 8) * max(K, 8) + 64, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(max(N, 8) * max(K, 8) + 64, dtype=torch.bfloat16, device=DEV)
    Cb = torch.full((max(M, 8) * max(N, 8),), float("nan"), dtype=torch.float32, device=DEV)
    a = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ab_dtype=G.BF16, c_dtype=G.F32, splits=1, k_per_split=max(K, 64),
             mode=G.EPI_PLAIN, alpha=1.0, drop_scale=1.0)
    ptr = {"A": A.data_ptr(), "B": B.data_ptr(), "C": Cb.data_ptr()}
    keep = []
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v(ptr[k])
        elif k == "colsum":
            keep.append(torch.zeros(M + 8, device=DEV))
            a[k] = keep[-1]
        else:
            a[k] = v
    g = _gemm_args(L, {k: v for k, v in a.items() if k not in _PTRS}, {k: a.get(k) for k in _PTRS})
    rc = L.lib().tm_gemm(C.c_void_p(ptr["A"]), C.c_void_p(ptr["B"]), C.c_void_p(ptr["C"]), C.byref(g), engine._stream())
    torch.cuda.synchronize()
    return rc, Cb


@pytest.mark.parametrize("M,N", [(0, 136), (136, 0), (0, 0)])
def test_empty_product_returns_zero_and_leaves_c_untouched(M, N):
    L, _ = _mods()
    rc, Cb = _plain_call(L, M, N, 64)
    assert rc == 0 and torch.isnan(Cb).all()


REFUSALS = [   # (id, what differs from a valid 136 x 136 x 128 bf16 call, text of tm_last_error())
    ("null-A", dict(A=lambda p: None), "null argument"),
    ("null-C", dict(C=lambda p: None), "null argument"),
    ("misaligned-A", dict(A=lambda p: p + 2), "16-B aligned"),
    ("lda-not-16B", dict(lda=68), "leading dimensions"),
    ("qkv-dh-12", dict(mode=G.EPI_QKV, nbags=1, nh=2, dh=12, seq=136, qscale=1.0), "dh % 8"),
    ("bf16-split-kps-96", dict(mode=G.EPI_SPLITK, splits=2, k_per_split=96), "multiple of 64"),
    ("colsum-off-the-ring", dict(mode=G.EPI_SPLITK, a_trans=1, b_kn=1, lda=136, ldb=72, K=100, k_per_split=128,
                                 colsum=True), "colsum needs"),
]


@pytest.mark.parametrize("why,over,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_arguments_return_one_with_a_message_and_leave_c_untouched(why, over, text):
    L, _ = _mods()
    over = dict(over)
    K = over.pop("K", 128)
    N = 72 if "dh" in over or "colsum" in over else 136
    rc, Cb = _plain_call(L, 136, N, K, **over)
    assert rc == 1, why
    assert text in L.last_error(), (why, L.last_error())
    assert torch.isnan(Cb).all()
