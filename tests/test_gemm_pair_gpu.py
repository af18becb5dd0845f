"""The paired ring launch (tm_gemm_pair_begin / tm_gemm_pair_end, gemm.hip's gemm_ring_pair_kernel):
a bf16 split-K weight gradient and a bf16 data gradient held and released as ONE grid.  Every case
compares bitwise against the same two products launched by plain ``tm_gemm`` on the same operands:
the pair runs the same 128 x 128 tile routine over the same tiles, only the launch grouping changes.

Shapes are the smallest at which the pair's block decode can go wrong (groups of 8 blocks dealt to
the two jobs, XCD-contiguous renumbering inside a job, partial row / column tiles, several splits,
very unequal job sizes); outputs are pre-filled with NaN so an unwritten tile shows."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _mods():
    from transmil_deepgraft_amd import _lib, engine
    return _lib, engine


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _Job:
    """One tm_gemm call: operands, a NaN-filled output and its arguments."""

    def __init__(self, A, B, out, g, extra=None):
        self.A, self.B, self.out, self.g, self.extra = A, B, out, g, extra

    def fresh(self):
        """The same call with fresh NaN-filled outputs (operands shared)."""
        _lib, _ = _mods()
        out = torch.full_like(self.out, float("nan"))
        g = _lib.GemmArgs.from_buffer_copy(self.g)
        extra = None
        if self.extra is not None:
            extra = torch.full_like(self.extra, float("nan"))
            g.colsum = extra.data_ptr()
        return _Job(self.A, self.B, out, g, extra)

    def call(self, stream):
        _lib, _ = _mods()
        _lib.call("tm_gemm", _ptr(self.A), _ptr(self.B), _ptr(self.out), C.byref(self.g), stream)

    def outputs(self):
        return [self.out] + ([self.extra] if self.extra is not None else [])


def _rand(gen, *shape):
    return (torch.rand(*shape, device="cuda", generator=gen) - 0.5).to(torch.bfloat16)


def wgrad_job(gen, M, N, K, splits, kps, slab_bf16=False, colsum=False):
    """out[z][M, N] = sum over split z's k of dY[k, m] X[k, n]  (k-strided operands, split-K slabs)."""
    _lib, _ = _mods()
    dY, X = _rand(gen, K, M), _rand(gen, K, N)
    out = torch.full((splits, M, N), float("nan"), device="cuda",
                     dtype=torch.bfloat16 if slab_bf16 else torch.float32)
    g = _lib.GemmArgs()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = M, N, N
    g.a_trans, g.b_kn = 1, 1
    g.ab_dtype, g.c_dtype = _lib.BF16, _lib.F32
    g.splits, g.k_per_split = splits, kps
    g.mode = _lib.EPI_SPLITK
    g.alpha = 1.0
    g.drop_scale = 1.0
    g.slab_bf16 = int(slab_bf16)
    extra = None
    if colsum:
        extra = torch.full((splits, M), float("nan"), device="cuda")
        g.colsum = extra.data_ptr()
    return _Job(dY, X, out, g, extra)


def dgrad_job(gen, M, N, K):
    """out[M, N] (bf16) = dY[m, k] W[k, n]  (b_kn = 1, plain store)."""
    _lib, _ = _mods()
    dY, W = _rand(gen, M, K), _rand(gen, K, N)
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    g = _lib.GemmArgs()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = K, N, N
    g.a_trans, g.b_kn = 0, 1
    g.ab_dtype, g.c_dtype = _lib.BF16, _lib.BF16
    g.splits, g.k_per_split = 1, (K + 63) // 64 * 64
    g.mode = _lib.EPI_PLAIN
    g.alpha = 1.0
    g.drop_scale = 1.0
    return _Job(dY, W, out, g)


def run_plain(jobs):
    _, engine = _mods()
    for j in jobs:
        j.call(engine._stream())
    torch.cuda.synchronize()


def run_paired(jobs):
    _lib, engine = _mods()
    st = engine._stream()
    _lib.call("tm_gemm_pair_begin", st)
    for j in jobs:
        j.call(st)
    _lib.call("tm_gemm_pair_end", st)
    torch.cuda.synchronize()


def assert_same(paired, plain):
    for jp, jr in zip(paired, plain):
        for a, b in zip(jp.outputs(), jr.outputs()):
            assert not torch.isnan(b.float()).any(), "reference left a tile unwritten"
            assert not torch.isnan(a.float()).any(), "the pair left a tile unwritten"
            assert torch.equal(a, b)


def check_pair(jobs):
    plain = [j.fresh() for j in jobs]
    run_plain(plain)
    paired = [j.fresh() for j in jobs]
    run_paired(paired)
    assert_same(paired, plain)


@pytest.mark.parametrize("dN", [128, 136])
@pytest.mark.parametrize("slab_bf16, colsum", [(False, False), (True, True)])
def test_pair_equals_plain_launches(dN, slab_bf16, colsum):
    """2 tiles x 5 splits of weight gradient with 3 row tiles (the last partial) of data gradient;
    dN = 136 adds a partial column tile.  fp32 slabs, and bf16 slabs with the fused column sums."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    w = wgrad_job(gen, 256, 128, 320, 5, 64, slab_bf16=slab_bf16, colsum=colsum)
    d = dgrad_job(gen, 300, dN, 256)
    check_pair([w, d])


@pytest.mark.parametrize("order", ["w_first", "d_first"])
@pytest.mark.parametrize("big", ["w", "d"])
def test_unequal_jobs_in_both_call_orders(order, big):
    """1 tile against 15: no block goes to the wrong job and no tile stays unwritten."""
    gen = torch.Generator(device="cuda").manual_seed(12)
    if big == "w":
        w = wgrad_job(gen, 384, 128, 320, 5, 64)          # 3 tiles x 5 splits
        d = dgrad_job(gen, 100, 128, 64)                  # 1 partial tile
    else:
        w = wgrad_job(gen, 128, 128, 64, 1, 64)           # 1 tile, 1 split
        d = dgrad_job(gen, 15 * 128 - 28, 128, 64)        # 15 row tiles, the last partial
    check_pair([w, d] if order == "w_first" else [d, w])


def test_not_ring_eligible_second_call_falls_back():
    """K = 96 is no multiple of the ring's 64-deep k-tile: separate launches, same results."""
    gen = torch.Generator(device="cuda").manual_seed(13)
    check_pair([wgrad_job(gen, 256, 128, 320, 5, 64), dgrad_job(gen, 300, 128, 96)])


def test_two_data_gradients_fall_back():
    gen = torch.Generator(device="cuda").manual_seed(14)
    check_pair([dgrad_job(gen, 300, 128, 256), dgrad_job(gen, 130, 136, 64)])


def test_one_call_and_no_call():
    _lib, engine = _mods()
    gen = torch.Generator(device="cuda").manual_seed(15)
    check_pair([dgrad_job(gen, 300, 128, 256)])
    check_pair([wgrad_job(gen, 256, 128, 320, 5, 64)])
    st = engine._stream()
    _lib.call("tm_gemm_pair_begin", st)
    _lib.call("tm_gemm_pair_end", st)
    _lib.call("tm_gemm_pair_end", st)      # no open pair: nothing to do
    torch.cuda.synchronize()


def test_error_inside_a_pair_leaves_nothing_held():
    """A host-side argument check fails on the second held call: it returns non-zero with a
    message, the pair is closed with nothing held (the first call is dropped, its output stays
    NaN), and after the following `end` a plain tm_gemm launches at once as usual."""
    _lib, engine = _mods()
    gen = torch.Generator(device="cuda").manual_seed(16)
    st = engine._stream()
    w = wgrad_job(gen, 256, 128, 320, 5, 64)
    d = dgrad_job(gen, 300, 128, 256)
    bad = d.fresh()
    bad.g.lda = 3                                   # not a multiple of 16 bytes
    _lib.call("tm_gemm_pair_begin", st)
    w.call(st)
    with pytest.raises(RuntimeError, match="leading dimensions"):
        bad.call(st)
    assert "leading dimensions" in _lib.last_error()
    _lib.call("tm_gemm_pair_end", st)
    torch.cuda.synchronize()
    assert torch.isnan(w.out).all() and torch.isnan(bad.out.float()).all()
    # begin on a thread that already has an open pair is refused, and closes it
    _lib.call("tm_gemm_pair_begin", st)
    with pytest.raises(RuntimeError, match="already open"):
        _lib.call("tm_gemm_pair_begin", st)
    # nothing is held now: a plain call runs at once
    ref, got = d.fresh(), d.fresh()
    run_paired([ref])
    got.call(st)
    torch.cuda.synchronize()
    assert_same([got], [ref])


def test_pair_under_graph_capture():
    _lib, engine = _mods()
    gen = torch.Generator(device="cuda").manual_seed(17)
    w = wgrad_job(gen, 256, 128, 320, 5, 64, slab_bf16=True, colsum=True)
    d = dgrad_job(gen, 300, 136, 256)
    plain = [w.fresh(), d.fresh()]
    run_plain(plain)
    jobs = [w.fresh(), d.fresh()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_paired(jobs)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = engine._stream()
        _lib.call("tm_gemm_pair_begin", st)
        for j in jobs:
            j.call(st)
        _lib.call("tm_gemm_pair_end", st)
    for _ in range(2):
        for j in jobs:
            for o in j.outputs():
                o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_same(jobs, plain)


@pytest.mark.parametrize("sel", [True, ("out", "qkv", "kv")])
def test_model_step_gradients_equal_with_pairing_off(monkeypatch, sel):
    """One bf16 training step (dropout on) at N = 300: every parameter gradient with the engine's
    ``pair_gemms`` on (the shipped pairs; every pair the engine can bracket) equals the unpaired
    step's bit for bit."""
    from transmil_deepgraft_amd import engine
    from transmil_deepgraft_amd.models import TransMIL
    torch.manual_seed(0)
    model = TransMIL(2, 512, 512).cuda().train().set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(1, 300, 512, device="cuda", generator=g)
    lab = torch.tensor([1], device="cuda")
    c0 = model._dropout_counter.clone()
    assert engine.TransMILEngine.pair_gemms is True
    grads = []
    for on in (sel, False):
        monkeypatch.setattr(engine.TransMILEngine, "pair_gemms", on)
        model.zero_grad(set_to_none=True)
        model._dropout_counter.copy_(c0)
        _, loss, _, _ = model.forward_ce(x, lab)
        loss.backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
    bad = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    assert not bad, bad
    assert all(torch.isfinite(v).all() for v in grads[0].values())
