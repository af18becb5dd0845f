"""tests/tail_refs.py against fp64 autograd (F.layer_norm, F.linear, CrossEntropyLoss on one-hot
targets, F.gelu) and the oracle PPEG, and the status path of the LayerNorm / head / glue entry
points (no GPU: every pointer is null, nothing is launched)."""
import pytest
import torch
import torch.nn.functional as F

import tail_refs as T

BOUND = 1e-12
EPS = 1e-5


def _err(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.mark.parametrize("B,S,pad,n_pad,D", [(2, 7, 5, 16, 64), (1, 1, 0, 1, 384), (3, 5, 3, 8, 128)])
def test_ln_fwd_ref_is_layer_norm_in_the_padded_layout(B, S, pad, n_pad, D):
    g = _gen(D + S)
    x = (0.3 + 1.5 * torch.randn(B * S, D, generator=g, dtype=torch.float64))
    x[0] = 1e-3 * torch.randn(D, generator=g, dtype=torch.float64)      # variance of the order of eps
    gamma = torch.rand(D, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(D, generator=g, dtype=torch.float64) * 0.4 - 0.2
    y, mean, rstd = T.ln_fwd_ref(x, gamma, beta, EPS, S, n_pad, pad)
    assert y.shape == (B, n_pad, D) and mean.shape == (B * S,) and rstd.shape == (B * S,)
    want = F.layer_norm(x, (D,), gamma, beta, EPS).view(B, S, D)
    assert _err(y[:, pad:pad + S], want) < BOUND
    assert (y[:, :pad] == 0).all() and torch.isnan(y[:, pad + S:]).all()
    assert _err(mean, x.mean(-1)) < BOUND
    assert _err(rstd, torch.rsqrt(x.var(-1, unbiased=False) + EPS)) < BOUND


@pytest.mark.parametrize("B,C,S,D", [(1, 2, 3, 64), (1, 5, 3, 384), (5, 7, 3, 128)])
def test_head_refs_are_layer_norm_and_linear_with_their_autograd(B, C, S, D):
    g = _gen(B * 100 + C)
    h = torch.randn(B, S, D, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gamma = torch.rand(D, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(D, generator=g, dtype=torch.float64) * 0.4 - 0.2
    W = torch.randn(C, D, generator=g, dtype=torch.float64) / D ** 0.5
    bias = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    dl = torch.randn(B, C, generator=g, dtype=torch.float64)
    ins = [t.clone().requires_grad_() for t in (h, gamma, beta, W, bias)]
    logits = F.linear(F.layer_norm(ins[0][:, 0], (D,), ins[1], ins[2], EPS), ins[3], ins[4])
    gh, ggamma, gbeta, gW, gbias = torch.autograd.grad(logits, ins, dl)
    got, xhat, rstd = T.head_ref(h.view(B * S, D), S, gamma, beta, EPS, W, bias)
    assert _err(got, logits.detach()) < BOUND
    x0 = h[:, 0]
    assert _err(rstd, torch.rsqrt(x0.var(-1, unbiased=False) + EPS)) < BOUND
    assert _err(xhat, F.layer_norm(x0, (D,), None, None, EPS)) < BOUND
    dW, dbias, dgamma, dbeta, dh = T.head_bwd_ref(dl, xhat, rstd, gamma, beta, W)
    assert (gh[:, 1:] == 0).all()
    for a, b in ((dW, gW), (dbias, gbias), (dgamma, ggamma), (dbeta, gbeta), (dh, gh[:, 0])):
        assert _err(a, b) < BOUND


@pytest.mark.parametrize("B,C", [(1, 2), (2, 3), (5, 7), (300, 2)])
def test_ce_refs_are_cross_entropy_on_one_hot_targets(B, C):
    g = _gen(B + 7 * C)
    logits = torch.randn(B, C, generator=g, dtype=torch.float64) * 3
    label = torch.randint(0, C, (B,), generator=g)
    dl_in = torch.randn(B, C, generator=g, dtype=torch.float64)
    lg = logits.clone().requires_grad_()
    ref = torch.nn.CrossEntropyLoss()(lg, F.one_hot(label, C).double())
    loss, prob, yhat, stats = T.ce_ref(logits, label)
    assert abs(loss.item() - ref.item()) < BOUND * max(1.0, abs(ref.item()))
    assert _err(prob, torch.softmax(logits, 1)) < BOUND
    assert torch.equal(yhat, torch.argmax(logits, 1))
    want = torch.zeros(C, 2, dtype=torch.int32)
    for y, hh in zip(label.tolist(), torch.argmax(logits, 1).tolist()):
        want[y, 0] += 1
        want[y, 1] += int(y == hh)
    assert torch.equal(stats, want) and stats.dtype == torch.int32
    (gl,) = torch.autograd.grad(0.7 * ref + (lg * dl_in).sum(), lg)
    assert _err(T.ce_dlogits_ref(prob, label, 0.7, dl_in), gl) < BOUND
    assert _err(T.ce_dlogits_ref(prob, label, 0.7, None), gl - dl_in) < BOUND


def test_ce_ref_ties_and_labels_out_of_range():
    logits = torch.tensor([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [3.0, 1.0, 3.0], [0.1, 0.2, 0.3]], dtype=torch.float64)
    loss, prob, yhat, stats = T.ce_ref(logits, torch.tensor([0, 2, 2, 1]))
    assert yhat.tolist() == [0, 1, 0, 2]                           # the first index of the maximum
    assert stats.tolist() == [[1, 1], [1, 0], [2, 0]]
    loss, prob2, yhat2, stats = T.ce_ref(logits, torch.tensor([0, -1, 3, 1]))
    assert torch.isnan(loss) and torch.equal(prob, prob2) and torch.equal(yhat, yhat2)
    assert stats.tolist() == [[1, 1], [1, 0], [0, 0]]


def test_gelu_grad_ref_is_the_derivative_of_the_erf_gelu():
    x = torch.cat([torch.randn(1000, generator=_gen(3), dtype=torch.float64) * 2,
                   torch.tensor([0.0, 1e-4, -1e-4, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0], dtype=torch.float64)])
    xr = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(F.gelu(xr).sum(), xr)
    assert (T.gelu_grad_ref(x) - gx).abs().max().item() < BOUND
    assert T.gelu_grad_ref(torch.tensor([40.0, -40.0])).tolist() == [1.0, 0.0]


@pytest.mark.parametrize("D", [4, 64])
def test_ppeg_fold_ref_is_the_oracle_ppeg_as_one_7x7_kernel(D):
    from oracle.transmil_ref import PPEG
    torch.manual_seed(D)
    ref = PPEG(D).double()
    G = 9
    x = torch.randn(2, 1 + G * G, D, generator=_gen(D), dtype=torch.float64)
    with torch.no_grad():
        want = ref(x, G, G)
        wf, bf = T.ppeg_fold_ref(ref.proj.weight, ref.proj.bias, ref.proj1.weight, ref.proj1.bias,
                                 ref.proj2.weight, ref.proj2.bias)
        assert wf.shape == (49, D) and bf.shape == (D,)
        grid = x[:, 1:].transpose(1, 2).reshape(2, D, G, G)
        got = F.conv2d(grid, wf.t().reshape(D, 1, 7, 7), bf, 1, 3, groups=D).flatten(2).transpose(1, 2)
    assert _err(got, want[:, 1:]) < BOUND
    assert torch.equal(want[:, 0], x[:, 0])


def test_tail_entry_points_refuse_bad_arguments():
    """A status path: nothing is launched (every pointer is null; the shape checks come first)."""
    from transmil_deepgraft_amd import _lib
    lib = _lib.lib()
    N = None
    width = "layernorm: D must be 64/128/256/384/512/768/1024"

    def ln_fwd(rows=14, D=512, S=7, n_pad=16, pad=5):
        return lib.tm_layernorm_fwd(N, N, N, EPS, rows, D, S, n_pad, pad, 0, N, N, N, N)

    def ln_bwd(rows=14, D=512, S=7, n_pad=16, pad=5, rpb=16):
        return lib.tm_layernorm_bwd(N, 0, N, N, N, N, rows, D, S, n_pad, pad, rpb, 0, N, N, N, N, N, N)

    def ln_seg(rows=14, D=512, S=7, n_pad=16, pad=5, rpb=16, dtype=1, seg_len=2, nseg=8, seg_rows=32):
        return lib.tm_layernorm_bwd_seg(N, dtype, N, N, N, N, rows, D, S, n_pad, pad, rpb, 0, N, seg_len, nseg,
                                        seg_rows, N, N, N, N, N, N)

    def head_fwd(B=2, S=3, D=512, C=2):
        return lib.tm_head_fwd(N, B, S, D, N, N, EPS, N, N, C, N, N, N, N)

    def head_bwd(B=2, C=2, S=3, D=512):
        return lib.tm_head_bwd(N, B, C, S, D, N, N, N, N, N, N, N, N, N, N, N)

    def head_ce_fwd(B=2, S=3, D=512, C=2):
        return lib.tm_head_ce_fwd(N, B, S, D, N, N, EPS, N, N, C, N, N, N, N, N, N, N, N, N)

    def head_ce_bwd(B=2, C=2, S=3, D=512):
        return lib.tm_head_ce_bwd(N, N, N, N, B, C, S, D, N, N, N, N, N, N, N, N, N, N, N, N)

    cases = [
        # an unsupported width, at every entry point that dispatches on it
        (lambda: ln_fwd(D=96), width), (lambda: ln_bwd(D=96), width), (lambda: ln_seg(D=96), width),
        (lambda: head_fwd(D=96), width), (lambda: head_bwd(D=96), width), (lambda: head_ce_fwd(D=96), width),
        (lambda: head_ce_bwd(D=96), width), (lambda: ln_bwd(D=0), width), (lambda: head_bwd(D=2048), width),
        # dy rows past the padded layout
        (lambda: ln_bwd(n_pad=11), "layernorm_bwd: n_pad < S + pad"),
        (lambda: ln_bwd(pad=-1), "layernorm_bwd: n_pad < S + pad"),
        (lambda: ln_bwd(rows=15), "layernorm_bwd: rows must be a multiple of S"),
        (lambda: ln_bwd(S=0), "layernorm_bwd: bad args"),
        (lambda: ln_bwd(rpb=0), "layernorm_bwd: bad args"),
        (lambda: ln_seg(n_pad=11), "layernorm_bwd_seg: n_pad < S + pad"),
        (lambda: ln_seg(rows=15), "layernorm_bwd_seg: rows must be a multiple of S"),
        (lambda: ln_seg(nseg=5), "layernorm_bwd_seg: rows past the segments"),
        (lambda: ln_seg(seg_rows=8), "layernorm_bwd_seg: bad args"),
        (lambda: ln_seg(dtype=0), "layernorm_bwd_seg: bf16 dy only"),
        # the class row of a bag is row b * S
        (lambda: head_fwd(S=0), "head_fwd: S must be at least 1"),
        (lambda: head_bwd(S=0), "head_bwd: S must be at least 1"),
        (lambda: head_ce_fwd(S=-2), "head_ce_fwd: S must be at least 1"),
        (lambda: head_ce_bwd(S=0), "head_ce_bwd: S must be at least 1"),
        (lambda: head_bwd(B=0), "head_bwd: empty logits"),
        (lambda: head_ce_bwd(C=0), "head_ce_bwd: empty logits"),
        # in range, but no pointers
        (ln_fwd, "layernorm_fwd: bad args"), (ln_bwd, "layernorm_bwd: null arg"),
        (ln_seg, "layernorm_bwd_seg: null arg"), (head_fwd, "head_fwd: bad args"),
        (head_bwd, "head_bwd: null arg"), (head_ce_fwd, "head_ce_fwd: bad args"),
        (head_ce_bwd, "head_ce_bwd: null arg"),
        # glue
        (lambda: lib.tm_ce_fwd(N, N, 0, 2, N, N, N, N, N), "ce_fwd: empty logits"),
        (lambda: lib.tm_ce_fwd(N, N, 2, 2, N, N, N, N, N), "ce_fwd: null arg"),
        (lambda: lib.tm_ce_bwd(N, N, 0, 2, N, N, N), "ce_bwd: empty logits"),
        (lambda: lib.tm_ce_bwd(N, N, 2, 0, N, N, N), "ce_bwd: empty logits"),
        (lambda: lib.tm_ce_bwd(N, N, 2, 2, N, N, N), "ce_bwd: null arg"),
        (lambda: lib.tm_put_cls(N, 0, 4, 64, N, N), "put_cls: bad shape"),
        (lambda: lib.tm_put_cls(N, 3, 0, 64, N, N), "put_cls: bad shape"),
        (lambda: lib.tm_put_cls(N, 3, 4, 64, N, N), "put_cls: null arg"),
    ]
    for i, (fn, text) in enumerate(cases):
        rc = fn()
        assert rc != 0 and _lib.last_error() == text, (i, rc, text, _lib.last_error())
