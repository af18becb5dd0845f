"""Kernel-level checks on the MI355X of layernorm.hip and the small kernels of glue.hip: the
LayerNorm forward and backward at every dispatch width, the class-token head and the fused head +
cross-entropy on both of their code paths, tm_step_prepare / tm_cast_f32_many / tm_cast_f32, and
tm_gelu_bwd / tm_gelu_bwd_pre / tm_add_relu / tm_put_cls.  Each is called through the C ABI as
engine.py calls it and compared with the fp64 restatements of tests/tail_refs.py and
tests/kernel_refs.py on the same, already-rounded operands (or bit for bit with PyTorch / a second
kernel path).  Outputs are prefilled with a NaN or 7.0 sentinel; every test prints the figures it
then asserts on (pytest -s shows them)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

import kernel_refs as R
import tail_refs as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = 7.0
EPS = 1e-5
WIDTHS = [64, 128, 256, 384, 512, 768, 1024]        # every TM_VPL_DISPATCH case
F32T, BF16T = torch.float32, torch.bfloat16


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
    return BF16 if dtype == BF16T else F32


def _dev(*ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16T else torch.int32)


def _affine(D, g):
    """gamma in [0.5, 1.5], beta in [-0.2, 0.2]."""
    return torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) * 0.4 - 0.2


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


# ============================================================================= a. tm_layernorm_fwd
LN_FWD_LAYOUTS = [(2, 7, 5, 16), (1, 1, 0, 1), (3, 5, 3, 8)]      # (B, S, pad, n_pad)


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_fwd_padded_layout_every_width(D, dtype):
    """tm_layernorm_fwd at every dispatch width, fp32 and bf16 output, in three layouts (B, S, pad,
    n_pad): (2, 7, 5, 16) -- 14 data rows and 10 pad rows, so the data rows and the zeroing rows both
    end inside a 4-row block, the second bag's pad rows are zeroed by the blocks past the data, four
    tail rows per bag; (1, 1, 0, 1); (3, 5, 3, 8) -- no tail.  x = 0.3 + 1.5 randn; row 0 is the
    constant 2.5 (its fp32 mean is exactly 2.5 at all seven widths, so y == T(beta) bitwise there); row
    1 is 1e-3 randn (variance of the order of eps: a dropped or misplaced eps shows).  y is one row
    longer than the layout and prefilled with 7.
      - pad rows exactly zero; tail rows and the extra row keep the sentinel;
      - mean, rstd within 1e-6 of fp64: in the max norm over the rows, rstd also element by element
        (it is well conditioned: var + eps >= eps), and the mean of every row within 1e-6 of that
        row's mean |x| (the error of a sum scales with its terms, not with what is left after they
        cancel: the mean of row 1 is far smaller than its elements);
      - fp32 y: max-norm error < 1e-5 of the largest reference entry (test_layernorm_fwd_bwd's bound);
      - bf16 y: element by element |y - ref| <= 2^-8 |ref| + 1e-5 max|ref|: one bf16 rounding (half an
        ulp, 2^-8 relative) of a value within the fp32 bound.
    The bitwise claim on the constant row failed at D = 384 with bf16 output before ln_fwd_kernel's mean
    was pinned to one rounded product (mul_rounded, layernorm.hip): that instantiation alone had the
    product fused into `v - mean`.
    Measured on the MI355X (max over the widths and layouts): mean 2.4e-8 (max norm) / 4.6e-8 (per row),
    rstd 8.0e-8 (max norm) / 1.2e-7 (elementwise), fp32 y 1.8e-7, bf16 y 0.98 of its bound."""
    L = _lib()
    _p, _stream = _eng()
    for B, S, pad, n_pad in LN_FWD_LAYOUTS:
        g = _gen(D * 31 + S)
        rows = B * S
        x = 0.3 + 1.5 * torch.randn(rows, D, generator=g)
        x[0] = 2.5
        if rows > 1:
            x[1] = 1e-3 * torch.randn(D, generator=g)
        gamma, beta = _affine(D, g)
        ref_y, ref_mean, ref_rstd = T.ln_fwd_ref(x, gamma, beta, EPS, S, n_pad, pad)
        xd, gd, bd = _dev(x, gamma, beta)
        y = torch.full((B * n_pad + 1, D), SENTINEL, dtype=dtype, device=DEV)
        mean = torch.full((rows,), NAN, device=DEV)
        rstd = torch.full((rows,), NAN, device=DEV)
        L.call("tm_layernorm_fwd", _p(xd), _p(gd), _p(bd), C.c_float(EPS), rows, D, S, n_pad, pad, _tt(dtype), _p(y),
               _p(mean), _p(rstd), _stream())
        torch.cuda.synchronize()
        out = y.cpu()
        assert (out[-1].float() == SENTINEL).all()
        out = out[:-1].view(B, n_pad, D)
        assert (_bits(out[:, :pad]) == 0).all()
        assert (out[:, pad + S:].float() == SENTINEL).all()
        data, want = out[:, pad:pad + S].float(), ref_y[:, pad:pad + S]
        assert torch.isfinite(data).all()
        # statistics
        mean, rstd = mean.cpu(), rstd.cpu()
        assert mean[0].item() == 2.5
        assert torch.equal(_bits(out[0, pad]), _bits(beta.to(dtype)))
        e_mean, e_rstd = _rel(mean, ref_mean), _rel(rstd, ref_rstd)
        e_rstd_el = ((rstd.double() - ref_rstd).abs() / ref_rstd).max().item()
        e_mean_row = ((mean.double() - ref_mean).abs() / x.double().abs().mean(-1)).max().item()
        tag = f"{D, dtype, (B, S, pad, n_pad)}"
        _report(f"ln fwd mean (max norm, per row / mean|x|), rstd (max norm, elementwise) {tag}",
                (e_mean, e_mean_row, e_rstd, e_rstd_el))
        assert e_mean < 1e-6 and e_mean_row < 1e-6 and e_rstd < 1e-6 and e_rstd_el < 1e-6
        if dtype == F32T:
            e = _rel(data, want)
            _report(f"ln fwd y fp32 {tag}", e)
            assert e < 1e-5
        else:
            bound = 2.0 ** -8 * want.abs() + 1e-5 * want.abs().max()
            ratio = ((data.double() - want).abs() / bound).max().item()
            _report(f"ln fwd y bf16, max |err| / bound {tag}", ratio)
            assert ratio <= 1.0


# ============================================================================= b. LayerNorm backward
LN_BWD_SHAPE = (2, 37, 48, 3)                              # (B, S, n_pad, pad): 74 rows
SEG_LEN, NSEG, SEG_ROWS = 2, 24, 32                        # not the step's geometry (n / 256, 256, 288)
# every width at 16 rows per block (a bag boundary inside block 2), and 3 (fewer rows than waves, a
# last block of 2, 25 partials) / 64 (a short second block) at the scalar-path and the widest width
LN_BWD_CASES = [(D, 16) for D in WIDTHS] + [(D, rpb) for D in (384, 1024) for rpb in (3, 64)]


@functools.lru_cache(maxsize=4)
def _ln_bwd_operands(D, dtype, with_seg):
    B, S, n, pad = LN_BWD_SHAPE
    g = _gen(D + 1000 * with_seg)
    x = torch.randn(B * S, D, generator=g) * 1.5 + 0.3
    gamma = torch.rand(D, generator=g) + 0.5
    mean = x.double().mean(-1).float()
    rstd = (1.0 / torch.sqrt(x.double().var(-1, unbiased=False) + EPS)).float()
    dy = torch.randn(B, n, D, generator=g).to(dtype)
    dy[:, :pad] = NAN                                   # pad rows of dy are never read
    acc = torch.randn(B * S, D, generator=g)
    seg = None
    if with_seg:                                         # every row distinct: a wrong segment index cannot cancel
        seg = torch.randn(B, SEG_ROWS, D, generator=g) + torch.arange(SEG_ROWS).view(1, SEG_ROWS, 1) * 0.01
    return x, gamma, mean, rstd, dy, acc, seg


def _ln_bwd_run(entry, D, rpb, dtype, resid, ops, queued):
    L = _lib()
    _p, _stream = _eng()
    B, S, n, pad = LN_BWD_SHAPE
    x, gamma, mean, rstd, dy, acc, seg = ops
    acc_in = acc.clone()
    if resid:
        acc_in.view(B, S, D)[:, 1:] = NAN               # written without being read
    xd, gd, md, rd, dyd, dx = _dev(x, gamma, mean, rstd, dy, acc_in)
    work = torch.full((L.query("tm_layernorm_bwd_workspace", B * S, D, rpb) // 4,), NAN, device=DEV)
    dg = torch.full((D,), NAN, device=DEV)
    db = torch.full((D,), NAN, device=DEV)

    def launch(rq):
        if entry == "tm_layernorm_bwd":
            L.call(entry, _p(dyd), _tt(dtype), _p(xd), _p(gd), _p(md), _p(rd), B * S, D, S, n, pad, rpb, resid, _p(dx),
                   _p(work), _p(dg), _p(db), rq, _stream())
        else:
            segd = seg.to(DEV)
            L.call(entry, _p(dyd), _tt(dtype), _p(xd), _p(gd), _p(md), _p(rd), B * S, D, S, n, pad, rpb, resid,
                   _p(segd), SEG_LEN, NSEG, SEG_ROWS, _p(dx), _p(work), _p(dg), _p(db), rq, _stream())
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


def _ln_bwd_check(entry, D, rpb, dtype, resid, with_seg):
    B, S, n, pad = LN_BWD_SHAPE
    ops = _ln_bwd_operands(D, dtype, with_seg)
    x, gamma, mean, rstd, dy, acc, seg = ops
    now = _ln_bwd_run(entry, D, rpb, dtype, resid, ops, queued=False)
    later = _ln_bwd_run(entry, D, rpb, dtype, resid, ops, queued=True)
    for a, b in zip(now[:3], later[:3]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    ref = R.ln_bwd_seg_ref(dy, x, gamma, mean, rstd, S, pad, now[3], resid, seg=seg, seg_len=SEG_LEN, nseg=NSEG)
    errs = tuple(_rel(a, b) for a, b in zip(now[:3], ref))
    _report(f"{entry} (dx, dgamma, dbeta) {D, rpb, dtype, resid}", errs)
    assert all(e < 1e-4 for e in errs), errs


@pytest.mark.parametrize("resid_cls_only", [0, 1])
@pytest.mark.parametrize("dtype", [BF16T, F32T])
@pytest.mark.parametrize("D,rpb", LN_BWD_CASES)
def test_layernorm_bwd_every_width_and_block_size(D, rpb, dtype, resid_cls_only):
    """tm_layernorm_bwd at every dispatch width (16 rows per block) and at 3 / 64 rows per block
    (D = 384, the scalar load / store path, and 1024), (B, S, n_pad, pad) = (2, 37, 48, 3): dy in
    fp32 / bf16 from the front-padded layout (pad rows NaN: never read; every width but 512 reads
    bf16 dy element by element), resid_cls_only 0 / 1 (1: the non-class rows of dx_accum hold NaN on
    entry and come out finite), the workspace NaN-filled, mean / rstd computed in fp64 and rounded.
    The immediate reduce and a caller-owned queue flushed afterwards give the same bits (3 rows per
    block: 25 partials, the several-lanes form of the reduce); dx, dgamma, dbeta within 1e-4 of
    kernel_refs.ln_bwd_seg_ref (the bound of test_layernorm_bwd_step_form).
    Measured on the MI355X (max over the cases): dx 1.5e-7, dgamma 2.7e-7, dbeta 1.3e-7; the two
    reduce forms bit-equal in every case."""
    _ln_bwd_check("tm_layernorm_bwd", D, rpb, dtype, resid_cls_only, False)


@pytest.mark.parametrize("resid_cls_only", [0, 1])
@pytest.mark.parametrize("D,rpb", LN_BWD_CASES)
def test_layernorm_bwd_seg_every_width_and_block_size(D, rpb, resid_cls_only):
    """tm_layernorm_bwd_seg (bf16 dy) on the same shapes with a segment geometry the step does not
    use, seg_add [B][32][D], seg_len = 2, nseg = 24, every seg_add row distinct: dy_eff[b][t] =
    dy[b][pad+t] + seg[b][(pad+t) // 2] + (t == 0) seg[b][24]; the checks of
    test_layernorm_bwd_every_width_and_block_size.
    Measured on the MI355X (max over the cases): dx 1.1e-7, dgamma 1.2e-7, dbeta 1.4e-7."""
    _ln_bwd_check("tm_layernorm_bwd_seg", D, rpb, BF16T, resid_cls_only, True)


# ============================================================================= c. head, head + CE
HEAD_S = 3
HEAD_WIDTHS = [64, 384, 512, 1024]      # VPL 1, the scalar path, the shipped width, the widest
# (1, 2) / (1, 4): the one-bag fast path and its limit; (1, 5): one bag on the general path; (5, 7):
# more bags than HEAD_CE_WAVES; (300, 2): more bags than the 256 threads of the CE loop
HEAD_BC = [(1, 2), (1, 4), (1, 5), (2, 3), (5, 7)]
HEAD_CASES = [(D, B, Cc) for D in HEAD_WIDTHS for B, Cc in HEAD_BC] + [(64, 300, 2)]
GLOSS = 0.7


@functools.lru_cache(maxsize=2)
def _head_case(D, B, Cc):
    """Operands of one head case and the fp64 forward on them.  h holds NaN outside row 0 of every
    bag.  The backward's inputs are the fp32-rounded fp64 forward (xhat, rstd, prob), so that the
    backward reference sees exactly what the kernels see."""
    g = _gen(D * 7 + B * 13 + Cc)
    h = torch.full((B, HEAD_S, D), NAN)
    h[:, 0] = 0.3 + 1.5 * torch.randn(B, D, generator=g)
    gamma, beta = _affine(D, g)
    W = torch.randn(Cc, D, generator=g) * (2.0 / D ** 0.5)
    bias = torch.randn(Cc, generator=g) * 0.1
    label = torch.randint(0, Cc, (B,), generator=g)
    dl_in = torch.randn(B, Cc, generator=g) * 0.3
    logits, xhat, rstd = T.head_ref(h.view(B * HEAD_S, D), HEAD_S, gamma, beta, EPS, W, bias)
    _, prob, _, _ = T.ce_ref(logits, label)
    return SimpleNamespace(h=h, gamma=gamma, beta=beta, W=W, bias=bias, label=label, dl_in=dl_in, logits=logits,
                           xhat=xhat, rstd=rstd, xhat32=xhat.float(), rstd32=rstd.float(), prob32=prob.float())


def _head_fwd_launch(c, D, B, Cc, fused, label=None, stats=None, W=None, bias=None):
    """tm_head_fwd (fused = False) or tm_head_ce_fwd: outputs prefilled with NaN."""
    L = _lib()
    _p, _stream = _eng()
    hd, gd, bd, Wd, biasd = _dev(c.h, c.gamma, c.beta, c.W if W is None else W, c.bias if bias is None else bias)
    o = SimpleNamespace(logits=torch.full((B, Cc), NAN, device=DEV), xhat=torch.full((B, D), NAN, device=DEV),
                        rstd=torch.full((B,), NAN, device=DEV), loss=torch.full((1,), NAN, device=DEV),
                        prob=torch.full((B, Cc), NAN, device=DEV),
                        yhat=torch.full((B,), -7, dtype=torch.int64, device=DEV))
    if fused:
        labd = (c.label if label is None else label).to(DEV)
        L.call("tm_head_ce_fwd", _p(hd), B, HEAD_S, D, _p(gd), _p(bd), C.c_float(EPS), _p(Wd), _p(biasd), Cc, _p(labd),
               _p(o.logits), _p(o.xhat), _p(o.rstd), _p(o.loss), _p(o.prob), _p(o.yhat), _p(stats), _stream())
    else:
        L.call("tm_head_fwd", _p(hd), B, HEAD_S, D, _p(gd), _p(bd), C.c_float(EPS), _p(Wd), _p(biasd), Cc, _p(o.logits),
               _p(o.xhat), _p(o.rstd), _stream())
    torch.cuda.synchronize()
    return o


def _ce_launch(logits, label, stats):
    """tm_ce_fwd on fp32 logits: (loss, prob, yhat), prefilled with NaN / -7."""
    L = _lib()
    _p, _stream = _eng()
    B, Cc = logits.shape
    lg, lab = _dev(logits, label)
    loss = torch.full((1,), NAN, device=DEV)
    prob = torch.full((B, Cc), NAN, device=DEV)
    yhat = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    L.call("tm_ce_fwd", _p(lg), _p(lab), B, Cc, _p(loss), _p(prob), _p(yhat), _p(stats), _stream())
    torch.cuda.synchronize()
    return loss, prob, yhat


def _ce_check(tag, logits32, label, loss, prob, yhat, stats_before=None, stats_after=None):
    """loss / prob / yhat / class stats of one CE launch against ce_ref on the fp32 logits the kernel
    read (the bounds of test_fused_cross_entropy_matches_torch: 1e-6 relative + 1e-6 / 1e-7 absolute)."""
    r_loss, r_prob, r_yhat, r_stats = T.ce_ref(logits32, label)
    e_prob = ((prob.cpu().double() - r_prob).abs() / (1e-7 + 1e-6 * r_prob)).max().item()
    assert torch.equal(yhat.cpu(), r_yhat)
    if torch.isnan(r_loss):
        assert torch.isnan(loss.cpu()).all()
        e_loss = 0.0
    else:
        e_loss = abs(loss.item() - r_loss.item()) / (1e-6 + 1e-6 * abs(r_loss.item()))
    _report(f"{tag} (loss, prob) error / bound", (e_loss, e_prob))
    assert e_loss <= 1.0 and e_prob <= 1.0
    if stats_after is not None:
        assert torch.equal(stats_after.cpu(), stats_before + r_stats)


@pytest.mark.parametrize("D,B,Cc", HEAD_CASES)
def test_head_forward_and_cross_entropy_against_fp64(D, B, Cc):
    """tm_head_fwd, tm_head_ce_fwd and tm_ce_fwd, S = 3 with h NaN outside row 0 of every bag:
      - logits within 1e-5, xhat within 1e-5 and rstd within 1e-6 (max norm) of tail_refs.head_ref,
        from both head entry points;
      - loss and prob within 1e-6 of tail_refs.ce_ref on the fp32 logits the launch itself produced
        (tm_head_ce_fwd) or was given (tm_ce_fwd), yhat equal to the reference's first-index argmax;
      - class_stats starts from non-zero counts and grows by the reference's (count, correct); the
        same calls once more with class_stats = NULL.
    Measured on the MI355X (max over the cases): logits 2.8e-7, xhat 1.5e-7, rstd 9.7e-8; the loss at
    most 0.07 and prob at most 0.11 of their bounds (tm_ce_fwd and tm_head_ce_fwd alike)."""
    c = _head_case(D, B, Cc)
    start = (torch.arange(2 * Cc, dtype=torch.int32) + 3).view(Cc, 2)
    for fused in (False, True):
        stats = start.clone().to(DEV) if fused else None
        o = _head_fwd_launch(c, D, B, Cc, fused, stats=stats)
        errs = (_rel(o.logits, c.logits), _rel(o.xhat, c.xhat), _rel(o.rstd, c.rstd))
        _report(f"head fwd (logits, xhat, rstd) {D, B, Cc, fused}", errs)
        assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[2] < 1e-6, errs
        if fused:
            _ce_check(f"head_ce_fwd {D, B, Cc}", o.logits.cpu(), c.label, o.loss, o.prob, o.yhat, start, stats)
            o2 = _head_fwd_launch(c, D, B, Cc, True, stats=None)
            _ce_check(f"head_ce_fwd, no stats {D, B, Cc}", o2.logits.cpu(), c.label, o2.loss, o2.prob, o2.yhat)
    logits32 = c.logits.float()
    stats = start.clone().to(DEV)
    loss, prob, yhat = _ce_launch(logits32, c.label, stats)
    _ce_check(f"ce_fwd {B, Cc}", logits32, c.label, loss, prob, yhat, start, stats)
    loss, prob, yhat = _ce_launch(logits32, c.label, None)
    _ce_check(f"ce_fwd, no stats {B, Cc}", logits32, c.label, loss, prob, yhat)


@pytest.mark.parametrize("D,B,Cc", [(64, 5, 3), (512, 1, 2), (384, 2, 4)])
def test_head_argmax_takes_the_lower_index_on_a_tie(D, B, Cc):
    """Rows 0 and 1 of W identical with equal bias (every other class pushed down by its bias): the two
    logits are bit-equal in every bag and yhat must be 0, from tm_head_ce_fwd and from tm_ce_fwd."""
    c = _head_case(D, B, Cc)
    W, bias = c.W.clone(), c.bias.clone()
    W[1] = W[0]
    bias[1] = bias[0]
    bias[2:] = -100.0
    label = torch.ones(B, dtype=torch.int64)
    stats = torch.zeros(Cc, 2, dtype=torch.int32, device=DEV)
    o = _head_fwd_launch(c, D, B, Cc, True, label=label, stats=stats, W=W, bias=bias)
    lg = o.logits.cpu()
    assert torch.equal(_bits(lg[:, 0]), _bits(lg[:, 1])) and (lg[:, 2:] < lg[:, :1]).all()
    assert (o.yhat.cpu() == 0).all()
    assert stats.cpu()[1].tolist() == [B, 0]
    _, _, yhat = _ce_launch(lg, label, None)
    assert (yhat.cpu() == 0).all()


@pytest.mark.parametrize("D,B,Cc", [(64, 5, 7), (512, 5, 7), (64, 300, 2)])
def test_cross_entropy_label_out_of_range(D, B, Cc):
    """One label at -1 and one at C (the header documents it, ce_fwd_kernel / head_ce_fwd_kernel guard
    it): the loss is NaN, prob and yhat are still right, those rows are left out of class_stats.
    Forward entry points only."""
    c = _head_case(D, B, Cc)
    label = c.label.clone()
    label[1] = -1
    label[B - 2] = Cc
    start = (torch.arange(2 * Cc, dtype=torch.int32) + 3).view(Cc, 2)
    stats = start.clone().to(DEV)
    o = _head_fwd_launch(c, D, B, Cc, True, label=label, stats=stats)
    assert torch.isnan(o.loss.cpu()).all()
    _ce_check(f"head_ce_fwd, bad labels {D, B, Cc}", o.logits.cpu(), label, o.loss, o.prob, o.yhat, start, stats)
    logits32 = c.logits.float()
    stats = start.clone().to(DEV)
    loss, prob, yhat = _ce_launch(logits32, label, stats)
    assert torch.isnan(loss.cpu()).all()
    _ce_check(f"ce_fwd, bad labels {B, Cc}", logits32, label, loss, prob, yhat, start, stats)


def _head_bwd_launch(c, D, B, Cc, dlogits=None, dl_in=None):
    """tm_head_bwd (dlogits given) or tm_head_ce_bwd on the fp32-rounded fp64 forward: (dW, dbias,
    dgamma, dbeta, dh [B, S, D], scratch); parameter gradients prefilled with NaN, dh with 7, the
    scratch (NULL on the one-bag fast path) with NaN."""
    L = _lib()
    _p, _stream = _eng()
    xh, rs, gd, bd, Wd = _dev(c.xhat32, c.rstd32, c.gamma, c.beta, c.W)
    dW = torch.full((Cc, D), NAN, device=DEV)
    dbias = torch.full((Cc,), NAN, device=DEV)
    dgamma = torch.full((D,), NAN, device=DEV)
    dbeta = torch.full((D,), NAN, device=DEV)
    dh = torch.full((B, HEAD_S, D), SENTINEL, device=DEV)
    scratch = None
    if dlogits is not None:
        dld = dlogits.to(DEV).contiguous()
        L.call("tm_head_bwd", _p(dld), B, Cc, HEAD_S, D, _p(xh), _p(rs), _p(gd), _p(bd), _p(Wd), _p(dW), _p(dbias),
               _p(dgamma), _p(dbeta), _p(dh), _stream())
    else:
        fast = B == 1 and Cc <= 4
        scratch = None if fast else torch.full((B * Cc,), NAN, device=DEV)
        probd, labd = _dev(c.prob32, c.label)
        gl = torch.tensor([GLOSS], device=DEV)
        dind = None if dl_in is None else dl_in.to(DEV)
        L.call("tm_head_ce_bwd", _p(probd), _p(labd), _p(gl), _p(dind), B, Cc, HEAD_S, D, _p(xh), _p(rs), _p(gd),
               _p(bd), _p(Wd), _p(dW), _p(dbias), _p(dgamma), _p(dbeta), _p(dh), _p(scratch), _stream())
    torch.cuda.synchronize()
    return [t.cpu() for t in (dW, dbias, dgamma, dbeta, dh)], None if scratch is None else scratch.cpu()


@pytest.mark.parametrize("with_dl_in", [False, True])
@pytest.mark.parametrize("D,B,Cc", HEAD_CASES)
def test_head_backward_against_fp64_on_both_paths(D, B, Cc, with_dl_in):
    """tm_head_ce_bwd (gloss = 0.7, dlogits_in NULL / random, scratch NULL on the one-bag fast path and
    NaN-filled [B*C] otherwise), tm_head_bwd and tm_ce_bwd:
      - dW, dbias, dgamma, dbeta and row 0 of dh of tm_head_ce_bwd within 1e-5 of
        tail_refs.head_bwd_ref(ce_dlogits_ref(...)); rows 1..S-1 of dh keep the sentinel;
      - the same from tm_head_bwd fed the fp32-rounded reference dlogits;
      - tm_head_bwd against tm_head_ce_bwd bit for bit.  The rounded fp64 dlogits cannot serve here:
        the fused kernel forms fp32(g / B) (prob - one_hot) + dlogits_in in fp32, which differs from
        the rounded fp64 value in the last bit of about half the entries whenever g / B is inexact
        (B = 5, 300) or the sum rounds.  So tm_head_bwd is fed the dlogits the fused launch itself
        formed -- its scratch on the general path, its dbias (= dlogits when B = 1) on the fast path --
        after those are checked within 1e-6 of ce_dlogits_ref; then all five outputs are bit-equal;
      - tm_ce_bwd within 1e-6 of ce_dlogits_ref (dlogits_in = NULL).
    The bit-for-bit claim failed on its first case (D = 64, B = 1, C = 2: dh two fp32 ulps apart)
    while head_bwd_kernel, head_ce_bwd_kernel and head_bwd_b1 were three copies of the formulas: fp
    contraction fused different products in each.  They now share one body compiled with contraction
    off (head_bwd.h).
    Measured on the MI355X (max over the cases): dW 4.6e-7, dbias 4.2e-7, dgamma 4.5e-7, dbeta 8.4e-7,
    dh 1.8e-7 (both entry points); the fused launch's dlogits 9.7e-8, tm_ce_bwd 9.1e-8."""
    c = _head_case(D, B, Cc)
    dl_in = c.dl_in if with_dl_in else None
    ref_dl = T.ce_dlogits_ref(c.prob32, c.label, torch.tensor(GLOSS).item(), dl_in)
    ref = T.head_bwd_ref(ref_dl, c.xhat32, c.rstd32, c.gamma, c.beta, c.W)
    fused, scratch = _head_bwd_launch(c, D, B, Cc, dl_in=dl_in)
    split, _ = _head_bwd_launch(c, D, B, Cc, dlogits=ref_dl.float())
    for name, got in (("head_ce_bwd", fused), ("head_bwd", split)):
        assert (got[4][:, 1:] == SENTINEL).all()
        errs = tuple(_rel(a, b) for a, b in zip(got[:4] + [got[4][:, 0]], ref))
        _report(f"{name} (dW, dbias, dgamma, dbeta, dh) {D, B, Cc, with_dl_in}", errs)
        assert all(e < 1e-5 for e in errs), (name, errs)
    own_dl = fused[1].view(1, Cc) if scratch is None else scratch.view(B, Cc)
    e_dl = _rel(own_dl, ref_dl)
    _report(f"head_ce_bwd dlogits {D, B, Cc, with_dl_in}", e_dl)
    assert e_dl < 1e-6
    twin, _ = _head_bwd_launch(c, D, B, Cc, dlogits=own_dl)
    for a, b in zip(twin, fused):
        assert torch.equal(_bits(a), _bits(b))
    if not with_dl_in:
        L = _lib()
        _p, _stream = _eng()
        probd, labd = _dev(c.prob32, c.label)
        gl = torch.tensor([GLOSS], device=DEV)
        dl = torch.full((B * Cc + 8,), SENTINEL, device=DEV)
        L.call("tm_ce_bwd", _p(probd), _p(labd), B, Cc, _p(gl), _p(dl), _stream())
        torch.cuda.synchronize()
        assert (dl[B * Cc:].cpu() == SENTINEL).all()
        e = _rel(dl[:B * Cc].view(B, Cc), ref_dl)
        _report(f"ce_bwd dlogits {B, Cc}", e)
        assert e < 1e-6


# ============================================================================= d. casts, tm_step_prepare
_SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, -0.0, float("inf"), float("-inf"), 3.3895e38, -3.3895e38, 1e-40,
             -1e-40, NAN]     # the two round-to-even ties, signed zeros, infinities, near the bf16 maximum, denormals, NaN
_NAN_AT = len(_SPECIALS) - 1
TAIL = 8


def _cast_src(n, g, specials):
    x = torch.randn(n, generator=g) * 3
    if specials:
        k = min(n, len(_SPECIALS))
        x[:k] = torch.tensor(_SPECIALS[:k])
    return x


def _cast_check(name, x, dst, dtype):
    """dst[:n] is the bit-exact copy (fp32) / x.to(bfloat16) bit for bit (the NaN compared with isnan
    only); dst[n:] keeps the sentinel."""
    n = x.numel()
    out = dst.cpu()
    assert (out[n:].float() == SENTINEL).all(), name
    got, want = out[:n], x.to(dtype)
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan), name
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), name


def _table(sizes, dtype, g, misalign=()):
    """(CastTable, sources on the CPU, destinations on the device, keep-alive list) of one cast
    table; tensor i in ``misalign`` has its src one float past a 16-byte boundary (i even) or its
    dst one element past one (i odd): the per-piece fallback of step_prepare_kernel."""
    from transmil_deepgraft_amd._lib import CastTable
    _p, _ = _eng()
    tab = CastTable()
    tab.count = len(sizes)
    srcs, dsts, keep = [], [], []
    off = 0
    for i, n in enumerate(sizes):
        x = _cast_src(n, g, specials=(i == 0 or n >= 16))
        shift_src = 1 if (i in misalign and i % 2 == 0) else 0
        shift_dst = 1 if (i in misalign and i % 2 == 1) else 0
        sbuf = torch.zeros(n + 1, device=DEV)
        sview = sbuf[shift_src:shift_src + n]
        sview.copy_(x)
        dbuf = torch.full((n + TAIL + 1,), SENTINEL, dtype=dtype, device=DEV)
        dview = dbuf[shift_dst:]
        assert sbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
        tab.src[i] = sbuf.data_ptr() + 4 * shift_src          # non-null for an empty tensor as well
        tab.dst[i] = dview.data_ptr()
        tab.offset[i] = off
        off += n
        srcs.append(x)
        dsts.append(dview)
        keep += [sbuf, dbuf]
    tab.offset[len(sizes)] = off
    return tab, srcs, dsts, keep


CAST_TABLES = [
    ((4, 1020, 260), ()),        # tensor boundaries inside a wave's 256-element span, the table ends mid-wave
    ((4100,), ()),               # two cast blocks of CAST_PIECES * 1024
    ((256, 0, 256), ()),         # an empty tensor
    ((4,) * 8, ()),              # eight tensors
    ((512, 516, 260), (1, 2)),   # dst of tensor 1 and src of tensor 2 off their vector alignment
]


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("sizes,misalign", CAST_TABLES)
def test_step_prepare_and_cast_many_tables(sizes, misalign, dtype):
    """The cast table of tm_step_prepare (w7 = counter = cls = NULL: only the casts run) and of
    tm_cast_f32_many: TM_F32 is a bit-exact copy, TM_BF16 equals x.to(torch.bfloat16) bit for bit
    (round-to-even ties, signed zeros, infinities, the largest magnitudes, denormals; the NaN stays a
    NaN); every destination is 8 elements longer than its tensor and keeps the sentinel there."""
    L = _lib()
    _p, _stream = _eng()
    for entry in ("tm_step_prepare", "tm_cast_f32_many"):
        tab, srcs, dsts, keep = _table(sizes, dtype, _gen(sum(sizes) + len(sizes)), misalign)
        if entry == "tm_step_prepare":
            L.call(entry, _tt(dtype), C.byref(tab), *([None] * 6), 64, None, None, None, None, None, None, 0, 0, _stream())
        else:
            L.call(entry, _tt(dtype), C.byref(tab), _stream())
        torch.cuda.synchronize()
        for i, (x, d) in enumerate(zip(srcs, dsts)):
            _cast_check(f"{entry} tensor {i} of {sizes}", x, d, dtype)


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("count", [0, 1, 7, 8, 2047, 2048, 2049])
def test_cast_f32_counts(count, dtype):
    """tm_cast_f32 around its 8-element pieces and its 2048-element blocks: the cast semantics of
    test_step_prepare_and_cast_many_tables, the sentinel kept past `count`."""
    L = _lib()
    _p, _stream = _eng()
    x = _cast_src(count, _gen(count + 5), specials=True)
    xd = torch.zeros(count + TAIL, device=DEV)
    xd[:count] = x
    dst = torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_cast_f32", _tt(dtype), _p(xd), _p(dst), count, _stream())
    torch.cuda.synchronize()
    _cast_check(f"tm_cast_f32 {count}", x, dst, dtype)


def _ppeg_weights(D, g):
    return (torch.randn(D, 49, generator=g) * 0.2, torch.randn(D, generator=g) * 0.1,
            torch.randn(D, 25, generator=g) * 0.2, torch.randn(D, generator=g) * 0.1,
            torch.randn(D, 9, generator=g) * 0.2, torch.randn(D, generator=g) * 0.1)


@pytest.mark.parametrize("D", [64, 384])
def test_step_prepare_fold_counter_and_class_rows(D):
    """tm_step_prepare's other blocks, every switch both ways (49 D is no multiple of 256 at either
    width):
      - count = 0, the fold only (counter = cls = NULL): wfold / bfold against
        tail_refs.ppeg_fold_ref, element by element |err| <= 3 * 2^-24 (|w7| + |w5| + |w3| + 1) -- three
        fp32 additions, each rounding by at most 2^-24 of a partial sum that the sum of the magnitudes
        bounds -- and |err| <= 2 * 2^-24 (|b7| + |b5| + |b3|) for the two additions of the bias; both
        bit-equal to tm_ppeg_fold on the same weights; one element past each keeps the sentinel;
      - w7 = NULL with a one-tensor table, counter and cls set (B = 3, S = 5), called twice: wfold
        keeps the sentinel, the counter reads 1 then 2 and seed_out equals it each time, rows b * S of
        H equal cls and every other row keeps the sentinel;
      - the fold, the counter and the class rows in one call.
    Measured on the MI355X: wfold at most 0.34 and bfold at most 0.59 of their bounds; bit-equal to
    tm_ppeg_fold."""
    L = _lib()
    _p, _stream = _eng()
    from transmil_deepgraft_amd._lib import CastTable
    B, S = 3, 5
    g = _gen(D)
    w = _ppeg_weights(D, g)
    wd = _dev(*w)
    ref_wf, ref_bf = T.ppeg_fold_ref(*w)
    mag = w[0].double().abs().view(D, 7, 7).clone()
    mag[:, 1:6, 1:6] += w[2].double().abs().view(D, 5, 5)
    mag[:, 2:5, 2:5] += w[4].double().abs().view(D, 3, 3)
    wbound = 3 * 2.0 ** -24 * (mag.view(D, 49).t() + 1.0)
    bbound = 2 * 2.0 ** -24 * (w[1].double().abs() + w[3].double().abs() + w[5].double().abs())
    cls = torch.randn(D, generator=g)
    clsd = cls.to(DEV)
    empty = CastTable()
    empty.count = 0

    def outputs():
        return (torch.full((49 * D + 1,), SENTINEL, device=DEV), torch.full((D + 1,), SENTINEL, device=DEV),
                torch.full((B * S, D), SENTINEL, device=DEV))

    def check_fold(wf, bf):
        wf, bf = wf.cpu(), bf.cpu()
        assert wf[-1] == SENTINEL and bf[-1] == SENTINEL
        rw = ((wf[:-1].view(49, D).double() - ref_wf).abs() / wbound).max().item()
        rb = ((bf[:-1].double() - ref_bf).abs() / bbound).max().item()
        _report(f"step_prepare fold, max |err| / bound (wfold, bfold) D = {D}", (rw, rb))
        assert rw <= 1.0 and rb <= 1.0
        assert torch.equal(_bits(wf[:-1]), _bits(wf_sep)) and torch.equal(_bits(bf[:-1]), _bits(bf_sep))

    def check_cls(H):
        H = H.cpu().view(B, S, D)
        assert torch.equal(_bits(H[:, 0]), _bits(cls.expand(B, D))) and (H[:, 1:] == SENTINEL).all()

    wf_sep = torch.full((49 * D,), NAN, device=DEV)
    bf_sep = torch.full((D,), NAN, device=DEV)
    L.call("tm_ppeg_fold", *(_p(t) for t in wd), D, _p(wf_sep), _p(bf_sep), _stream())
    torch.cuda.synchronize()
    wf_sep, bf_sep = wf_sep.cpu(), bf_sep.cpu()
    # the fold only
    wf, bf, H = outputs()
    L.call("tm_step_prepare", 0, C.byref(empty), *(_p(t) for t in wd), D, _p(wf), _p(bf), None, None, None, None, 0, 0,
           _stream())
    torch.cuda.synchronize()
    check_fold(wf, bf)
    # no fold; one cast tensor, the counter (twice) and the class rows
    tab, srcs, dsts, keep = _table((260,), BF16T, g)
    wf, bf, H = outputs()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    seed = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    for step in (1, 2):
        L.call("tm_step_prepare", 1, C.byref(tab), *([None] * 6), D, _p(wf), _p(bf), _p(counter), _p(seed), _p(clsd),
               _p(H), B, S, _stream())
        torch.cuda.synchronize()
        assert counter.item() == step and seed.item() == step
    assert (wf.cpu() == SENTINEL).all() and (bf.cpu() == SENTINEL).all()
    check_cls(H)
    _cast_check("step_prepare with counter and cls", srcs[0], dsts[0], BF16T)
    # everything at once
    wf, bf, H = outputs()
    counter.fill_(41)
    L.call("tm_step_prepare", 0, C.byref(empty), *(_p(t) for t in wd), D, _p(wf), _p(bf), _p(counter), _p(seed),
           _p(clsd), _p(H), B, S, _stream())
    torch.cuda.synchronize()
    assert counter.item() == 42 and seed.item() == 42
    check_fold(wf, bf)
    check_cls(H)


# ============================================================================= e. elementwise glue
_GELU_FIXED = [0.0, 1e-4, -1e-4, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]


def _gelu_operands(count, g):
    pre = torch.randn(count, generator=g) * 2
    k = min(count, len(_GELU_FIXED))
    pre[:k] = torch.tensor(_GELU_FIXED[:k])
    dy = torch.randn(count, generator=g)
    return pre, dy


def _gelu_check(tag, dpre, pre_t, dy, count, dtype):
    """dpre[:count] against dy * gelu_grad_ref(pre as the kernel read it): 1e-6 (fp32) / 4e-3 (bf16) of
    the largest entry (the bounds of test_fc1_gelu_bwd_against_fp64); exactly dy and exactly 0 at
    pre = +-40 (the exponential underflows); the sentinel past `count`."""
    out = dpre.cpu()
    assert (out[count:].float() == SENTINEL).all()
    if count == 0:
        return
    got = out[:count].float()
    assert torch.isfinite(got).all()
    ref = dy.double() * T.gelu_grad_ref(pre_t.float())
    e = _rel(got, ref)
    _report(f"{tag} {count, dtype}", e)
    assert e < (1e-6 if dtype == F32T else 4e-3)
    if count >= len(_GELU_FIXED):
        assert torch.equal(_bits(out[7:8]), _bits(dy[7:8].to(dtype))) and got[8] == 0.0


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("count", [0, 3, 4, 1023, 1025])
def test_gelu_bwd_against_fp64(count, dtype):
    """tm_gelu_bwd (fp32 dy and pre, dpre in fp32 / bf16) around its 4-element pieces and its
    1024-element blocks; pre = 2 randn plus 0, +-1e-4, +-6, +-12, +-40.
    Measured on the MI355X (max over the counts): 9.9e-8 (fp32), 2.8e-3 (bf16)."""
    L = _lib()
    _p, _stream = _eng()
    pre, dy = _gelu_operands(count, _gen(count))
    pred = torch.zeros(count + TAIL, device=DEV)
    dyd = torch.zeros(count + TAIL, device=DEV)
    pred[:count] = pre
    dyd[:count] = dy
    dpre = torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_gelu_bwd", _tt(dtype), _p(dyd), _p(pred), count, _p(dpre), _stream())
    torch.cuda.synchronize()
    _gelu_check("gelu_bwd", dpre, pre, dy, count, dtype)


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("count", [8, 2048, 2056])
def test_gelu_bwd_pre_against_fp64(count, dtype):
    """tm_gelu_bwd_pre (pre and dpre both in T, 8 elements per thread, 2048 per block): the inputs and
    bounds of test_gelu_bwd_against_fp64, the reference taken on the T-rounded pre.
    Measured on the MI355X (max over the counts): 8.2e-8 (fp32), 2.5e-3 (bf16)."""
    L = _lib()
    _p, _stream = _eng()
    pre, dy = _gelu_operands(count, _gen(count))
    pre_t = pre.to(dtype)
    pred = torch.zeros(count + TAIL, dtype=dtype, device=DEV)
    dyd = torch.zeros(count + TAIL, device=DEV)
    pred[:count] = pre_t
    dyd[:count] = dy
    dpre = torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_gelu_bwd_pre", _tt(dtype), _p(dyd), _p(pred), count, _p(dpre), _stream())
    torch.cuda.synchronize()
    _gelu_check("gelu_bwd_pre", dpre, pre_t, dy, count, dtype)


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, 2047, 2049])
def test_add_relu_is_the_rounded_fp32_sum(count, dtype, alias):
    """tm_add_relu around its 8-element pieces and 2048-element blocks, y separate from a and y
    aliasing a: bit-equal to torch.relu(a.float() + b.float()).to(T); the sentinel survives past
    `count`."""
    L = _lib()
    _p, _stream = _eng()
    g = _gen(count + 17)
    a = torch.randn(count, generator=g).to(dtype)
    b = torch.randn(count, generator=g).to(dtype)
    want = torch.relu(a.float() + b.float()).to(dtype)
    ad = torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    bd = torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    ad[:count] = a
    bd[:count] = b
    y = ad if alias else torch.full((count + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    L.call("tm_add_relu", _tt(dtype), _p(ad), _p(bd), _p(y), count, _stream())
    torch.cuda.synchronize()
    out = y.cpu()
    assert (out[count:].float() == SENTINEL).all()
    assert torch.equal(_bits(out[:count]), _bits(want))
    if not alias:
        assert torch.equal(_bits(ad.cpu()[:count]), _bits(a))


@pytest.mark.parametrize("D", [64, 384, 1000])
def test_put_cls_writes_the_class_rows_only(D):
    """tm_put_cls, B = 3, S = 4 (D = 1000 is no multiple of the 256-thread stride): rows b * S of H
    equal cls, every other row keeps the sentinel."""
    L = _lib()
    _p, _stream = _eng()
    B, S = 3, 4
    cls = torch.randn(D, generator=_gen(D))
    clsd = cls.to(DEV)
    H = torch.full((B * S + 1, D), SENTINEL, device=DEV)
    L.call("tm_put_cls", _p(clsd), B, S, D, _p(H), _stream())
    torch.cuda.synchronize()
    out = H.cpu()
    assert (out[-1] == SENTINEL).all()
    out = out[:-1].view(B, S, D)
    assert torch.equal(_bits(out[:, 0]), _bits(cls.expand(B, D))) and (out[:, 1:] == SENTINEL).all()
