"""The ``simple`` tile backbone on the MI355X: the fused 5x5 convolution + ReLU + 2x2 max-pool kernel
(csrc/conv5x5.hip, tm_conv5x5_relu_pool) in both stages and compute modes -- exact placement (one-hot
weights, integer operands), fp64 references with derived bounds, bitwise reproducibility, 64-bit
addressing --, the 140450 -> width Linear + ReLU on tm_gemm over the rows the second stage writes,
and encoder.SimpleCNN against the fp64 restatement (tests/simple_cnn_ref.py), through ImageBagModel
and TransMILTask.

Kernel shapes: the smallest legal input (6 x 6: one pooled pixel), odd convolution outputs whose last
row / column the floor-mode pool drops (7 x 9, 13 x 22, 40 x 37), extents on both sides of the 8 x 16
(f32 second stage: 4 x 16) pooled-pixel patch of a workgroup (13 x 22: one patch, partly filled;
40 x 37: 18 x 16 pooled pixels = 3 (5) x 1 patches, the last rows partly filled; 110 x 110: 7 (14) x 4
with a 5-column last patch; 224 x 224: 14 x 7) and the model's own 224 x 224 / 110 x 110, each with one
and three tiles."""
import functools

import pytest
import torch
import torch.nn.functional as F

from simple_cnn_ref import deterministic_simple_params_, forward_fp64, stage, tiles

pytestmark = pytest.mark.gpu

STAGES = {1: (3, 20), 2: (20, 50)}
HW = [(6, 6), (7, 9), (13, 22), (40, 37), (110, 110)]
GRID = [(1, n, hw, lay) for n in (1, 3) for hw in HW for lay in ("nchw", "cl")] + \
       [(1, 1, (224, 224), lay) for lay in ("nchw", "cl")] + [(2, n, hw, "cl24") for n in (1, 3) for hw in HW]
IDS = [f"stage{s}_n{n}_{hw[0]}x{hw[1]}_{lay}" for s, n, hw, lay in GRID]
MODES = [torch.float32, torch.bfloat16]
TAIL = 6


def _seed(*key):
    return hash(key) % (2 ** 31)


def _run(x, w, b, st, layout):
    """x [n, cin, h, w], w [cout, cin, 5, 5] CPU tensors of one dtype, b fp32 [cout] -> the kernel's
    pooled output [n, cout, ph, pw] on the CPU.  The output buffer starts as NaN: the pad channels
    (first stage: 20 .. 23) and the tail after each tile must come back as zeros."""
    from transmil_deepgraft_amd.encoder import conv5x5_relu_pool, pack_conv5x5
    cin, cout = STAGES[st]
    n, _, h, wd = x.shape
    ph, pw = (h - 4) // 2, (wd - 4) // 2
    cpo = 24 if st == 1 else 50
    so = ph * pw * cpo + TAIL
    xg = x.cuda()
    if layout == "cl":
        xg = xg.contiguous(memory_format=torch.channels_last)
        assert xg.stride(1) == 1 or cin == 1
    elif layout == "cl24":
        xg = torch.zeros(n, h, wd, 24, dtype=x.dtype, device="cuda")
        xg[..., :20] = x.cuda().permute(0, 2, 3, 1)
    out = torch.full((n, so), float("nan"), dtype=x.dtype, device="cuda")
    conv5x5_relu_pool(xg, pack_conv5x5(w.cuda(), x.dtype), b.float().cuda(), cout, out, so, cpo, TAIL)
    torch.cuda.synchronize()
    out = out.cpu()
    pix = out[:, :ph * pw * cpo].view(n, ph, pw, cpo)
    assert not bool(out[:, ph * pw * cpo:].float().abs().sum() != 0), "tail not zero"
    assert not bool(pix[..., cout:].float().abs().sum() != 0), "pad channels not zero"
    return pix[..., :cout].permute(0, 3, 1, 2).contiguous()


# ----------------------------------------------------------------------------- exact placement
def _one_hot(cin, cout):
    """w[co, ci = (7 co + 3) mod cin, tap = co mod 25] = 1: an asymmetric map, so a swapped tap,
    row / column or channel index cannot pass."""
    w = torch.zeros(cout, cin, 5, 5)
    co = torch.arange(cout)
    tap = co % 25
    w[co, (7 * co + 3) % cin, tap // 5, tap % 5] = 1.0
    return w


def _gather_pool(x, cin, cout):
    """The shifted gather, ReLU and floor-mode pool the one-hot convolution must equal."""
    n, _, h, wd = x.shape
    ho, wo = h - 4, wd - 4
    conv = torch.empty(n, cout, ho, wo, dtype=x.dtype)
    for co in range(cout):
        ky, kx = (co % 25) // 5, (co % 25) % 5
        conv[:, co] = x[:, (7 * co + 3) % cin, ky:ky + ho, kx:kx + wo]
    return F.max_pool2d(conv.relu(), 2, 2)


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("st,n,hw,layout", GRID, ids=IDS)
def test_one_hot_placement_is_bitwise(st, n, hw, layout, dtype):
    cin, cout = STAGES[st]
    g = torch.Generator().manual_seed(_seed(st, n, hw))
    x = torch.randn(n, cin, *hw, generator=g).bfloat16().float()      # bf16-representable
    got = _run(x.to(dtype), _one_hot(cin, cout).to(dtype), torch.zeros(cout), st, layout)
    assert torch.equal(got.float(), _gather_pool(x, cin, cout))


@pytest.mark.parametrize("st,n,hw,layout", GRID, ids=IDS)
def test_f32_small_integers_are_bitwise(st, n, hw, layout):
    """x in [-3, 3], dense w in [-2, 2], integer bias: every partial sum is an integer below 2^24 (at
    most 3 * 2 * 500 + 4), so any summation order gives the integer result exactly."""
    cin, cout = STAGES[st]
    g = torch.Generator().manual_seed(_seed(st, n, hw) + 1)
    x = torch.randint(-3, 4, (n, cin, *hw), generator=g).float()
    w = torch.randint(-2, 3, (cout, cin, 5, 5), generator=g).float()
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    got = _run(x, w, b, st, layout)
    assert torch.equal(got.double(), stage(x.double(), w.double(), b.double()))


# ----------------------------------------------------------------------------- random operands
@functools.lru_cache(maxsize=4)
def _operands(st, n, hw):
    """fp32 random operands of one grid point (shared by the modes and layouts)."""
    cin, cout = STAGES[st]
    g = torch.Generator().manual_seed(_seed(st, n, hw) + 2)
    x = torch.randn(n, cin, *hw, generator=g)
    w = torch.randn(cout, cin, 5, 5, generator=g) * (25 * cin) ** -0.5
    b = torch.randn(cout, generator=g)
    return x, w, b


@pytest.mark.parametrize("st,n,hw,layout", GRID, ids=IDS)
def test_f32_random_against_fp64(st, n, hw, layout):
    """TM_F32: the error against the fp64 stage of the same fp32 operands, relative to the largest
    output, within 4 x the same error of torch's CPU fp32 conv2d -> relu -> max_pool2d (the rule
    for kernels without a prior bound)."""
    x, w, b = _operands(st, n, hw)
    ref = stage(x.double(), w.double(), b.double())
    cpu = stage(x, w, b)
    got = _run(x, w, b, st, layout)
    scale = ref.abs().max()
    bound = 4 * (cpu.double() - ref).abs().max() / scale
    err = (got.double() - ref).abs().max() / scale
    print(f"conv5x5 f32 stage{st} n{n} {hw} {layout}: err {err:.3e} bound {bound:.3e} ratio {float(err / bound):.3f}")
    assert err <= bound, (float(err), float(bound))


@pytest.mark.parametrize("st,n,hw,layout", GRID, ids=IDS)
def test_bf16_random_against_fp64(st, n, hw, layout):
    """TM_BF16 against the fp64 stage of the bf16-rounded x and w (the bias is an fp32 operand),
    elementwise.  Per convolution pixel b = 2^-8 |ref| + (25 cin + 2) 2^-24 A, A = conv(|x|, |w|) +
    |bias| (one bf16 output rounding with a 2 x margin + fp32 accumulation in any order); a pooled
    output's bound is the max of b over its window, since |max a_i - max r_i| <= max |a_i - r_i|."""
    cin, cout = STAGES[st]
    x, w, b = _operands(st, n, hw)
    x, w = x.bfloat16(), w.bfloat16()
    xd, wd_, bd = x.double(), w.double(), b.double()
    conv = F.conv2d(xd, wd_, bd).relu()
    A = F.conv2d(xd.abs(), wd_.abs(), bd.abs())
    bound = F.max_pool2d(2.0 ** -8 * conv + (25 * cin + 2) * 2.0 ** -24 * A, 2, 2)
    ref = F.max_pool2d(conv, 2, 2)
    got = _run(x, w, b, st, layout)
    err = (got.double() - ref).abs()
    print(f"conv5x5 bf16 stage{st} n{n} {hw} {layout}: worst err/bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16"])
@pytest.mark.parametrize("st", [1, 2])
def test_two_launches_are_bitwise_equal(st, dtype):
    x, w, b = _operands(st, 3, (40, 37))
    lay = "nchw" if st == 1 else "cl24"
    a = _run(x.to(dtype), w.to(dtype), b, st, lay)
    c = _run(x.to(dtype), w.to(dtype), b, st, lay)
    assert torch.equal(a, c)


# ----------------------------------------------------------------------------- large offsets
@pytest.mark.parametrize("st", [1, 2])
def test_tiles_and_outputs_more_than_2_31_bytes_apart(st):
    """x and out are views into one buffer of 2 GiB + 16 MiB: two tiles whose inputs lie 2^31 + 256
    bytes apart (the tile stride sn), their outputs the same distance apart (so), the second output
    more than 2^31 bytes past the first input.  Both tiles equal the densely packed run."""
    from transmil_deepgraft_amd.encoder import conv5x5_relu_pool, pack_conv5x5
    cin, cout = STAGES[st]
    h, wd = 40, 37
    ph, pw = (h - 4) // 2, (wd - 4) // 2
    cpo = 24 if st == 1 else 50
    x, w, b = _operands(st, 3, (h, wd))
    x = x[:2]
    want = _run(x, w, b, st, "nchw" if st == 1 else "cl24")
    raw = torch.empty(2 ** 31 + 2 ** 24, dtype=torch.uint8, device="cuda")
    slab = raw.view(torch.float32)
    step = 2 ** 29 + 64                                              # elements between the two tiles
    if st == 1:
        xin = torch.as_strided(slab, (2, 3, h, wd), (step, h * wd, wd, 1))
        xin.copy_(x.cuda())
    else:
        xin = torch.as_strided(slab, (2, h, wd, 24), (step, wd * 24, 24, 1))
        xin.zero_()
        xin[..., :20] = x.cuda().permute(0, 2, 3, 1)
    out = torch.as_strided(slab, (2, ph * pw * cpo + TAIL), (step, 1), 2 ** 20)
    out.fill_(float("nan"))
    assert out[1].data_ptr() - xin[0].data_ptr() > 2 ** 31 and xin[1].data_ptr() - xin[0].data_ptr() > 2 ** 31
    conv5x5_relu_pool(xin, pack_conv5x5(w.cuda(), torch.float32), b.cuda(), cout, out, step, cpo, TAIL)
    torch.cuda.synchronize()
    got = out.cpu()
    assert not bool(got[:, ph * pw * cpo:].any())
    assert torch.equal(got[:, :ph * pw * cpo].view(2, ph, pw, cpo)[..., :cout].permute(0, 3, 1, 2), want)


# ----------------------------------------------------------------------------- the Linear
FC_WIDTH = 64


@functools.lru_cache(maxsize=None)
def _fc_operands():
    """130 second-stage inputs [130, 20, 110, 110] (bf16-representable) whose one-hot convolution gives
    the feature rows exactly, and a Linear(140450, 64) in the reference's (c, y, x) column order."""
    g = torch.Generator().manual_seed(31)
    x2 = torch.randn(130, 20, 110, 110, generator=g).bfloat16().float()
    feats = _gather_pool(x2, 20, 50).flatten(1)                      # NCHW flatten: c * 2809 + y * 53 + x
    W = (torch.randn(FC_WIDTH, 140450, generator=g) * 140450 ** -0.5)
    bias = torch.randn(FC_WIDTH, generator=g)
    return x2, feats, W, bias


@functools.lru_cache(maxsize=None)
def _fc_reference(bf16):
    x2, feats, W, bias = _fc_operands()
    Wd = (W.bfloat16() if bf16 else W).double()
    fd = feats.double()
    ref = (fd @ Wd.T + bias.double()).relu()
    A = fd.abs() @ Wd.abs().T + bias.double().abs()
    cpu = (feats @ W.T + bias).relu() if not bf16 else None
    return ref, A, cpu


def _fc_run(m, dtype):
    """Rows through the kernels: NaN-filled [m, 140480] rows, written by the second stage (one-hot
    weights: the rows are exactly the pooled gather, the 30-element tail zeros), then the GEMM."""
    from transmil_deepgraft_amd.encoder import (SIMPLE_K, SIMPLE_KP, conv5x5_relu_pool, pack_conv5x5, pack_simple_fc,
                                                simple_fc)
    x2, feats, W, bias = _fc_operands()
    xg = torch.zeros(m, 110, 110, 24, dtype=dtype, device="cuda")
    xg[..., :20] = x2[:m].cuda().permute(0, 2, 3, 1)
    a = torch.full((m, SIMPLE_KP), float("nan"), dtype=dtype, device="cuda")
    conv5x5_relu_pool(xg, pack_conv5x5(_one_hot(20, 50).cuda(), dtype), torch.zeros(50, device="cuda"), 50, a,
                      SIMPLE_KP, 50, SIMPLE_KP - SIMPLE_K)
    rows = a[:, :SIMPLE_K].view(m, 53, 53, 50).permute(0, 3, 1, 2).flatten(1).float().cpu()
    assert torch.equal(rows, feats[:m]) and not bool(a[:, SIMPLE_K:].float().abs().sum() != 0)
    out = torch.empty(m, FC_WIDTH, dtype=torch.float32, device="cuda")
    simple_fc(a, pack_simple_fc(W.cuda(), dtype), bias.cuda(), out)
    torch.cuda.synchronize()
    return out.cpu().double()


@pytest.mark.parametrize("m", [1, 3, 130])
def test_fc_f32_against_fp64(m):
    """relu(x W^T + b) over the unpadded operands in fp64; the error relative to the largest output
    within 4 x the same error of torch's CPU fp32 product."""
    ref, _, cpu = _fc_reference(False)
    ref, cpu = ref[:m], cpu[:m]
    got = _fc_run(m, torch.float32)
    scale = ref.abs().max()
    bound = 4 * (cpu.double() - ref).abs().max() / scale
    err = (got - ref).abs().max() / scale
    print(f"simple fc f32 m{m}: err {err:.3e} bound {bound:.3e} ratio {float(err / bound):.3f}")
    assert err <= bound, (float(err), float(bound))


@pytest.mark.parametrize("m", [1, 3, 130])
def test_fc_bf16_against_fp64(m):
    """bf16 operands, fp32 accumulation, fp32 output: |err| <= 2^-8 |ref| + (140450 + 2) 2^-24
    (|x| |W|^T + |b|) elementwise, against fp64 of the bf16-rounded weights (the rows are bf16 already)."""
    ref, A, _ = _fc_reference(True)
    ref, A = ref[:m], A[:m]
    got = _fc_run(m, torch.bfloat16)
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (140450 + 2) * 2.0 ** -24 * A
    print(f"simple fc bf16 m{m}: worst err/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err - bound).max())


# ----------------------------------------------------------------------------- the model
def _encoder(width=64, dtype=torch.float32, seed=2021):
    from transmil_deepgraft_amd.encoder import simple_cnn
    return deterministic_simple_params_(simple_cnn(width=width), seed).set_compute_dtype(dtype).eval()


@functools.lru_cache(maxsize=None)
def _model_reference(n):
    x = tiles(n, seed=n)
    return x, forward_fp64(_encoder().state_dict(), x)


def _rel_l2(got, ref):
    return ((got.double().cpu() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2e-3), (torch.bfloat16, 6e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [2, 5])
def test_model_matches_fp64(n, dtype, rtol):
    """Per-tile relative L2 error of the [n, 64] output against the fp64 restatement; five tiles with
    chunk 2 run three chunks, the last a single tile."""
    x, ref = _model_reference(n)
    m = _encoder(dtype=dtype).cuda()
    m.chunk = 2
    got = m(x.cuda())
    assert got.shape == (n, 64) and got.dtype == torch.float32 and not got.requires_grad
    err = _rel_l2(got, ref)
    print(f"simple cnn n{n} {dtype}: rel L2 {err:.3e} (bound {rtol})")
    assert err < rtol, err


@functools.lru_cache(maxsize=None)
def _full_width_encoder():
    """The 1024-wide encoder with torch's own initialisation (one build shared by the tests below)."""
    from transmil_deepgraft_amd.encoder import simple_cnn
    torch.manual_seed(7)
    return simple_cnn().eval()


def test_full_width_bf16_matches_fp64():
    enc = _full_width_encoder()
    x = tiles(2, seed=9)
    ref = forward_fp64(enc.state_dict(), x)
    got = enc.cuda()(x.cuda())
    assert got.shape == (2, 1024)
    err = _rel_l2(got, ref)
    print(f"simple cnn width 1024 bf16: rel L2 {err:.3e} (bound 6e-2)")
    assert err < 6e-2, err


def test_train_and_eval_mode_are_bitwise_equal():
    x = tiles(2, seed=2).cuda()
    m = _encoder(dtype=torch.bfloat16).cuda()
    a = m.eval()(x)
    b = m.train()(x)
    assert torch.equal(a, b) and not b.requires_grad


def test_refolds_after_an_in_place_weight_edit():
    """The _fold_key contract: an in-place edit of 7.weight changes the next forward, which then
    equals a freshly built encoder with the same edit."""
    x = tiles(2, seed=4).cuda()
    m = _encoder().cuda()
    before = m(x)
    with torch.no_grad():
        m.state_dict()["7.weight"].mul_(0.5)
        after = m(x)
        fresh = _encoder()
        fresh.state_dict()["7.weight"].mul_(0.5)
        want = fresh.cuda()(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_image_path_gradients_and_task_steps():
    """[1, 4, 3, 224, 224] -> SimpleCNN -> AttMIL(2, 1024): the logits equal encoder-then-model run
    separately; backward gives every AttMIL parameter the forward uses a finite gradient and no CNN parameter any;
    TransMILTask trains one step (only MIL parameters move) and records one validation step."""
    from transmil_deepgraft_amd.encoder import ImageBagModel
    from transmil_deepgraft_amd.interface import TransMILTask
    from transmil_deepgraft_amd.models import AttMIL
    torch.manual_seed(0)
    enc = _full_width_encoder().cuda()
    mil = AttMIL(2, 1024).cuda().eval()
    model = ImageBagModel(enc, mil).eval()
    x = tiles(4, seed=5).cuda().view(1, 4, 3, 224, 224)
    logits = model(x)
    with torch.no_grad():
        apart = mil(enc(x[0]).view(1, 4, 1024))
    torch.testing.assert_close(logits.detach(), apart, rtol=0, atol=1e-5)
    logits.sum().backward()
    for name, p in mil.named_parameters():
        if name.startswith("feature_extractor_part2."):          # constructed but unused, as in the reference
            assert p.grad is None, name
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for name, p in enc.named_parameters():
        assert p.grad is None, name
    mil.zero_grad(set_to_none=True)

    task = TransMILTask(model, lr=2e-4)
    (opt,), _ = task.configure_optimizers()
    label = torch.tensor([1], device="cuda")
    cnn0 = [p.detach().clone() for p in (enc.state_dict()[k] for k in ("0.weight", "3.bias", "7.bias"))]
    mil0 = [p.detach().clone() for p in mil.parameters()]
    model.train()
    loss = task.optimization_step((x, label, None), opt)
    assert torch.isfinite(loss).all()
    assert any(not torch.equal(p, q) for p, q in zip(mil.parameters(), mil0))
    assert all(torch.equal(enc.state_dict()[k], q) for k, q in zip(("0.weight", "3.bias", "7.bias"), cnn0))
    assert all(p.grad is None for p in enc.parameters())
    model.eval()
    out = task.validation_step((x, label, (["slide0"], None, ["patient0"])))
    assert out.shape == (1, 2) and torch.isfinite(out).all()
    assert task.eval_state("val").record.n == 1


def test_simple_yaml_builds_and_runs_on_tile_batches(tmp_path):
    """A ``backbone: simple`` YAML builds on the GPU and evaluates a [1, 3, 3, 224, 224] batch."""
    from test_simple_cnn_cpu import _cfg
    from transmil_deepgraft_amd import config
    cfg = _cfg(tmp_path)
    cfg.General.grad_acc = 1
    torch.manual_seed(0)
    model = config.build_model(cfg, device="cuda")
    task = config.build_task(cfg, model)
    (opt,), _ = task.configure_optimizers()
    x = tiles(3, seed=8).cuda().view(1, 3, 3, 224, 224)
    label = torch.tensor([2], device="cuda")
    model.train()
    assert torch.isfinite(task.optimization_step((x, label, None), opt)).all()
    model.eval()
    logits = task.validation_step((x, label, (["slide0"], None, ["patient0"])))
    assert logits.shape == (1, 3) and torch.isfinite(logits).all()
