"""The ResNet-18 tile encoder (encoder.ResNet18: stem kernels, tm_conv3x3 BasicBlocks, 1x1 GEMM
downsamples, HIP fc) on the MI355X against the fp64 restatement (tests/resnet18_ref.py), in eval
(BN folded) and train (whole-bag batch statistics) mode, through ImageBagModel and TransMILTask."""
import functools

import pytest
import torch

from resnet18_ref import deterministic_resnet18_params_, resnet18_fp64, tiles

pytestmark = pytest.mark.gpu


def _encoder(dtype=torch.float32, seed=2021):
    from transmil_deepgraft_amd.encoder import resnet18
    return deterministic_resnet18_params_(resnet18(), seed).set_compute_dtype(dtype).eval()


@functools.lru_cache(maxsize=None)
def _eval_reference(h, w, n):
    x = tiles(n, h, w, seed=h + w)
    return x, resnet18_fp64(_encoder().state_dict(), x)[1]


@functools.lru_cache(maxsize=None)
def _train_reference():
    x = tiles(6, seed=3)
    _, out, stats = resnet18_fp64(_encoder().state_dict(), x, train=True)
    return x, out, stats


def _rel_l2(got, ref):
    return ((got.double().cpu() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2e-3), (torch.bfloat16, 6e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("h,w,n", [(224, 224, 4), (72, 88, 3)], ids=["224x224", "72x88"])
def test_eval_matches_fp64(h, w, n, dtype, rtol):
    """Per-tile relative L2 error of the [n, 512] output; 72 x 88 tiles run layer4 on a 3 x 3 grid."""
    x, ref = _eval_reference(h, w, n)
    torch.backends.cudnn.allow_tf32 = False
    m = _encoder(dtype).cuda()
    with torch.no_grad():
        got = m(x.cuda())
    assert got.shape == (n, 512) and got.dtype == torch.float32
    err = _rel_l2(got, ref)
    print(f"resnet18 eval {h}x{w} {dtype}: rel L2 {err:.3e} (bound {rtol})")
    assert err < rtol, err


@pytest.mark.parametrize("dtype,rtol,stol", [(torch.float32, 2e-3, 1e-3), (torch.bfloat16, 6e-2, 3e-2)],
                         ids=["f32", "bf16"])
def test_train_mode_uses_whole_bag_statistics(dtype, rtol, stol):
    """6 tiles, chunk 4: the bag spans two pieces while every BatchNorm's statistics span all six;
    features, updated running statistics and num_batches_tracked equal the fp64 train-mode BN."""
    x, ref, stats = _train_reference()
    torch.backends.cudnn.allow_tf32 = False
    enc = _encoder(dtype)
    enc.chunk = 4
    enc = enc.cuda().train()
    with torch.no_grad():
        got = enc(x.cuda())
    err = _rel_l2(got, ref)
    sd = enc.state_dict()
    worst = max(((sd[k].double().cpu() - v).abs().max() / v.abs().max().clamp_min(1e-6)).item()
                for k, v in stats.items())
    print(f"resnet18 train {dtype}: rel L2 {err:.3e} (bound {rtol}), running stats {worst:.3e} (bound {stol})")
    assert len(stats) == 40                       # 20 BatchNorms: running_mean and running_var
    assert err < rtol, err
    assert worst < stol, worst
    tracked = [v.item() for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert len(tracked) == 20 and all(t == 1 for t in tracked), tracked


def test_image_path_and_gradients():
    """[1, 6, 3, 224, 224] -> encoder -> TransMIL(2, 512): logits equal encoder-then-model run
    separately; backward reaches every MIL parameter and model_ft.fc, no other encoder parameter."""
    from transmil_deepgraft_amd.encoder import ImageBagModel
    from transmil_deepgraft_amd.models import TransMIL
    torch.manual_seed(0)
    enc = _encoder().cuda()
    mil = TransMIL(2, 512).cuda().eval().set_compute_dtype(torch.float32)
    model = ImageBagModel(enc, mil).eval()
    x = tiles(6, seed=5).cuda().view(1, 6, 3, 224, 224)
    logits = model(x)
    with torch.no_grad():
        apart = mil(enc(x[0]).view(1, 6, 512))
    torch.testing.assert_close(logits.detach(), apart, rtol=0, atol=1e-5)
    logits.sum().backward()
    for name, p in mil.named_parameters():
        assert p.grad is not None, name
    for name, p in enc.named_parameters():
        assert (p.grad is not None) == name.startswith("fc."), name
    assert float(enc.fc.weight.grad.abs().max()) > 0


def test_refolds_after_an_in_place_statistics_edit():
    """The _fold_key contract: an in-place edit of a running statistic changes the next eval
    forward, which then equals a freshly built encoder with the same edit."""
    x = tiles(2, 72, 88, seed=11).cuda()
    m = _encoder().cuda()
    with torch.no_grad():
        before = m(x)
        m.layer1[0].bn1.running_mean.add_(0.25)
        after = m(x)
        fresh = _encoder()
        fresh.layer1[0].bn1.running_mean.add_(0.25)
        want = fresh.cuda()(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_task_runs_a_training_and_an_evaluation_step_on_tile_batches(tmp_path):
    """A ``backbone: resnet18`` YAML builds; TransMILTask trains one step on a [1, bag, 3, H, W]
    batch (only MIL parameters move: the optimizer holds no encoder parameter) and records one
    validation step."""
    from test_resnet18_cpu import _cfg
    from transmil_deepgraft_amd import config
    cfg = _cfg(tmp_path)
    cfg.General.grad_acc = 1
    torch.manual_seed(0)
    model = config.build_model(cfg, device="cuda")
    task = config.build_task(cfg, model)
    (opt,), _ = task.configure_optimizers()
    x = tiles(5, 72, 88, seed=2).cuda().view(1, 5, 3, 72, 88)
    label = torch.tensor([1], device="cuda")
    fc0 = model.model_ft.fc.weight.clone()
    mil0 = [p.detach().clone() for p in model.model.parameters()]
    model.train()
    loss = task.optimization_step((x, label, None), opt)
    assert torch.isfinite(loss).all()
    # model_ft.fc receives a gradient that nobody applies, as in the reference
    assert torch.equal(model.model_ft.fc.weight, fc0) and model.model_ft.fc.weight.grad is not None
    assert any(not torch.equal(p, q) for p, q in zip(model.model.parameters(), mil0))
    model.eval()
    logits = task.validation_step((x, label, (["slide0"], None, ["patient0"])))
    assert logits.shape == (1, 3) and torch.isfinite(logits).all()
    assert task.eval_state("val").record.n == 1
