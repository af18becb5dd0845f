"""The ``backbone: resnet18`` image path without a GPU: the encoder's torchvision layout and frozen
body, the BN folding against the fp64 restatement (tests/resnet18_ref.py), tm_conv3x3's argument
checks and the config / optimizer plumbing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet18_ref import deterministic_resnet18_params_, resnet18_fp64, state_dict_layout, tiles
from test_config import YAML


def test_state_dict_is_torchvisions_resnet18():
    from transmil_deepgraft_amd.encoder import resnet18
    m = resnet18()
    sd = m.state_dict()
    layout = state_dict_layout()
    assert len(layout) == 122
    assert list(sd.keys()) == [k for k, _ in layout]
    assert [tuple(v.shape) for v in sd.values()] == [s for _, s in layout]
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)
    assert tuple(sd["layer2.0.downsample.0.weight"].shape) == (128, 64, 1, 1)
    assert tuple(sd["fc.weight"].shape) == (512, 512)
    body = sum(p.numel() for n, p in m.named_parameters() if not n.startswith("fc."))
    assert body == 11_176_512
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["fc.bias", "fc.weight"]


def test_imagenet_checkpoint_loads_without_its_head(tmp_path):
    from transmil_deepgraft_amd.encoder import resnet18
    src = deterministic_resnet18_params_(resnet18(), 5)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)     # the ImageNet head
    torch.save(sd, tmp_path / "r18.pth")
    m = resnet18()
    fc = m.fc.weight.clone()
    res = m.load_imagenet_checkpoint(tmp_path / "r18.pth")
    assert sorted(res.missing_keys) == ["fc.bias", "fc.weight"] and not res.unexpected_keys
    assert torch.equal(m.layer3[1].conv2.weight, src.layer3[1].conv2.weight) and torch.equal(m.fc.weight, fc)


def test_folding_math_on_host():
    """The eval-mode BN folding reproduces the fp64 restatement (run here on CPU tensors as a logic
    check -- the product forward refuses CPU tensors)."""
    from transmil_deepgraft_amd.encoder import resnet18
    m = deterministic_resnet18_params_(resnet18(), 2021).set_compute_dtype(torch.float32).eval()
    x = tiles(2, 64, 64)
    body, out, _ = resnet18_fp64(m.state_dict(), x)
    with torch.no_grad():
        m._fold_all()
        folded = m._forward_folded(x)
        plain = m._forward_modules(x)
        np.testing.assert_allclose(folded.numpy(), body.numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(plain.numpy(), body.numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(F.linear(folded, m.fc.weight, m.fc.bias).numpy(), out.numpy(), rtol=1e-4, atol=1e-5)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x)


@pytest.mark.parametrize("name,args", [
    ("cin = 96", dict(cin=96)), ("cout = 576", dict(cout=576)), ("stride = 3", dict(stride=3)),
    ("h = 0", dict(h=0)), ("NULL x", dict())])
def test_conv3x3_refuses_before_any_device_work(name, args):
    """Null pointers and no GPU: every refusal is status 1 with a ``conv3x3:`` message."""
    from transmil_deepgraft_amd import _lib
    a = dict(h=8, wd=8, cin=64, cout=64, stride=1)
    a.update(args)
    rc = _lib.lib().tm_conv3x3(_lib.BF16, None, None, None, None, None, 1, a["h"], a["wd"], a["cin"], a["cout"],
                               a["stride"], 0, None)
    assert rc == 1 and _lib.last_error().startswith("conv3x3:"), (name, rc, _lib.last_error())
    with pytest.raises(RuntimeError, match="conv3x3:"):
        _lib.call("tm_conv3x3", _lib.BF16, None, None, None, None, None, 1, a["h"], a["wd"], a["cin"], a["cout"],
                  a["stride"], 0, None)


def test_conv3x3_refuses_misaligned_pointers():
    import ctypes as C
    from transmil_deepgraft_amd import _lib
    buf = C.create_string_buffer(256)
    base = (C.addressof(buf) + 15) & ~15
    rc = _lib.lib().tm_conv3x3(_lib.F32, C.c_void_p(base + 4), C.c_void_p(base), None, None, C.c_void_p(base + 64),
                               1, 1, 1, 64, 64, 1, 0, None)
    assert rc == 1 and _lib.last_error().startswith("conv3x3:") and "aligned" in _lib.last_error()


def _cfg(tmp_path, in_features=None):
    from transmil_deepgraft_amd import config
    text = YAML.replace("    feature_extractor: retccl\n", "")
    text = text.replace("    backbone: features\n", "    backbone: resnet18\n")
    text = text.replace("    in_features: 1024\n", f"    in_features: {in_features}\n" if in_features else "")
    assert "resnet18" in text and "feature_extractor" not in text and ("in_features" in text) == bool(in_features)
    p = tmp_path / "TransMIL_resnet18.yaml"
    p.write_text(text)
    return config.read_yaml(p)


def test_config_builds_the_resnet18_image_model(tmp_path):
    from transmil_deepgraft_amd import config
    from transmil_deepgraft_amd.encoder import ImageBagModel, ResNet18
    model = config.build_model(_cfg(tmp_path), device="cpu")
    assert isinstance(model, ImageBagModel) and isinstance(model.model_ft, ResNet18)
    fc = model.model_ft.fc
    assert isinstance(fc, torch.nn.Linear) and (fc.in_features, fc.out_features) == (512, 512)
    assert model.model.in_features == 512 and model.n_classes == 3
    assert model.model_ft.compute_dtype == torch.bfloat16
    assert config.build_model(_cfg(tmp_path, 512), device="cpu").model.in_features == 512
    with pytest.raises(ValueError, match="512"):
        config.build_model(_cfg(tmp_path, 1024), device="cpu")


def test_optimizer_sees_the_mil_model_only(tmp_path):
    from transmil_deepgraft_amd import config
    cfg = _cfg(tmp_path)
    model = config.build_model(cfg, device="cpu")
    (opt,), _ = config.build_task(cfg, model).configure_optimizers()
    got = {id(p) for g in opt.param_groups for p in g["params"]}
    assert got == {id(p) for p in model.model.parameters()}
    assert not got & {id(p) for p in model.model_ft.parameters()}
