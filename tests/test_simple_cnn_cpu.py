"""The ``backbone: simple`` image path without a GPU: the encoder's state_dict layout and frozen
parameters against the torch restatement (tests/simple_cnn_ref.py), its input checks, the Lightning
checkpoint loader, the weight packing, tm_conv5x5_relu_pool's argument checks and the config plumbing."""
import pytest
import torch

from simple_cnn_ref import deterministic_simple_params_, simple_cnn_ref
from test_config import YAML

WIDTH = 64       # a narrow Linear keeps the 140450-wide weight at 36 MB


def test_state_dict_is_the_reference_sequentials():
    from transmil_deepgraft_amd.encoder import SimpleCNN, simple_cnn
    m = simple_cnn(width=WIDTH)
    ref = simple_cnn_ref(WIDTH, torch.float32)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert isinstance(m, SimpleCNN) and m.width == WIDTH and SimpleCNN.__init__.__defaults__[0] == 1024
    assert list(sd.keys()) == list(rsd.keys()) == ["0.weight", "0.bias", "3.weight", "3.bias", "7.weight", "7.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    assert tuple(sd["0.weight"].shape) == (20, 3, 5, 5) and tuple(sd["3.weight"].shape) == (50, 20, 5, 5)
    assert tuple(sd["7.weight"].shape) == (WIDTH, 140450)
    ref.load_state_dict(sd)          # ... and loads into it


def test_all_parameters_are_frozen():
    from transmil_deepgraft_amd.encoder import simple_cnn
    m = simple_cnn(width=WIDTH)
    assert len(list(m.parameters())) == 6 and not any(p.requires_grad for p in m.parameters())
    # torch's own initialisation: kaiming_uniform(a = sqrt(5)) bounds weights by 1 / sqrt(fan_in)
    for name, fan_in in (("0", 75), ("3", 500), ("7", 140450)):
        w = m.state_dict()[name + ".weight"]
        assert 0.9 * fan_in ** -0.5 < float(w.abs().max()) <= fan_in ** -0.5, name


def test_cpu_tensor_and_other_tile_sizes_are_refused():
    from transmil_deepgraft_amd.encoder import simple_cnn
    m = simple_cnn(width=WIDTH)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match=r"\[n, 3, 224, 224\]"):
        m(torch.zeros(1, 3, 200, 200))
    with pytest.raises(ValueError, match="bfloat16 or torch.float32"):
        m.set_compute_dtype(torch.float16)
    assert m.set_compute_dtype(torch.float32) is m and m.compute_dtype == torch.float32


def test_load_lightning_state_dict_picks_the_model_ft_tensors():
    from transmil_deepgraft_amd.encoder import simple_cnn
    src = deterministic_simple_params_(simple_cnn(width=WIDTH), 5)
    ckpt = {"model_ft." + k: v.clone() for k, v in src.state_dict().items()}
    ckpt["model.attention.0.weight"] = torch.zeros(3, 3)           # the MIL model's tensors are not ours
    ckpt["model.classifier.0.bias"] = torch.zeros(2)
    m = simple_cnn(width=WIDTH)
    res = m.load_lightning_state_dict(ckpt)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_lightning_state_dict({"model_ft.0.weight": ckpt["model_ft.0.weight"]})


def test_packed_weights_name_every_tap_once():
    """pack_conv5x5: every weight appears exactly once in the fragment order, everything else is zero;
    pack_simple_fc maps the (c, y, x) flatten order to (y, x, c) and zero-pads K."""
    from transmil_deepgraft_amd.encoder import SIMPLE_K, SIMPLE_KP, pack_conv5x5, pack_simple_fc
    for cout, cin, ns, nu in ((20, 3, 8, 1), (50, 20, 38, 2)):
        w = torch.arange(1, cout * cin * 25 + 1, dtype=torch.float64).view(cout, cin, 5, 5)
        wp = pack_conv5x5(w, torch.float64)
        assert tuple(wp.shape) == (ns, nu, 2, 32, 8)
        assert sorted(wp[wp != 0].tolist()) == w.flatten().tolist()
        # [s][u][hf][r][j] -> row 32 u + r, fragment 2 s + hf
        rows = wp.permute(1, 3, 0, 2, 4).reshape(32 * nu, 2 * ns, 8)
        assert not bool(rows[cout:].any())
        if cin == 3:       # fragment 3 ky + sub, element 4 (kx - 2 sub) + c
            assert rows[7, 3 * 2 + 1, 4 * 1 + 2] == w[7, 2, 2, 3]
        else:              # fragment 3 (5 ky + kx) + sub, element c - 8 sub
            assert rows[41, 3 * (5 * 4 + 1) + 2, 3] == w[41, 19, 4, 1]
    fc = torch.arange(2 * SIMPLE_K, dtype=torch.float32).view(2, SIMPLE_K)
    fp = pack_simple_fc(fc, torch.float32)
    assert tuple(fp.shape) == (2, SIMPLE_KP) and SIMPLE_KP % 64 == 0 and not bool(fp[:, SIMPLE_K:].any())
    c, y, x = 17, 30, 52
    assert fp[1, (y * 53 + x) * 50 + c] == fc[1, c * 2809 + y * 53 + x]


def _cfg(tmp_path, in_features=1024):
    from transmil_deepgraft_amd import config
    text = YAML.replace("    feature_extractor: retccl\n", "")
    text = text.replace("    backbone: features\n", "    backbone: simple\n")
    text = text.replace("    name: TransMIL\n", "    name: AttMIL\n")
    text = text.replace("    in_features: 1024\n", f"    in_features: {in_features}\n" if in_features else "")
    assert "simple" in text and "AttMIL" in text and "feature_extractor" not in text
    assert ("in_features" in text) == bool(in_features)
    p = tmp_path / "AttMIL_simple.yaml"
    p.write_text(text)
    return config.read_yaml(p)


def test_config_builds_the_simple_image_model(tmp_path):
    from transmil_deepgraft_amd import config
    from transmil_deepgraft_amd.encoder import ImageBagModel, SimpleCNN
    from transmil_deepgraft_amd.models import AttMIL
    model = config.build_model(_cfg(tmp_path), device="cpu")
    assert isinstance(model, ImageBagModel) and isinstance(model.model_ft, SimpleCNN)
    assert isinstance(model.model, AttMIL) and model.model.n_classes == 3 and model.n_classes == 3
    assert model.model_ft.width == 1024 and model.model_ft.compute_dtype == torch.bfloat16
    assert sorted(k for k in model.state_dict() if k.startswith("model_ft.")) == sorted(
        "model_ft." + k for k in ("0.weight", "0.bias", "3.weight", "3.bias", "7.weight", "7.bias"))


def test_config_in_features_must_be_1024(tmp_path):
    from transmil_deepgraft_amd import config
    with pytest.raises(ValueError, match="1024"):
        config.in_features_of(_cfg(tmp_path, 512))
    with pytest.raises(ValueError, match="1024"):
        config.build_model(_cfg(tmp_path, 512), device="cpu")
    assert config.in_features_of(_cfg(tmp_path, None)) == 1024
    assert config.in_features_of(_cfg(tmp_path, 1024)) == 1024


def test_optimizer_sees_the_mil_model_only(tmp_path):
    from transmil_deepgraft_amd import config
    cfg = _cfg(tmp_path)
    model = config.build_model(cfg, device="cpu")
    (opt,), _ = config.build_task(cfg, model).configure_optimizers()
    got = {id(p) for g in opt.param_groups for p in g["params"]}
    assert got == {id(p) for p in model.model.parameters()}


@pytest.mark.parametrize("name,args", [
    ("(cin, cout) = (3, 50)", dict(cin=3, cout=50)), ("(cin, cout) = (20, 20)", dict(cin=20, cout=20)),
    ("h = 5", dict(h=5)), ("w = 5", dict(w=5)), ("n = 0", dict(n=0)), ("NULL pointers", dict())])
def test_conv5x5_refuses_before_any_device_work(name, args):
    """Null pointers and no GPU: every refusal is status 1 with a ``conv5x5:`` message."""
    from transmil_deepgraft_amd import _lib
    a = dict(n=1, h=8, w=8, cin=3, cout=20)
    a.update(args)
    call = ("tm_conv5x5_relu_pool", _lib.BF16, None, None, None, None, a["n"], a["h"], a["w"], a["cin"], a["cout"],
            3 * 64, 64, 8, 1, 2 * 2 * 24, 24, 0, None)
    rc = getattr(_lib.lib(), call[0])(*call[1:])
    assert rc == 1 and _lib.last_error().startswith("conv5x5:"), (name, rc, _lib.last_error())
    with pytest.raises(RuntimeError, match="conv5x5:"):
        _lib.call(*call)


def test_conv5x5_refuses_bad_output_layouts():
    import ctypes as C
    from transmil_deepgraft_amd import _lib
    buf = C.create_string_buffer(4096)
    base = (C.addressof(buf) + 15) & ~15
    x, wp, b, out = (C.c_void_p(base + 512 * i) for i in range(4))

    def rc(**kw):
        a = dict(cin=3, cout=20, sc=64, sh=8, sw=1, so=96, cpo=24, tail=0, out=out)
        a.update(kw)
        r = _lib.lib().tm_conv5x5_relu_pool(_lib.F32, x, wp, b, a["out"], 1, 8, 8, a["cin"], a["cout"], 192, a["sc"],
                                            a["sh"], a["sw"], a["so"], a["cpo"], a["tail"], None)
        return r, _lib.last_error()

    for kw in (dict(cpo=18), dict(cpo=21), dict(cpo=34), dict(so=94), dict(tail=1), dict(tail=-1), dict(so=97),
               dict(out=C.c_void_p(base + 4)), dict(cin=20, cout=50, cpo=50, so=200),      # first-stage strides
               dict(cin=20, cout=50, cpo=50, so=200, sc=1, sw=24, sh=100)):               # sh % 8 != 0
        r, msg = rc(**kw)
        assert r == 1 and msg.startswith("conv5x5:"), (kw, r, msg)


def test_library_exports_the_entry_point():
    from transmil_deepgraft_amd import _lib
    assert "tm_conv5x5_relu_pool" in _lib.EXPORTED and hasattr(_lib.lib(), "tm_conv5x5_relu_pool")
    assert len(_lib._SIGS["tm_conv5x5_relu_pool"][1]) == 18
