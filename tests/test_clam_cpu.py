"""CLAM_MB without a GPU: the restatement against the reference-run fixtures, the state dict, the
config, the constructor's refusals, the refusal of CPU tensors and the entry points' status path."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as G
from clam_ref import ClamMBRef, case_input, extreme_gap, fixture_cases, ref_model, select, targets_of
from transmil_deepgraft_amd import config
from transmil_deepgraft_amd.models import CLAM_MB

CASES = fixture_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_fixture(name):
    K, N, size, k, subtyping, label = CASES[name]
    fx = G.load(name)
    assert float(fx["gap"]) >= 256.0 * float(fx["err32"]) > 0.0
    x = torch.from_numpy(case_input(N, int(fx["seed"])))
    for dtype, suffix in ((torch.float32, ""), (torch.float64, ".f64")):
        with torch.no_grad():
            r = ref_model(name, CASES[name], dtype)(x.to(dtype), label, instance_eval=True)
        assert np.abs(r["logits"].numpy() - fx["logits" + suffix]).max() < 2e-4
        assert abs(float(r["instance_loss"]) - float(fx["instance_loss" + suffix])) < 2e-4
        assert np.array_equal(r["idx"], fx["idx"])
        assert np.array_equal(r["inst_preds"], fx["inst_preds"])
        assert np.array_equal(r["inst_targets"], fx["inst_targets"])
    a64 = r["A_raw"].numpy()
    assert fx["idx"].shape == (K, 2 * k) and fx["idx"].max() < N
    assert np.array_equal(select(a64, label, k, subtyping), fx["idx"])
    assert np.array_equal(targets_of(fx["idx"], label, k), fx["inst_targets"])
    # fp64 sums may differ in the last bits between BLAS builds: 1e-9 relative, far inside the gap
    assert extreme_gap(a64, label, k, subtyping) == pytest.approx(float(fx["gap"]), rel=1e-6, abs=1e-12)
    if N <= 1000:
        assert np.abs(a64 - fx["A_raw.f64"]).max() < 1e-11
        assert np.abs(fx["A_raw"].astype(np.float64) - fx["A_raw.f64"]).max() == pytest.approx(float(fx["err32"]))
    n_eval = 2 * k + (K - 1) * k * int(subtyping)
    assert (fx["idx"] >= 0).sum() == n_eval == (fx["inst_preds"] >= 0).sum()


def test_peaky_scores_need_the_max_shift():
    fx = G.load("clam_n300_peaky")
    a = fx["A_raw"]
    assert a[0].min() > 89.0 and a[1].max() < -89.0           # exp(a) overflows / underflows in fp32
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(a[0])).all() and (np.exp(a[1].astype(np.float32)) < 1e-38).all()


@pytest.mark.parametrize("name", ["clam_n300", "clam_n300_big", "clam_n300_sub_c3", "clam_n4100_c5"])
def test_state_dict_round_trip(name):
    K, N, size, k, subtyping, label = CASES[name]
    fx = G.load(name)
    ours = CLAM_MB(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping)
    sd = ours.state_dict()
    assert list(sd) == [str(s) for s in fx["keys"]]
    assert ["x".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in fx["shapes"]]
    ref = ClamMBRef(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    D = {"small": 256, "big": 384}[size]
    assert sd["attention_net.2.attention_a.0.weight"].shape == (D, 512)
    assert sd["attention_net.2.attention_c.weight"].shape == (K, D)
    assert sd["classifiers.0.weight"].shape == (1, 512) and sd[f"instance_classifiers.{K - 1}.weight"].shape == (2, 512)


def test_initialisation_follows_the_reference():
    torch.manual_seed(0)
    m = CLAM_MB(n_classes=3)
    for mod in m.modules():
        if isinstance(mod, nn.Linear):
            assert (mod.bias == 0).all()
            fan_out, fan_in = mod.weight.shape
            std = (2.0 / (fan_in + fan_out)) ** 0.5            # xavier_normal_
            if mod.weight.numel() >= 1 << 15:
                assert mod.weight.std().item() == pytest.approx(std, rel=0.05)
    assert (m.k_sample, m.n_classes, m.subtyping) == (8, 3, False)


YAML = """
General: {{precision: 32}}
Model: {{name: CLAM_MB, n_classes: 3, backbone: {backbone}{extra}}}
"""


@pytest.mark.parametrize("extra,D,k,sub", [
    ("", 256, 8, False), (", size_arg: big, k_sample: 4", 384, 4, False), (", subtyping: true", 256, 8, True),
    (", in_features: 1024, out_features: 512", 256, 8, False)])
def test_build_model_from_yaml(tmp_path, extra, D, k, sub):
    path = tmp_path / "clam.yaml"
    path.write_text(YAML.format(backbone="features", extra=extra))
    model = config.build_model(config.read_yaml(path), device="cpu")
    assert isinstance(model, CLAM_MB) and (model.n_classes, model.k_sample, model.subtyping) == (3, k, sub)
    assert model.attention_net[2].attention_c.in_features == D and len(model.instance_classifiers) == 3


def test_build_model_passes_the_named_arguments_on(tmp_path):
    """``gate: false`` / ``dropout: true`` reach the constructor, which refuses them."""
    path = tmp_path / "clam.yaml"
    for extra in (", gate: false", ", dropout: true"):
        path.write_text(YAML.format(backbone="features", extra=extra))
        with pytest.raises(NotImplementedError, match="not on the MI355X path"):
            config.build_model(config.read_yaml(path), device="cpu")


def test_build_model_refuses_bags_of_another_width(tmp_path):
    path = tmp_path / "clam.yaml"
    path.write_text("Data: {feature_extractor: retccl}\nModel: {name: CLAM_MB, n_classes: 2, backbone: features}\n")
    with pytest.raises(ValueError, match="not on the MI355X path for Data.feature_extractor retccl, whose bags are "
                                         "2048 wide"):
        config.build_model(config.read_yaml(path), device="cpu")
    path.write_text(YAML.format(backbone="resnet18", extra=""))
    with pytest.raises(ValueError, match="not on the MI355X path for backbone resnet18, whose bags are 512 wide"):
        config.build_model(config.read_yaml(path), device="cpu")
    from transmil_deepgraft_amd.encoder import ImageBagModel
    path.write_text(YAML.format(backbone="simple", extra=""))             # 1024 wide: composes
    model = config.build_model(config.read_yaml(path), device="cpu")
    assert isinstance(model, ImageBagModel) and isinstance(model.model, CLAM_MB)


def test_unknown_model_message_names_chowder_then_clam(tmp_path):
    path = tmp_path / "m.yaml"
    path.write_text("Model: {name: DTFDMIL, n_classes: 2}\n")
    with pytest.raises(ValueError, match="AttMIL, Chowder, CLAM_MB"):
        config.build_model(config.read_yaml(path), device="cpu")


@pytest.mark.parametrize("kw", [dict(gate=False), dict(dropout=True), dict(instance_loss_fn=nn.BCEWithLogitsLoss()),
                                dict(instance_loss_fn=nn.CrossEntropyLoss(label_smoothing=0.1))])
def test_constructor_refuses_what_the_kernels_do_not_compute(kw):
    with pytest.raises(NotImplementedError, match="CLAM_MB"):
        CLAM_MB(**kw)


def test_cpu_tensor_raises():
    m = CLAM_MB()
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        m(torch.zeros(16, 1024))
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        m(torch.zeros(1, 16, 1024), label=torch.tensor([0]), instance_eval=True)


def test_entry_points_refuse_shapes_outside_the_limits():
    """A status path: nothing is launched (every pointer is null)."""
    from transmil_deepgraft_amd import _lib
    lib = _lib.lib()
    for N, L, D, K, text in ((64, 512, 256, 9, "n_classes must be in [1, 8]"), (64, 256, 256, 2, "L must be 512"),
                             (64, 512, 258, 2, "D must be a multiple of 4"), (0, 512, 256, 2, "N must be >= 1")):
        rc = lib.tm_clam_fwd(None, None, N, L, D, K, None, None, None, None, None, None, None, 8, 0, None, None,
                             None, None, None, None, None, None, None, None, None)
        assert rc != 0 and text in _lib.last_error()
        rc = lib.tm_clam_bwd(None, None, None, None, None, N, L, D, K, None, None, None, None, None, 8, None, None,
                             None, None, None, None, None, None, None, None, None, None)
        assert rc != 0 and text in _lib.last_error()
    rc = lib.tm_clam_scores(None, 64, 256, 9, None, None, None, None)
    assert rc != 0 and "n_classes must be in [1, 8]" in _lib.last_error()
    # 300 rows: 19 blocks of 16 rows; fwd = blocks x K x (L + 2) floats
    assert lib.tm_clam_fwd_workspace(300, 2) == 19 * 2 * 514 * 4
    assert lib.tm_clam_fwd_workspace(300, 9) == 0
    assert lib.tm_clam_bwd_workspace(300, 256, 2, 8) == (2 * 512 + 8 + 32 + 32 * 512 + 19 * 2 * 257) * 4
