"""Chowder without a GPU: state dict, config, the task's tuple unwrap, the refusal of CPU tensors,
the entry points' status path and the fixtures' forced-selection condition."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as G
from chowder_ref import ChowderRef, case_input, bf16_round, extreme_gap, fixture_cases, rounding_bound, select
from oracle.transmil_ref import deterministic_params_
from transmil_deepgraft_amd import config
from transmil_deepgraft_amd.interface import TransMILTask
from transmil_deepgraft_amd.models import Chowder

CASES = fixture_cases()


@pytest.mark.parametrize("kw", [dict(n_classes=2), dict(n_classes=3, features=2048, r=7)])
def test_state_dict_matches_the_restatement(kw):
    ref, ours = ChowderRef(**kw), Chowder(**kw)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    r = kw.get("r", 5)
    assert want["f1.0.weight"] == (1, kw.get("features", 512), 1) and want["f2.0.weight"] == (200, 2 * r)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert (ours.L, ours.n_classes, ours.R) == (ref.L, ref.n_classes, ref.R)


YAML = """
General: {{precision: 32}}
Model: {{name: Chowder, n_classes: 3, backbone: {backbone}{extra}}}
"""


@pytest.mark.parametrize("extra,L,R", [("", 512, 5), (", r: 8", 512, 8), (", features: 2048, r: 3", 2048, 3),
                                        (", in_features: 1024, out_features: 512", 512, 5)])
def test_build_model_from_yaml(tmp_path, extra, L, R):
    path = tmp_path / "chowder.yaml"
    path.write_text(YAML.format(backbone="resnet50", extra=extra))
    model = config.build_model(config.read_yaml(path), device="cpu")
    assert isinstance(model, Chowder) and (model.L, model.R, model.n_classes) == (L, R, 3)
    assert model.f2[0].in_features == 2 * R and model.f1[0].in_channels == L


def test_build_model_with_the_resnet18_backbone(tmp_path):
    from transmil_deepgraft_amd.encoder import ImageBagModel
    path = tmp_path / "chowder.yaml"
    path.write_text(YAML.format(backbone="resnet18", extra=""))
    model = config.build_model(config.read_yaml(path), device="cpu")
    assert isinstance(model, ImageBagModel) and isinstance(model.model, Chowder) and model.model.L == 512
    path.write_text(YAML.format(backbone="resnet18", extra=", features: 1024"))
    with pytest.raises(ValueError, match="not on the MI355X path for backbone resnet18, whose bags are 512 wide"):
        config.build_model(config.read_yaml(path), device="cpu")


def test_build_model_checks_the_feature_extractors_width(tmp_path):
    """``Data.feature_extractor: retccl`` makes 2048-wide bags (code/train.py:392-397): Chowder's default
    512 features cannot take them (``in_features`` is not an argument of Chowder's), 2048 can."""
    path = tmp_path / "chowder.yaml"
    text = ("Data: {{feature_extractor: retccl}}\n"
            "Model: {{name: Chowder, n_classes: 2, backbone: features, in_features: 1024{extra}}}\n")
    path.write_text(text.format(extra=""))
    with pytest.raises(ValueError, match="features = 512 is not on the MI355X path for Data.feature_extractor retccl"):
        config.build_model(config.read_yaml(path), device="cpu")
    path.write_text(text.format(extra=", features: 2048"))
    assert config.build_model(config.read_yaml(path), device="cpu").L == 2048


def test_unknown_model_message_names_chowder(tmp_path):
    path = tmp_path / "m.yaml"
    path.write_text("Model: {name: DTFDMIL, n_classes: 2}\n")
    with pytest.raises(ValueError, match="AttMIL, Chowder"):
        config.build_model(config.read_yaml(path), device="cpu")


class _Stub(nn.Module):
    def __init__(self, shape, as_tuple):
        super().__init__()
        self.n_classes, self.shape, self.as_tuple = shape[-1], shape, as_tuple
        self.p = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        out = torch.arange(float(np.prod(self.shape))).reshape(self.shape) + self.p
        return (out, None) if self.as_tuple else out


@pytest.mark.parametrize("shape,as_tuple", [((3, 1, 2), True), ((1, 2), True), ((3, 2), False)])
def test_task_forward_unwraps_a_tuple(shape, as_tuple):
    task = TransMILTask(_Stub(shape, as_tuple))
    out = task(torch.zeros(shape[0], 4, 8))
    assert out.shape == (shape[0], 2)
    assert torch.equal(out.detach().reshape(-1), torch.arange(float(shape[0] * 2)))
    logits, prob, y_hat = task.step(torch.zeros(shape[0], 4, 8))
    assert logits.shape == prob.shape == (shape[0], 2) and y_hat.tolist() == [1] * shape[0]
    loss = task.training_step((torch.zeros(shape[0], 4, 8), torch.zeros(shape[0], dtype=torch.int64), None))
    assert loss.shape == (1,)


def test_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        Chowder(2)(torch.zeros(1, 16, 512))


def test_entry_points_refuse_shapes_outside_the_limits():
    """A status path: nothing is launched (every pointer is null)."""
    from transmil_deepgraft_amd import _lib
    lib = _lib.lib()
    for N, L, R, text in ((64, 512, 33, "R must be in"), (64, 12, 5, "multiple of 8"), (64, 4104, 5, "<= 4096"),
                          (4, 512, 5, "N must be >= R")):
        rc = lib.tm_chowder_fwd(_lib.F32, None, 1, N, L, None, None, R, None, None, 200, None, None, 100, None, None,
                                2, None, None, None, None, None, None, None)
        assert rc != 0 and text in _lib.last_error()
        rc = lib.tm_chowder_bwd(_lib.F32, None, 1, N, L, None, R, None, 200, None, 100, None, 2, None, None, None,
                                None, None, None, None, None, None, None, None, None, None, None, None)
        assert rc != 0 and text in _lib.last_error()
    assert lib.tm_chowder_fwd_workspace(2, 257, 512, 5) == 2 * 5 * 10 * 8
    assert lib.tm_chowder_bwd_workspace(2, 512, 5, 200, 100, 2) == 2 * 310 * 4


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_selection_is_forced(name):
    """gap >= 2 max_E from the stored numbers, and (the small cases) recomputed from the inputs."""
    B, N, L, R, C, bf16 = CASES[name]
    fx = G.load(name)
    assert float(fx["gap"]) >= 2.0 * float(fx["max_E"]) > 0.0
    assert fx["idx"].shape == (B, 2 * R) and fx["logits"].reshape(B, C).shape == (B, C)
    assert 0 <= fx["idx"].min() and fx["idx"].max() < N
    if B * N * L > 1 << 20:
        return
    x = case_input((B, N, L), int(fx["seed"]))
    if bf16:
        x = bf16_round(x)
    ref = deterministic_params_(ChowderRef(C, L, R), 2021).double().eval()
    with torch.no_grad():
        s = ref.scores(torch.from_numpy(x).double())[:, 0, :].numpy()
        logits = ref(torch.from_numpy(x).double())[0].numpy()
    sd = ref.state_dict()
    E = rounding_bound(x, sd["f1.0.weight"].numpy(), float(sd["f1.0.bias"]))
    # fp64 sums may differ in the last bits between BLAS builds: 1e-9 relative, far inside the gap
    assert extreme_gap(s, R) == pytest.approx(float(fx["gap"]), rel=1e-9, abs=1e-13)
    assert E.max() == pytest.approx(float(fx["max_E"]), rel=1e-9)
    assert np.array_equal(select(s, R), fx["idx"])
    assert np.allclose(logits, fx["logits.f64"], rtol=0, atol=1e-12)
