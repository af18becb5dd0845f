"""DTFD-MIL without a GPU: the restatement against the reference-run fixtures, the state dict, the
constructors' refusals, the refusal of CPU tensors and short bags, the entry that is not
``config.build_model``, the optimizers and the entry points' status path."""
import numpy as np
import pytest
import torch

import golden_util as G
from dtfd_ref import CASES, DtfdRef, case_input, case_perm, optimization_step, optimizers_for, ref_model
from transmil_deepgraft_amd import config, dtfd
from transmil_deepgraft_amd.dtfd import (Attention_Gated, Attention_with_Classifier, Classifier_1fc, DimReduction,
                                         DTFDMIL, DTFDTask, residual_block)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_fixture(name):
    C, N, S, cap, label = CASES[name]
    fx = G.load(name)
    seed = int(fx["seed"])
    perm = case_perm(N, seed)
    assert np.array_equal(perm.numpy(), fx["perm"]) and np.array_equal(np.sort(fx["perm"]), np.arange(N))
    x = torch.from_numpy(case_input(N, seed))
    Gn = min(cap, N // S)
    for dtype, suffix, bar in ((torch.float32, "", 2e-4), (torch.float64, ".f64", 1e-10)):
        with torch.no_grad():
            r = ref_model(name, dtype)(x.to(dtype), perm, S, cap, label)
        assert r["sub"].shape == (Gn, C) and r["slide"].shape == (1, C)
        assert np.abs(r["sub"].numpy() - fx["sub" + suffix]).max() < bar
        assert np.abs(r["slide"].numpy() - fx["slide" + suffix]).max() < bar
        assert abs(float(r["sub_loss"]) - float(fx["sub_loss" + suffix])) < bar
        assert abs(float(r["slide_loss"]) - float(fx["slide_loss" + suffix])) < bar
    assert max(np.abs(fx["sub.f64"]).max(), np.abs(fx["slide.f64"]).max()) >= 1.0      # the absolute bar bites
    err32 = max(np.abs(fx["sub"] - fx["sub.f64"]).max(), np.abs(fx["slide"] - fx["slide.f64"]).max())
    assert err32 == pytest.approx(float(fx["err32"])) and 0.0 < err32 < 2e-4
    assert r["cam"].shape == (Gn, S, C) and r["p1"].shape == (Gn, S) and r["p2"].shape == (Gn,)
    # the CAM of :204-205 sums over the instances to the pseudo-bag's logits without the bias
    bias = ref_model(name).classifier.fc.bias
    assert (r["cam"].sum(1) + bias - r["sub"]).abs().max() < 1e-10


def test_peaky_scores_need_the_max_shift():
    name = "dtfd_n960_s120_peaky"
    C, N, S, cap, label = CASES[name]
    fx = G.load(name)
    with torch.no_grad():
        r = ref_model(name)(torch.from_numpy(case_input(N, int(fx["seed"]))).double(), case_perm(N, int(fx["seed"])),
                            S, cap, label)
    a = r["a1"].numpy()
    assert a.max() > 89.0 and a.min() < -89.0                  # exp(a) overflows / underflows in fp32
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(a.astype(np.float32))).any()


@pytest.mark.parametrize("name", ["dtfd_n120_s120", "dtfd_n130_s65_c5", "dtfd_n960_s120_c3"])
def test_state_dict_round_trip(name):
    C = CASES[name][0]
    fx = G.load(name)
    ours = DTFDMIL(C)
    sd = ours.state_dict()
    assert list(sd) == [str(s) for s in fx["keys"]]
    assert ["x".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in fx["shapes"]]
    ref = DtfdRef(C)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert sd["dimreduction.fc1.weight"].shape == (512, 1024) and "dimreduction.fc1.bias" not in sd
    assert sd["attention.attention_V.0.weight"].shape == (128, 512)
    assert sd["attention.attention_weights.weight"].shape == (1, 128)
    assert sd["classifier.fc.weight"].shape == (C, 512) and sd["attCls.classifier.fc.weight"].shape == (C, 512)
    assert sd["attCls.attention.attention_U.0.bias"].shape == (128,)


def test_containers_take_the_reference_arguments():
    assert Attention_Gated(features=256, D=64, K=1).attention_V[0].weight.shape == (64, 256)
    assert Classifier_1fc(512, 3, droprate=0.0).fc.weight.shape == (3, 512)
    assert [tuple(p.shape) for p in residual_block(nChn=256).parameters()] == [(256, 256), (256, 256)]
    assert DimReduction(1024, m_dim=512, numLayer_Res=0).fc1.bias is None
    m = Attention_with_Classifier(L=512, D=128, K=1, num_cls=4, droprate=0)
    assert m.classifier.fc.weight.shape == (4, 512) and m.attention.attention_weights.weight.shape == (1, 128)


@pytest.mark.parametrize("make", [
    lambda: Attention_Gated(K=2), lambda: Classifier_1fc(512, 2, droprate=0.25),
    lambda: DimReduction(1024, numLayer_Res=1), lambda: Attention_with_Classifier(K=3),
    lambda: Attention_with_Classifier(droprate=0.5)])
def test_constructors_refuse_what_the_kernels_do_not_compute(make):
    with pytest.raises(NotImplementedError, match="not on the MI355X path"):
        make()


def test_cpu_tensor_raises():
    m = DTFDMIL(2)
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        m(torch.zeros(240, 1024))
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        m(torch.zeros(1, 240, 1024), label=torch.tensor([0]))
    with pytest.raises(RuntimeError, match="needs a GPU tensor: there is no CPU path"):
        dtfd.dtfd_pool(torch.zeros(240, 1024), torch.arange(240), *m._tensors())


def test_a_bag_shorter_than_bag_size_raises():
    """The reference fails there too (torch.cat of an empty list); checked on the shape alone, before the device."""
    m = DTFDMIL(2)
    with pytest.raises(RuntimeError, match="holds no pseudo-bag of bag_size = 120"):
        m(torch.zeros(119, 1024))
    with pytest.raises(RuntimeError, match="holds no pseudo-bag of bag_size = 7"):
        m(torch.zeros(1, 6, 1024), bag_size=7)
    with pytest.raises(RuntimeError, match="needs a GPU tensor"):
        m(torch.zeros(1, 7, 1024), bag_size=7)


def test_models_package_does_not_gain_the_name(tmp_path):
    import transmil_deepgraft_amd.models as models
    assert not hasattr(models, "DTFDMIL")
    path = tmp_path / "m.yaml"
    path.write_text("Model: {name: DTFDMIL, n_classes: 2}\n")
    with pytest.raises(ValueError, match="'DTFDMIL' is not on the MI355X path"):
        config.build_model(config.read_yaml(path), device="cpu")


YAML = """
General: {{precision: 16, grad_acc: 2}}
Model: {{name: DTFDMIL, n_classes: {C}, backbone: resnet50, in_features: 512, out_features: 512{extra}}}
Optimizer: {{opt: lookahead_radam, lr: 0.0002, weight_decay: 0.01}}
Loss: {{base_loss: CrossEntropyLoss}}
"""


@pytest.mark.parametrize("C,extra,S,cap", [(2, "", 120, 8), (3, ", bag_size: 64, max_pseudo_bags: 16", 64, 16)])
def test_build_dtfd_task_from_yaml(tmp_path, C, extra, S, cap):
    path = tmp_path / "dtfd.yaml"
    path.write_text(YAML.format(C=C, extra=extra))
    task = config.build_dtfd_task(config.read_yaml(path), device="cpu")
    assert isinstance(task, DTFDTask) and isinstance(task.model, DTFDMIL)
    m = task.model
    assert (m.n_classes, m.bag_size, m.max_pseudo_bags, m.in_features) == (C, S, cap, 1024)
    assert m.dimreduction.fc1.weight.shape == (512, 1024)          # self.out_features = 1024, not Model.in_features


def test_configure_optimizers_returns_the_two_groups():
    task = DTFDTask(DTFDMIL(2))
    opts, scheds = task.configure_optimizers()
    assert len(opts) == 2 and len(scheds) == 2
    m = task.model
    first = list(m.classifier.parameters()) + list(m.attention.parameters()) + list(m.dimreduction.parameters())
    second = list(m.attCls.parameters())
    for opt, want in zip(opts, (first, second)):
        assert type(opt) is torch.optim.Adam and len(opt.param_groups) == 1
        got = opt.param_groups[0]
        assert len(got["params"]) == len(want) and all(a is b for a, b in zip(got["params"], want))
        assert got["lr"] == 1e-4 and got["weight_decay"] == 1e-2
    assert len(first) == 9 and len(second) == 8 and len(first) + len(second) == len(list(m.parameters()))
    for s, opt in zip(scheds, opts):
        assert type(s) is torch.optim.lr_scheduler.MultiStepLR and s.optimizer is opt
        assert dict(s.milestones) == {100: 1} and s.gamma == 0.2


def test_restated_optimization_step_toggles_the_groups():
    """The fp64 two-pass step the GPU test compares with: pass 0 moves group 0 only, pass 1 attCls only."""
    name = "dtfd_n30_s7"
    C, N, S, cap, label = CASES[name]
    model = ref_model(name).train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.from_numpy(case_input(N, 3)).double()
    perms = [case_perm(N, 3), torch.randperm(N)]
    totals = optimization_step(model, x, label, perms, S, cap, optimizers_for(model))
    assert len(totals) == 2 and all(np.isfinite(totals))
    for k, v in model.state_dict().items():
        assert not torch.equal(v, before[k]), k
    assert all(p.requires_grad and p.grad is None for p in model.parameters())


def test_entry_points_refuse_shapes_outside_the_limits():
    """A status path: nothing is launched (every pointer is null)."""
    from transmil_deepgraft_amd import _lib
    lib = _lib.lib()
    cases = ((8, 120, 256, 128, 2, "m_dim must be 512"), (8, 120, 512, 516, 2, "D must be a multiple of 4, <= 512"),
             (8, 120, 512, 130, 2, "D must be a multiple of 4"), (8, 120, 512, 128, 9, "n_classes must be in [1, 8]"),
             (8, 120, 512, 128, 0, "n_classes must be in [1, 8]"), (8, 1025, 512, 128, 2, "bag_size must be in [1, 1024]"),
             (8, 0, 512, 128, 2, "bag_size must be in [1, 1024]"), (65, 120, 512, 128, 2, "pseudo-bags must be in [1, 64]"),
             (0, 120, 512, 128, 2, "pseudo-bags must be in [1, 64]"))
    for Gn, S, L, D, C, text in cases:
        rc = lib.tm_dtfd_fwd(None, None, Gn, S, L, D, C, *([None] * 25))
        assert rc != 0 and text in _lib.last_error(), (text, _lib.last_error())
        rc = lib.tm_dtfd_bwd(*([None] * 10), Gn, S, L, D, C, *([None] * 10), 1, 1, *([None] * 16))
        assert rc != 0 and text in _lib.last_error(), (text, _lib.last_error())
    # dsub [64 x 8] | dF [512] | dw partials [G x D] | db partials [64] | ceil(D / 8) slices x G x 512
    assert lib.tm_dtfd_bwd_workspace(8, 128, 2) == (512 + 512 + 8 * 128 + 64 + 16 * 8 * 512) * 4
    assert lib.tm_dtfd_bwd_workspace(65, 128, 2) == 0 and lib.tm_dtfd_bwd_workspace(8, 128, 9) == 0
    # in limits, but no gradient asked for: nothing to do, nothing launched
    assert lib.tm_dtfd_bwd(*([None] * 10), 8, 120, 512, 128, 2, *([None] * 10), 0, 0, *([None] * 16)) == 0
