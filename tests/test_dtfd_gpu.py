"""DTFD-MIL on the GPU: the fused double-tier pseudo-bag pooling against the reference-run fixtures
(tests/golden/make_golden_dtfd.py) and fp64 autograd of the restatement (tests/dtfd_ref.py), bitwise
repeatability, the host and device permutation paths, graph capture, the two-optimizer toggling, the
limits and the task surface."""
import functools

import numpy as np
import pytest
import torch

import golden_util as G
from dtfd_ref import CASES, case_input, case_perm, optimization_step, optimizers_for, ref_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _models(name):
    """(fp64 restatement, ours on the GPU) with the fixtures' weights."""
    from transmil_deepgraft_amd.dtfd import DTFDMIL
    C, N, S, cap, label = CASES[name]
    ref = ref_model(name)
    ours = DTFDMIL(C, bag_size=S, max_pseudo_bags=cap).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, ours


def _pool(model, x, perm, label=None, return_cam=False):
    from transmil_deepgraft_amd.dtfd import dtfd_pool
    return dtfd_pool(x, perm, *model._tensors(), bag_size=model.bag_size, max_pseudo_bags=model.max_pseudo_bags,
                     label=label, return_cam=return_cam)


def _param_grads(model):
    return {k: (p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(p).double().cpu())
            for k, p in model.named_parameters()}


def _objective(sub, slide, sub_loss, slide_loss, c_sub, c_slide):
    return (slide * c_slide).sum() + (sub * c_sub).sum() + (sub_loss + slide_loss) / 2


@functools.lru_cache(maxsize=None)
def _run(name):
    """One forward + backward of a fixture case on the GPU and in fp64 on the CPU (computed once,
    shared by the tests below, never modified)."""
    C, N, S, cap, label = CASES[name]
    fx = G.load(name)
    x = case_input(N, int(fx["seed"]))
    perm = torch.from_numpy(fx["perm"])
    Gn = min(cap, N // S)
    ref, ours = _models(name)
    rng = np.random.default_rng(5)
    c_sub, c_slide = torch.from_numpy(rng.uniform(0.5, 1.5, (Gn, C))), torch.from_numpy(rng.uniform(0.5, 1.5, (1, C)))

    xr = torch.from_numpy(x).double().requires_grad_(True)
    r = ref(xr, perm, S, cap, label)
    _objective(r["sub"], r["slide"], r["sub_loss"], r["slide_loss"], c_sub, c_slide).backward()

    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    sub, slide, M, p1, p2, sub_loss, slide_loss, y_prob, y_hat, cam = _pool(
        ours, xg, perm.to(DEV), torch.tensor([label], device=DEV), return_cam=True)
    _objective(sub, slide, sub_loss, slide_loss, c_sub.to(DEV).float(), c_slide.to(DEV).float()).backward()
    torch.cuda.synchronize()
    ref_out = {k: v.detach().numpy() for k, v in r.items()}
    ours_out = dict(sub=sub, slide=slide, M=M, p1=p1, p2=p2, sub_loss=sub_loss, slide_loss=slide_loss, cam=cam,
                    y_prob=y_prob, y_hat=y_hat)
    return dict(fx=fx, G=Gn, perm=fx["perm"], ref=ref_out, g_ref=_param_grads(ref), dx_ref=xr.grad,
                ours={k: v.detach().cpu().numpy() for k, v in ours_out.items()}, g=_param_grads(ours),
                dx=xg.grad.detach().cpu())


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_forward(name):
    C, N, S, cap, label = CASES[name]
    r = _run(name)
    fx, ours, ref, Gn = r["fx"], r["ours"], r["ref"], r["G"]
    assert ours["sub"].shape == (Gn, C) and ours["slide"].shape == (1, C) and ours["M"].shape == (Gn, 512)
    assert ours["p1"].shape == (Gn, S) and ours["p2"].shape == (Gn,) and ours["cam"].shape == (Gn, S, C)
    assert ours["y_prob"].shape == (1, C) and ours["y_hat"].shape == (1,) and ours["y_hat"].dtype == np.int64
    worst = 0.0
    for key in ("sub", "slide", "M", "sub_loss", "slide_loss", "cam", "p1", "p2"):
        err = np.abs(ours[key].astype(np.float64) - ref[key]).max()
        worst = max(worst, err) if key in ("sub", "slide") else worst
        print(f"{name}: max |{key} - fp64| = {err:.3e}")
        assert err < 2e-4, key
    print(f"{name}: logits error {worst:.3e}, the reference's own fp32 error {float(fx['err32']):.3e}")
    for key in ("sub", "slide", "sub_loss", "slide_loss"):
        assert np.abs(ours[key].astype(np.float64) - fx[key + ".f64"]).max() < 2e-4, key
    assert np.abs(ours["p1"].sum(1) - 1).max() < 1e-5 and abs(ours["p2"].sum() - 1) < 1e-5
    e = np.exp(ref["slide"] - ref["slide"].max())
    assert np.abs(ours["y_prob"] - e / e.sum()).max() < 2e-4 and int(ours["y_hat"][0]) == int(ref["slide"].argmax())


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_gradients(name):
    """Measured on an MI355X: every figure is at most 0.011 of its bar except the attention biases,
    whose exact gradient is 0, against the 1e-6 floor (at most 0.35) and ``dx`` (0.49) /
    ``dimreduction.fc1.weight`` (0.014) of
    ``dtfd_n2048_s32_g64``, whose errors are in the ratio |x row| / |W1 row|: one element of h lies on
    the other side of the ReLU kink in fp32 than in fp64."""
    C, N, S, cap, label = CASES[name]
    r = _run(name)
    assert set(r["g"]) == set(r["g_ref"]) and len(r["g"]) == 17
    for k, g_ref in list(r["g_ref"].items()) + [("dx", r["dx_ref"])]:
        g = r["dx"].double() if k == "dx" else r["g"][k]
        assert g.shape == g_ref.shape, k
        err, bar = (g - g_ref).norm().item(), 2e-3 * g_ref.norm().item() + 1e-6
        print(f"{name} {k}: |g - g64| = {err:.3e} (bar {bar:.3e})")
        assert err < bar, k
    unused = r["perm"][r["G"] * S:]
    assert unused.size == N - r["G"] * S
    assert (r["dx"][unused] == 0.0).all() and (r["dx_ref"][unused] == 0.0).all()
    if not name.endswith("peaky"):                 # there p1 underflows to 0.0 for most rows, and their dx with it
        assert (r["dx"][r["perm"][:r["G"] * S]] != 0.0).any(dim=1).all()


@pytest.mark.parametrize("name", ["dtfd_n30_s7", "dtfd_n600_s257", "dtfd_n2048_s32_g64"])
def test_two_runs_agree_bitwise(name):
    C, N, S, cap, label = CASES[name]
    fx = G.load(name)
    _, ours = _models(name)
    perm, lab = torch.from_numpy(fx["perm"]).to(DEV), torch.tensor([label], device=DEV)
    runs = []
    for _ in range(2):
        ours.zero_grad(set_to_none=True)
        x = torch.from_numpy(case_input(N, int(fx["seed"]))).to(DEV).requires_grad_(True)
        out = _pool(ours, x, perm, lab, return_cam=True)
        (out[0].sum() + out[1].sum() + (out[5] + out[6]) / 2).backward()
        runs.append(list(out) + [x.grad] + [p.grad for p in ours.parameters()])
    assert len(runs[0]) == 10 + 1 + 17
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_host_perm_equals_device_perm_and_draws_once():
    name = "dtfd_n239_s120"
    C, N, S, cap, label = CASES[name]
    _, ours = _models(name)
    x = torch.from_numpy(case_input(N, 2)).to(DEV)
    lab = torch.tensor([label], device=DEV)
    with torch.no_grad():
        torch.manual_seed(77)
        drawn = ours(x, label=lab)                              # perm=None: the forward draws
        state = torch.get_rng_state()
        torch.manual_seed(77)
        perm = torch.randperm(N)
        assert torch.equal(torch.get_rng_state(), state)         # one randperm(N) and nothing else
        on_device = ours(x, perm=perm.to(DEV), label=lab)
        on_host = ours(x[None], perm=perm, label=lab)            # [1, N, F], a checked CPU perm
        other = ours(x, perm=torch.randperm(N).to(DEV), label=lab)
    for a, b, c in zip(drawn[:4], on_device[:4], on_host[:4]):
        assert torch.equal(a, b) and torch.equal(a, c)
    for key in ("sub_loss", "slide_loss", "M", "p1", "p2"):
        assert torch.equal(drawn[4][key], on_device[4][key]) and torch.equal(drawn[4][key], on_host[4][key])
    assert not torch.equal(drawn[0], other[0])                   # another permutation, other pseudo-bags
    assert set(drawn[4]) == {"sub_loss", "slide_loss", "M", "p1", "p2"}
    with torch.no_grad():
        plain = ours(x, perm=perm.to(DEV))
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, on_device[:4]))
    bad = perm.clone()
    bad[0] = bad[1]
    with pytest.raises(ValueError, match="every row id"):
        ours(x, perm=bad)
    with pytest.raises(RuntimeError, match="holds no pseudo-bag"):
        ours(x[:119])


def test_graph_capture_reads_perm_and_label_on_the_device():
    """dtfd_pool forward + backward captured once; the permutation and the label are then overwritten in
    place and the replay equals the eager run on the new contents (so nothing read them on the host)."""
    name = "dtfd_n960_s120_c3"
    C, N, S, cap, label = CASES[name]
    _, ours = _models(name)
    params = list(ours.parameters())
    x = torch.from_numpy(case_input(N, 6)).to(DEV)
    perms = [case_perm(N, s).to(DEV) for s in (0, 1)]
    labels = [torch.tensor([2], device=DEV), torch.tensor([0], device=DEV)]

    def step(x, perm, lab):
        out = _pool(ours, x, perm, lab, return_cam=True)
        grads = torch.autograd.grad(out[0].sum() + out[1].sum() + (out[5] + out[6]) / 2, [x] + params)
        return list(out) + list(grads)

    x_s, perm_s, lab_s = x.clone().requires_grad_(True), perms[0].clone(), labels[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x_s, perm_s, lab_s)                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(x_s, perm_s, lab_s)
    perm_s.copy_(perms[1])
    lab_s.copy_(labels[1])
    graph.replay()
    torch.cuda.synchronize()
    eager = step(x.clone().requires_grad_(True), perms[1], labels[1])
    eager0 = step(x.clone().requires_grad_(True), perms[0], labels[0])
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
    assert not torch.equal(captured[0], eager0[0]) and not torch.equal(captured[5], eager0[5])


def test_optimization_step_toggles_the_two_groups():
    from transmil_deepgraft_amd.dtfd import DTFDTask
    name = "dtfd_n239_s120"
    C, N, S, cap, label = CASES[name]
    ref, ours = _models(name)
    task = DTFDTask(ours)
    opts, _ = task.configure_optimizers()
    first, second = ours.group_parameters()
    snap = lambda ps: [p.detach().clone() for p in ps]
    start = (snap(first), snap(second))
    seen = {}
    opts[0].register_step_post_hook(lambda *a: seen.update(after0=(snap(first), snap(second))))
    opts[1].register_step_pre_hook(lambda *a: seen.update(
        grads1=[p.grad is None for p in first], flags1=[p.requires_grad for p in first],
        own1=[p.grad is not None for p in second]))
    x = case_input(N, 2)
    hot = torch.nn.functional.one_hot(torch.tensor([label]), C).float().to(DEV)          # the reference's label row
    torch.manual_seed(11)
    outs = task.optimization_step((torch.from_numpy(x)[None].to(DEV), hot, None), opts)
    torch.cuda.synchronize()
    # pass 0: attCls bitwise unchanged, every tensor of group 0 changed
    assert all(torch.equal(a, b) for a, b in zip(seen["after0"][1], start[1]))
    assert all(not torch.equal(a, b) for a, b in zip(seen["after0"][0], start[0]))
    # pass 1: the other way round; group 0 had no gradient and was switched off
    assert all(torch.equal(p, b) for p, b in zip(first, seen["after0"][0]))
    assert all(not torch.equal(p, b) for p, b in zip(second, seen["after0"][1]))
    assert all(seen["grads1"]) and not any(seen["flags1"]) and all(seen["own1"])
    assert all(p.requires_grad and p.grad is None for p in ours.parameters())
    # the two totals against the fp64 two-pass restatement on the same two draws
    torch.manual_seed(11)
    perms = [torch.randperm(N), torch.randperm(N)]
    ref.train()
    totals = optimization_step(ref, torch.from_numpy(x).double(), label, perms, S, cap, optimizers_for(ref))
    for out, want in zip(outs, totals):
        assert set(out) == {"loss", "Y_prob", "Y_hat", "label"} and int(out["label"]) == label
        print(f"total {out['loss'].item():.6f} fp64 {want:.6f}")
        assert abs(out["loss"].item() - want) < 2e-4
    assert abs(totals[0] - totals[1]) > 1e-6                     # a fresh permutation per pass


def test_validation_step_returns_device_tensors():
    from transmil_deepgraft_amd.dtfd import DTFDTask
    name = "dtfd_n130_s65_c5"
    C, N, S, cap, label = CASES[name]
    fx = G.load(name)
    ref, ours = _models(name)
    x = case_input(N, int(fx["seed"]))
    torch.manual_seed(int(fx["seed"]))
    out = DTFDTask(ours).validation_step((torch.from_numpy(x)[None].to(DEV), torch.tensor([label]), None))
    assert set(out) == {"val_sub_loss", "val_slide_loss", "logits", "Y_prob", "Y_hat", "label"}
    assert all(v.is_cuda and not v.requires_grad for v in out.values())
    assert abs(float(out["val_sub_loss"]) - float(fx["sub_loss.f64"])) < 2e-4
    assert abs(float(out["val_slide_loss"]) - float(fx["slide_loss.f64"])) < 2e-4
    assert np.abs(out["logits"].cpu().numpy() - fx["slide.f64"]).max() < 2e-4 and int(out["label"]) == label


def test_shapes_outside_the_limits_raise():
    from transmil_deepgraft_amd.dtfd import DTFDMIL, dtfd_pool
    m = DTFDMIL(2).to(DEV)
    t = list(m._tensors())
    x = torch.zeros(1100, 1024, device=DEV)
    perm = torch.arange(1100, device=DEV)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    with pytest.raises(RuntimeError, match=r"n_classes must be in \[1, 8\]"):
        dtfd_pool(x, perm, *t[:7], z(9, 512), z(9), *t[9:])
    with pytest.raises(RuntimeError, match="m_dim must be 512"):
        dtfd_pool(x, perm, z(256, 1024), *t[1:])
    with pytest.raises(RuntimeError, match="D must be a multiple of 4, <= 512"):
        dtfd_pool(x, perm, t[0], z(516, 512), z(516), z(516, 512), z(516), z(1, 516), *t[6:])
    with pytest.raises(RuntimeError, match=r"bag_size must be in \[1, 1024\]"):
        dtfd_pool(x, perm, *t, bag_size=1025)
    with pytest.raises(RuntimeError, match=r"pseudo-bags must be in \[1, 64\]"):
        dtfd_pool(x, perm, *t, bag_size=1, max_pseudo_bags=65)
    with pytest.raises(RuntimeError, match="holds no pseudo-bag"):
        dtfd_pool(x[:100], perm[:100], *t)
    with pytest.raises(RuntimeError, match="int64 GPU tensor"):
        dtfd_pool(x, perm.cpu(), *t)
    with pytest.raises(RuntimeError, match="label must be an int64 GPU tensor"):
        dtfd_pool(x, perm, *t, label=torch.tensor([0]))
    out = dtfd_pool(x, perm, *t, bag_size=1, max_pseudo_bags=64)             # the largest G is served
    assert len(out) == 5 and out[0].shape == (64, 2) and torch.isfinite(out[1]).all()


def test_a_label_outside_the_classes_gives_nan_losses():
    """As tm_ce_fwd: the kernel reads the label, finds no class for it and writes NaN; nothing else changes."""
    name = "dtfd_n30_s7"
    C, N, S, cap, label = CASES[name]
    _, ours = _models(name)
    x = torch.from_numpy(case_input(N, 3)).to(DEV)
    perm = case_perm(N, 3).to(DEV)
    with torch.no_grad():
        good = _pool(ours, x, perm, torch.tensor([label], device=DEV))
        for bad_label in (C, -1):
            bad = _pool(ours, x, perm, torch.tensor([bad_label], device=DEV))
            assert torch.isnan(bad[5]) and torch.isnan(bad[6])
            for i in (0, 1, 2, 3, 4, 7, 8):
                assert torch.equal(bad[i], good[i])
    assert torch.isfinite(good[5]) and torch.isfinite(good[6])
