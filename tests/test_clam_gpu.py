"""CLAM_MB on the GPU: the fused gated-attention pooling, instance selection and instance loss
against the reference-run fixtures (tests/golden/make_golden_clam.py) and fp64 autograd of the
restatement (tests/clam_ref.py), bitwise repeatability, placement and tie cases with indices known
in closed form, the forward's modes, the error path, graph capture and the task surface."""
import functools

import numpy as np
import pytest
import torch

import golden_util as G
from clam_ref import case_input, fixture_cases, ref_model, select, targets_of

CASES = fixture_cases()

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _models(name, case=None):
    """(fp64 restatement, ours on the GPU) with the fixtures' weights."""
    from transmil_deepgraft_amd.models import CLAM_MB
    K, N, size, k, subtyping, label = case or CASES[name]
    ref = ref_model(name, (K, N, size, k, subtyping, label))
    ours = CLAM_MB(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping).to(DEV)
    ours.load_state_dict({kk: v.float() for kk, v in ref.state_dict().items()}, strict=True)
    return ref, ours


def _pool(model, x, label=None):
    """clam_pool on the module's parameters: (logits, A_raw, M, instance_loss, idx, preds, targets)."""
    from transmil_deepgraft_amd.models.CLAM import clam_pool
    Wcls = torch.cat([m.weight for m in model.classifiers])
    bcls = torch.cat([m.bias for m in model.classifiers])
    Wic = torch.stack([m.weight for m in model.instance_classifiers])
    bic = torch.stack([m.bias for m in model.instance_classifiers])
    if label is not None and not torch.is_tensor(label):
        label = torch.tensor([label], device=DEV)
    return clam_pool(x, *model._params(), Wcls, bcls, Wic, bic, label, model.k_sample, model.subtyping)


def _param_grads(model):
    return {k: (p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(p).double().cpu())
            for k, p in model.named_parameters()}


def _objective(logits, loss, coef):
    return (logits * coef).sum() + 0.5 * loss


@functools.lru_cache(maxsize=None)
def _run(name):
    """One forward + backward of a fixture case on the GPU and in fp64 on the CPU (computed once,
    shared by the tests below, never modified)."""
    K, N, size, k, subtyping, label = CASES[name]
    fx = G.load(name)
    x = case_input(N, int(fx["seed"]))
    ref, ours = _models(name)
    coef = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 1.5, (1, K)))

    xr = torch.from_numpy(x).double().requires_grad_(True)
    r = ref(xr, label, instance_eval=True)
    _objective(r["logits"], r["instance_loss"], coef).backward()

    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    logits, A_raw, M, loss, idx, preds, targets = _pool(ours, xg, label)
    _objective(logits, loss, coef.to(DEV).float()).backward()
    torch.cuda.synchronize()
    return dict(fx=fx, a_ref=r["A_raw"].detach().numpy(), l_ref=r["logits"].detach().numpy(),
                loss_ref=float(r["instance_loss"].detach()), M_ref=r["M"].detach().numpy(), g_ref=_param_grads(ref),
                dx_ref=xr.grad, logits=logits.detach().cpu().numpy(), A_raw=A_raw.cpu().numpy(),
                M=M.cpu().numpy(), loss=float(loss), idx=idx.cpu().numpy(), preds=preds.cpu().numpy(),
                targets=targets.cpu().numpy(), g=_param_grads(ours), dx=xg.grad.detach().double().cpu())


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_forward(name):
    K, N, size, k, subtyping, label = CASES[name]
    r = _run(name)
    fx = r["fx"]
    assert r["A_raw"].shape == (K, N) and r["logits"].shape == (1, K)
    serr = np.abs(r["A_raw"].astype(np.float64) - r["a_ref"]).max()
    print(f"{name}: max |A_raw - a64| = {serr:.3e} (bar gap / 4 = {float(fx['gap']) / 4:.3e}, "
          f"reference fp32 {float(fx['err32']):.3e})")
    assert serr < float(fx["gap"]) / 4
    for key, got in (("idx", r["idx"]), ("inst_targets", r["targets"]), ("inst_preds", r["preds"])):
        assert got.dtype == np.int32 and got.shape == (K, 2 * k)
        assert np.array_equal(got, fx[key]), (key, got, fx[key])
    lerr = np.abs(r["logits"].astype(np.float64) - r["l_ref"]).max()
    print(f"{name}: max |logits - fp64| = {lerr:.3e}, |instance_loss - fp64| = {abs(r['loss'] - r['loss_ref']):.3e}")
    assert lerr < 2e-4 and np.abs(r["logits"] - fx["logits.f64"]).max() < 2e-4
    assert abs(r["loss"] - r["loss_ref"]) < 2e-4 and abs(r["loss"] - float(fx["instance_loss.f64"])) < 2e-4
    assert np.abs(r["M"].astype(np.float64) - r["M_ref"]).max() < 2e-4


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_gradients(name):
    r = _run(name)
    assert set(r["g"]) == set(r["g_ref"])
    for k, g_ref in list(r["g_ref"].items()) + [("dx", r["dx_ref"])]:
        g = r["dx"] if k == "dx" else r["g"][k]
        assert g.shape == g_ref.shape, k
        err, bar = (g - g_ref).norm().item(), 2e-3 * g_ref.norm().item() + 1e-6
        print(f"{name} {k}: |g - g64| = {err:.3e} (bar {bar:.3e})")
        assert err < bar, k


@pytest.mark.parametrize("name", ["clam_n8", "clam_n300_sub_c3"])
def test_two_runs_agree_bitwise(name):
    """The cases where a row is selected more than once (as largest and smallest, or by several classes)."""
    K, N, size, k, subtyping, label = CASES[name]
    fx = G.load(name)
    _, ours = _models(name)
    runs = []
    for _ in range(2):
        ours.zero_grad(set_to_none=True)
        x = torch.from_numpy(case_input(N, int(fx["seed"]))).to(DEV).requires_grad_(True)
        out = _pool(ours, x, label)
        (out[0].sum() + 0.5 * out[3]).backward()
        runs.append(list(out) + [x.grad] + [p.grad for p in ours.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _closed_form_model(K, k, subtyping):
    """Fixture weights, but the scores are a closed form of column 0 of the bag:
    a[c, i] = Wc[c, 0] * 0.5 * tanh(x[i, 0]) + bc[c]  (h[:, 0] = x[:, 0], Za[:, 0] = h[:, 0], Zb = 0)."""
    _, ours = _models("closed", (K, 0, "small", k, subtyping, 0))
    fc, gated = ours.attention_net[0], ours.attention_net[2]
    with torch.no_grad():
        for lin in (fc, gated.attention_a[0], gated.attention_b[0]):
            lin.weight.zero_()
            lin.bias.zero_()
        fc.weight[0, 0] = 1.0
        gated.attention_a[0].weight[0, 0] = 1.0
        gated.attention_c.weight.zero_()
    return ours


@pytest.mark.parametrize("N", [8, 300, 4100])
def test_all_ties_take_the_lowest_indices(N):
    """Wa = Wb = 0 (and ba = 0): every score of class c equals bc[c], so both sides take rows 0..k-1."""
    K, k = 3, 8
    ours = _closed_form_model(K, k, True)
    with torch.no_grad():
        ours.attention_net[2].attention_a[0].weight.zero_()
    x = torch.from_numpy(case_input(N, 3)).to(DEV)
    _, A_raw, _, _, idx, _, targets = _pool(ours, x, 1)
    bc = ours.attention_net[2].attention_c.bias.detach()
    assert torch.equal(A_raw, bc[:, None].expand(K, N))
    want = np.full((K, 2 * k), -1)
    want[:, :k] = np.arange(k)
    want[1, k:] = np.arange(k)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(targets.cpu().numpy(), targets_of(want, 1, k))


@pytest.mark.parametrize("N", [257, 300, 4100])
def test_planted_extremes_at_block_boundaries(N):
    """Extremes planted at rows 0, 15 / 16, 63 / 64 (the ends of 16- and 64-row blocks) and N - 1."""
    K, k = 2, 8
    ours = _closed_form_model(K, k, True)
    with torch.no_grad():
        ours.attention_net[2].attention_c.weight[0, 0] = 1.0
        ours.attention_net[2].attention_c.weight[1, 0] = -1.0
    top = np.array([0, 15, 16, 63, 64, 65, N - 2, N - 1])
    bot = np.array([1, 14, 17, 62, 66, 127, 128, N - 3])
    x = case_input(N, 4)
    x[:, 0] = 0.3 + 0.4 * np.random.default_rng(11).permutation(N) / N
    x[top, 0] = 0.9 + 0.01 * np.arange(k)
    x[bot, 0] = 0.01 + 0.01 * np.arange(k)
    want = np.full((K, 2 * k), -1)
    want[0, :k] = top[::-1]                     # class 0 (out of class): its k largest
    want[1] = np.concatenate([bot, top[::-1]])  # class 1 = label, weight -1: largest = smallest x, then the smallest
    a = np.stack([0.5 * np.tanh(x[:, 0].astype(np.float64)), -0.5 * np.tanh(x[:, 0].astype(np.float64))])
    assert np.array_equal(select(a, 1, k, True), want)      # the closed form is the contract's selection
    _, A_raw, _, _, idx, _, _ = _pool(ours, torch.from_numpy(x).to(DEV), 1)
    bc = ours.attention_net[2].attention_c.bias.detach().double().cpu().numpy()
    assert np.abs(A_raw.cpu().numpy() - (a + bc[:, None])).max() < 1e-6
    assert np.array_equal(idx.cpu().numpy(), want)


def test_modes_agree():
    name = "clam_n300_sub_c3"
    K, N, size, k, subtyping, label = CASES[name]
    _, ours = _models(name)
    x = torch.from_numpy(case_input(N, 0)).to(DEV)
    lab = torch.tensor([label], device=DEV)
    with torch.no_grad():
        l1, prob, y_hat, A1, res1 = ours(x, label=lab, instance_eval=True, return_features=True)
        l0, _, _, A0, res0 = ours(x)
        A_only = ours(x, attention_only=True)
        l3, _, _, A3, _ = ours(x[None], label=lab, instance_eval=True)      # [1, N, 1024]
        pooled = _pool(ours, x, lab)
    assert res0 == {} and set(res1) == {"instance_loss", "inst_labels", "inst_preds", "features"}
    assert torch.equal(l0, l1) and torch.equal(A0, A1) and torch.equal(l3, l1) and torch.equal(A3, A1)
    assert torch.equal(A_only, A1) and A_only.shape == (K, N)
    assert torch.equal(res1["features"], pooled[2]) and res1["features"].shape == (K, 512)
    assert torch.equal(res1["instance_loss"], pooled[3])
    assert prob.shape == (1, K) and y_hat.shape == (1, 1) and int(y_hat) == int(l1.argmax())
    fx = G.load(name)
    n_eval = 2 * k + (K - 1) * k
    assert isinstance(res1["inst_preds"], np.ndarray) and res1["inst_preds"].shape == (n_eval,)
    assert np.array_equal(res1["inst_preds"], fx["inst_preds"][fx["inst_preds"] >= 0])
    assert np.array_equal(res1["inst_labels"], fx["inst_targets"][fx["inst_targets"] >= 0])


def test_a_bag_smaller_than_k_sample_raises():
    _, ours = _models("clam_n8")
    x = torch.zeros(7, 1024, device=DEV)
    with pytest.raises(RuntimeError, match="out of range"):
        ours(x, label=torch.tensor([0], device=DEV), instance_eval=True)
    assert ours(x)[0].shape == (1, 2)                       # without instance evaluation the bag is fine
    from transmil_deepgraft_amd import _lib
    rc = _lib.lib().tm_clam_fwd(None, None, 7, 512, 256, 2, None, None, None, None, None, None, x.data_ptr(), 8, 0,
                                None, None, None, None, None, None, None, None, None, None, None)
    assert rc != 0 and "N must be >= k_sample" in _lib.last_error()


def test_graph_capture_reads_the_label_on_the_device():
    """clam_pool forward + backward captured once; the bag and the label are then overwritten in place
    and the replay equals the eager run on the new data (so nothing read the label on the host)."""
    name = "clam_n300_sub_c3"
    K, N, size, k, subtyping, label = CASES[name]
    _, ours = _models(name)
    params = list(ours.parameters())
    bags = [torch.from_numpy(case_input(N, s)).to(DEV) for s in (0, 1)]
    labels = [torch.tensor([1], device=DEV), torch.tensor([2], device=DEV)]

    def step(x, lab):
        out = _pool(ours, x, lab)
        grads = torch.autograd.grad(out[0].sum() + 0.5 * out[3], [x] + params)
        return list(out) + list(grads)

    x_s, lab_s = bags[0].clone().requires_grad_(True), labels[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x_s, lab_s)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(x_s, lab_s)
    with torch.no_grad():
        x_s.copy_(bags[1])
        lab_s.copy_(labels[1])
    graph.replay()
    torch.cuda.synchronize()
    eager = step(bags[1].clone().requires_grad_(True), labels[1])
    eager0 = step(bags[0].clone().requires_grad_(True), labels[0])
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
    assert not torch.equal(captured[4], eager0[4])           # the other label selects other rows


def test_task_training_step():
    from transmil_deepgraft_amd.interface import TransMILTask
    name = "clam_n300"
    ref, ours = _models(name)
    task = TransMILTask(ours)
    x = case_input(300, 9)
    label = torch.tensor([1], device=DEV)
    loss = task.training_step((torch.from_numpy(x)[None].to(DEV), label, None))
    task.backward(loss)
    with torch.no_grad():
        lr = ref(torch.from_numpy(x).double())["logits"]
    want = torch.nn.functional.cross_entropy(lr, label.cpu())
    assert abs(loss.item() - want.item()) < 1e-4
    for k, p in ours.named_parameters():
        assert (p.grad is None) == k.startswith("instance_classifiers"), k
