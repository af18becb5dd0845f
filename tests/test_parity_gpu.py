"""Whole-model parity: the HIP TransMIL (through the C ABI) against the CPU oracle.

Bar (BASELINE.json north_star): fp32 logits within 1e-4 of the reference CPU
path, class argmax bit-exact.  Gradients: max relative error (to the largest
entry of each tensor) 2e-3 in the fp32 parity mode.  bf16 (bench) mode is held
to argmax equality on clear-margin bags and 5e-2 on logits.
"""
import numpy as np
import pytest
import torch

from golden_util import load, bag_input
from kernel_refs import dropout_keep

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pair(ncls, feat=512, seed=2021, dtype=torch.float32):
    from oracle.transmil_ref import TransMIL as Ref, deterministic_params_
    from transmil_deepgraft_amd.models import TransMIL
    torch.manual_seed(0)
    ref = deterministic_params_(Ref(ncls, feat, 512), seed).double().eval()
    ours = TransMIL(ncls, feat, 512).to(DEV).eval()
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.set_compute_dtype(dtype)
    return ref, ours


def _ref64(ref, x, **kw):
    """Run the oracle in fp64 (its `x.float()` at :174 is bypassed).  Without ``return_attn``
    the unused [B,h,n',n'] product of TransLayer (:47) is skipped: it reaches neither the logits
    nor any gradient, and at N = 32768 it would need 71 GB."""
    from oracle.transmil_ref import TransLayer
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self
    TransLayer.compute_attn = bool(kw.get("return_attn", False))
    try:
        return ref(x.double(), **kw)
    finally:
        torch.Tensor.float = orig
        TransLayer.compute_attn = True


def _ref_forward_backward(ref, x, label, ncls):
    logits = _ref64(ref, x)
    y = torch.tensor([label] * x.shape[0])
    loss = torch.nn.CrossEntropyLoss()(logits, torch.nn.functional.one_hot(y, ncls).double())
    loss.backward()
    return logits.detach(), {n: p.grad.detach() for n, p in ref.named_parameters()}


def _ours_forward_backward(ours, x, label, ncls):
    logits = ours(x.float().to(DEV))
    y = torch.tensor([label] * x.shape[0], device=DEV)
    loss = torch.nn.CrossEntropyLoss()(logits, torch.nn.functional.one_hot(y, ncls).float())
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().cpu(), {n: p.grad.detach().cpu() for n, p in ours.named_parameters()}


@pytest.mark.parametrize("N,B,ncls", [(1, 1, 2), (2, 1, 2), (3, 1, 2), (100, 1, 2), (1000, 1, 2),
                                      (257, 1, 3), (300, 2, 2), (4000, 1, 3), (8192, 1, 2)])
def test_transmil_fp32_logits_and_grads(N, B, ncls):
    ref, ours = _pair(ncls)
    x = torch.from_numpy(bag_input(N, 512, 77 + N, B))
    lr, gr = _ref_forward_backward(ref, x, 1, ncls)
    lo, go = _ours_forward_backward(ours, x, 1, ncls)
    np.testing.assert_allclose(lo.numpy(), lr.numpy(), rtol=0, atol=1e-4)
    assert torch.equal(lo.argmax(1), lr.argmax(1))
    bad = []
    for name, g in gr.items():
        err = ((go[name].double() - g).abs().max() / g.abs().max().clamp_min(1e-12)).item()
        if err > 2e-3:
            bad.append((name, err))
    assert not bad, bad


@pytest.mark.parametrize("name,N", [("d512_n1024", 1024), ("d512_n8192", 8192)])
def test_golden_d512_logits(name, N):
    """Logits of the reference itself (fixture) at d=512, fp32 parity mode."""
    fx = load(name)
    _, ours = _pair(2)
    x = torch.from_numpy(bag_input(N, 512, 2021 + 1000 + N)).to(DEV)
    with torch.no_grad():
        lo = ours(x).cpu().numpy()
    np.testing.assert_allclose(lo, fx["logits"], rtol=0, atol=1e-4)
    assert (lo.argmax(1) == fx["logits"].argmax(1)).all()


@pytest.mark.parametrize("dtype,atol", [(torch.float32, 1e-4), (torch.bfloat16, 5e-2)])
def test_golden_long_sequence_c3(dtype, atol):
    """Config C3 (SURVEY.md section 8 d): 3-class, N = 32768 (n' = 33280, l = 130) against
    the oracle-generated fixture (tests/golden/make_golden_long.py); fp32 within 1e-4, bf16
    within 5e-2, argmax equal.  The train-mode backward at this size is checked against the
    fp64 oracle in test_train_mode_dropout_matches_oracle_with_same_mask."""
    fx = load("d512c3_n32768")
    _, ours = _pair(3, dtype=dtype)
    N = 32768
    x = torch.from_numpy(bag_input(N, 512, 2021 + 1000 + N)).to(DEV)
    with torch.no_grad():
        lo = ours(x).cpu().numpy()
    np.testing.assert_allclose(lo, fx["logits.f64"], rtol=0, atol=atol)
    assert (lo.argmax(1) == fx["logits"].argmax(1)).all()


@pytest.mark.parametrize("name", ["d512_b4_n300", "d512_peaky_n1024", "d512c3_ref_n32768"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_golden_reference_d512_round2(name, dtype):
    """Logits of the reference's own code/models/TransMIL.py at the bench width
    (tests/golden/make_golden_r2.py): B = 4 bags in one forward (the pseudo-inverse's global max
    couples them), sharpened attention (q x 8), and config C3 (N = 32768, 3-class).  fp32 parity
    mode: within 1e-4, argmax bit-exact.  bf16 bench mode: within 5e-2, argmax equal on every bag
    whose fp64 top-2 margin exceeds 0.05."""
    from golden_util import index
    meta = index()[name]
    fx = load(name)
    ncls, n, batch = meta["n_classes"], meta["n"], meta["batch"]
    ref, ours = _pair(ncls, dtype=dtype)
    if "peaky" in name:
        with torch.no_grad():
            for layer in (ours.layer1, ours.layer2):
                w = layer.attn.to_qkv.weight
                w[: w.shape[0] // 3] *= 8.0
    x = torch.from_numpy(bag_input(n, 512, 2021 + 1000 + n, batch)).to(DEV)
    with torch.no_grad():
        lo = ours(x).cpu().numpy()
    ref64 = fx["logits.f64"]
    if dtype == torch.float32:
        np.testing.assert_allclose(lo, ref64, rtol=0, atol=1e-4)
        assert (lo.argmax(1) == fx["logits"].argmax(1)).all()
    else:
        np.testing.assert_allclose(lo, ref64, rtol=0, atol=5e-2)
        top2 = np.sort(ref64, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 0.05
        assert clear.any()
        assert (lo.argmax(1)[clear] == ref64.argmax(1)[clear]).all()


# (N, model seed): fp64 oracle margins |logit1 - logit0| of 0.17 (2021: class 0), 0.25-0.26 (3002: class 0),
# 0.29-0.37 (3004: class 1) at N = 1024 / 8192 on bag_input(N, 512, 5 + N) -- each at least 3x the 5e-2
# logit tolerance, both classes represented
@pytest.mark.parametrize("N", [1024, 8192])
@pytest.mark.parametrize("seed", [2021, 3002, 3004])
def test_bf16_mode_close_to_oracle(N, seed):
    """The timed path's arithmetic (bf16 mode, eval) against the fp64 oracle at C1 / C2 sizes: logits
    within 5e-2 and the class argmax equal, asserted unconditionally on bags whose oracle margin is
    clear (checked first: a seed whose margin shrank below 0.15 fails here, it is not skipped)."""
    ref, ours = _pair(2, dtype=torch.bfloat16, seed=seed)
    x = torch.from_numpy(bag_input(N, 512, 5 + N))
    with torch.no_grad():
        lr = _ref64(ref, x)
        lo = ours(x.to(DEV)).cpu()
    lr_np = lr.numpy()
    top2 = np.sort(lr_np, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 0.15, lr_np       # the bag's construction, not a skip
    np.testing.assert_allclose(lo.numpy(), lr_np, rtol=0, atol=5e-2)
    assert (lo.numpy().argmax(1) == lr_np.argmax(1)).all()


@pytest.mark.parametrize("N,B,ncls", [(1, 1, 2), (2, 1, 2), (3, 1, 2), (255, 1, 2), (256, 1, 3), (257, 1, 2),
                                      (300, 2, 2), (1000, 1, 2), (4000, 1, 2)])
def test_bf16_mode_grads_close_to_oracle(N, B, ncls):
    """Bench-mode (bf16 operands) gradients against the fp64 oracle: every parameter's
    gradient within 6e-2 of its max magnitude (bf16 operands carry ~3 significant digits).
    Ragged and tiny bags (n' = 256: one landmark segment of l = 1; S = 256 / 257 around the pad
    boundary) and B = 2 bags through the bf16 kernels' split / clamp paths."""
    ref, ours = _pair(ncls, dtype=torch.bfloat16)
    x = torch.from_numpy(bag_input(N, 512, 99 + N, B))
    lr, gr = _ref_forward_backward(ref, x, 1, ncls)
    lo, go = _ours_forward_backward(ours, x, 1, ncls)
    np.testing.assert_allclose(lo.numpy(), lr.numpy(), rtol=0, atol=5e-2)
    bad = []
    for name, g in gr.items():
        err = ((go[name].double() - g).abs().max() / g.abs().max().clamp_min(1e-12)).item()
        if err > 6e-2:
            bad.append((name, err))
    assert not bad, bad


def test_return_attn_contract():
    """(logits, (attn [B,8,n',n'], padding)) with the class token at row `padding` (:209-210)."""
    ref, ours = _pair(2)
    x = torch.from_numpy(bag_input(200, 512, 9))
    with torch.no_grad():
        lr, (ar, pr) = _ref64(ref, x, return_attn=True)
        lo, (ao, po) = ours(x.to(DEV), return_attn=True)
    assert po == pr and ao.shape == ar.shape
    H = 200
    row_r = ar[0, :, pr + 1, pr + 1:pr + 1 + H]
    row_o = ao[0, :, po + 1, po + 1:po + 1 + H].cpu().double()
    assert ((row_o - row_r).abs().max() / row_r.abs().max()).item() < 1e-3


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("N,B", [(200, 1), (1000, 2)])
def test_attention_map_rows_match_the_full_product(dtype, tol, N, B):
    """SURVEY.md section 8 f rank 1: return_attn rows through tm_nys_attn_row (no n x n
    matrix) against the materialised attn1 Z attn3 of the same factors, for the consumers'
    row (padding + 1), the class-token row, the last row (negative index) and bag 1."""
    from transmil_deepgraft_amd.nystrom_attention import AttentionMap
    _, ours = _pair(2, dtype=dtype)
    x = torch.from_numpy(bag_input(N, 512, 31 + N, B)).to(DEV)
    with torch.no_grad():
        _, (attn, pad) = ours(x, return_attn=True)
    assert isinstance(attn, AttentionMap)
    n = attn.shape[-1]
    assert attn.shape == (B, 8, n, n) and (n - pad) % 1 == 0
    rows = [(0, pad + 1), (0, pad), (B - 1, -1), (B - 1, n // 2)]
    got = [attn[b, :, r, pad + 1:pad + 1 + N].clone() for b, r in rows]
    full = attn.full()
    for (b, r), g in zip(rows, got):
        ref = full[b, :, r, pad + 1:pad + 1 + N]
        assert g.shape == ref.shape
        assert ((g - ref).abs().max() / ref.abs().max()).item() < tol, (b, r)
    # after materialisation every index goes through the full tensor
    assert torch.equal(attn[0, :, pad + 1], full[0, :, pad + 1])


def test_nystrom_module_return_attn_is_an_attention_map():
    from transmil_deepgraft_amd.nystrom_attention import NystromAttention, AttentionMap
    torch.manual_seed(3)
    m = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6,
                         residual=True, dropout=0.7).to(DEV).eval()
    x = torch.randn(1, 300, 512, device=DEV)
    with torch.no_grad():
        out, attn = m(x, return_attn=True)
    assert isinstance(attn, AttentionMap) and attn.shape == (1, 8, 512, 512)
    r = attn[0, :, 300, :]
    full = attn.full()[0, :, 300, :]
    assert ((r - full).abs().max() / full.abs().max()).item() < 1e-5
    assert attn.sum().item() == attn.full().sum().item()  # tensor methods forward to the full product


def _hook_norms(model, acts, grads):
    def fwd_hook(name):
        def h(_m, _inp, out):
            acts[name] = out.detach().cpu().double()
            out.register_hook(lambda g: grads.__setitem__(name, g.detach().cpu().double()))
        return h
    return [model.norm.register_forward_hook(fwd_hook("norm")),
            model.layer1.norm.register_forward_hook(fwd_hook("layer1.norm")),
            model.layer2.norm.register_forward_hook(fwd_hook("layer2.norm"))]


def test_norm_hooks_fire_and_match_the_oracle():
    """GradCAM hooks model.norm / layer{1,2}.norm (code/visualize_mil.py:225-234): with a
    hook registered the model runs module by module on the HIP ops; the hooked activations
    and the gradients flowing into them match the oracle's (fp32 parity mode), and logits
    and parameter gradients match the fused path."""
    ref, ours = _pair(2)
    x = torch.from_numpy(bag_input(300, 512, 41))
    lf, gf = _ours_forward_backward(ours, x, 1, 2)          # fused path, no hooks
    ours.zero_grad(set_to_none=True)
    acts, grads, racts, rgrads = {}, {}, {}, {}
    handles = _hook_norms(ours, acts, grads)
    try:
        assert ours._hooked()
        lh, gh = _ours_forward_backward(ours, x, 1, 2)
    finally:
        for hd in handles:
            hd.remove()
    assert not ours._hooked()
    rh = _hook_norms(ref, racts, rgrads)
    try:
        _ref_forward_backward(ref, x, 1, 2)
    finally:
        for hd in rh:
            hd.remove()
    np.testing.assert_allclose(lh.numpy(), lf.numpy(), rtol=0, atol=1e-5)
    for name in gf:
        assert ((gh[name].double() - gf[name].double()).abs().max()
                / gf[name].double().abs().max().clamp_min(1e-12)).item() < 2e-3, name
    for name in ("norm", "layer1.norm", "layer2.norm"):
        assert acts[name].shape == racts[name].shape == (1, 18 * 18 + 1, 512), name
        assert (acts[name] - racts[name]).abs().max().item() < 1e-4, name
        assert ((grads[name] - rgrads[name]).abs().max() / rgrads[name].abs().max()).item() < 2e-3, name


def test_train_mode_dropout_is_applied_and_reproducible():
    """The mask stream is a device-side counter (hipGraph-safe): restoring the
    counter reproduces the mask; every forward advances it; eval mode has none."""
    _, ours = _pair(2)
    ours.train()
    x = torch.from_numpy(bag_input(500, 512, 3)).to(DEV)
    start = ours._dropout_counter.clone()
    a = ours(x).detach()
    c = ours(x).detach()
    ours._dropout_counter.copy_(start)
    b = ours(x).detach()
    ours.eval()
    with torch.no_grad():
        e = ours(x)
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and not torch.equal(a, e)


@pytest.mark.parametrize("N,ncls,dtype,ltol,gtol", [
    (300, 2, torch.float32, 1e-4, 2e-3),
    (8192, 2, torch.float32, 1e-4, 2e-3),      # config C2's shape in the fp32 parity mode
    (8192, 2, torch.bfloat16, 5e-2, 6e-2),     # config C2 exactly as bench.py times it
    (32768, 3, torch.bfloat16, 5e-2, 6e-2),    # config C3
])
def test_train_mode_dropout_matches_oracle_with_same_mask(N, ncls, dtype, ltol, gtol):
    """Train mode (dropout 0.7 on to_out), the step the reference trains with
    (code/models/model_interface.py:333-349 -> code/models/TransMIL.py:167-211): the mask the
    kernels draw is replayed into the fp64 oracle through the host restatement of the kernel
    hash, then logits and EVERY parameter gradient are compared (relative to each tensor's
    largest entry).  fp32 parity mode: logits 1e-4, gradients 2e-3.  bf16 bench mode (the
    configuration bench.py times, N = 8192; and config C3, N = 32768, 3-class): logits 5e-2,
    gradients 6e-2 (bf16 operands carry ~3 significant digits)."""
    import math
    from transmil_deepgraft_amd.engine import TransMILEngine
    ref, ours = _pair(ncls, dtype=dtype)
    ours.train()
    B = 1
    G = math.ceil(math.sqrt(N))
    S = G * G + 1
    npad = (S + 255) // 256 * 256
    pad = npad - S
    seed_val = int(ours._dropout_counter.item()) + 1
    layer_seeds = TransMILEngine.forward.__defaults__[1]
    x = torch.from_numpy(bag_input(N, 512, 21 + N, B))
    label = ncls - 1
    lo, go = _ours_forward_backward(ours, x, label, ncls)
    hooks = []
    for li, layer in ((0, ref.layer1), (1, ref.layer2)):
        keep = dropout_keep(seed_val, layer_seeds[li], B * S, 512, 0.7).reshape(B, S, 512)
        m = torch.from_numpy(keep.astype(np.float64) / 0.3)

        def hook(_mod, _inp, out, m=m):
            out = out.clone()
            out[:, pad:, :] = out[:, pad:, :] * m
            return out
        hooks.append(layer.attn.to_out[0].register_forward_hook(hook))
    try:
        lr, gr = _ref_forward_backward(ref, x, label, ncls)
    finally:
        for h in hooks:
            h.remove()
    np.testing.assert_allclose(lo.numpy(), lr.numpy(), rtol=0, atol=ltol)
    bad = []
    for name, g in gr.items():
        err = ((go[name].double() - g).abs().max() / g.abs().max().clamp_min(1e-12)).item()
        if err > gtol:
            bad.append((name, err))
    assert not bad, bad


def _branch_pair(name, dtype):
    """(oracle fp64, ours) for the in_features=2048 TransMIL branch or MDMIL with the
    deterministic weights of tests/golden/make_golden_branches.py."""
    from golden_util import index
    from oracle.transmil_ref import TransMIL as Ref, deterministic_params_
    from oracle.mdmil_ref import MDMIL as RefMD
    from transmil_deepgraft_amd.models import TransMIL, MDMIL
    meta = index()[name]
    torch.manual_seed(0)
    if meta["model"] == "MDMIL":
        ref, ours = RefMD(2), MDMIL(2)
    else:
        ref, ours = Ref(2, meta["feat"], 512), TransMIL(2, meta["feat"], 512)
    deterministic_params_(ref, 2021)
    ref = ref.double().eval()
    ours = ours.to(DEV).eval()
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.set_compute_dtype(dtype)
    x = torch.from_numpy(bag_input(meta["n"], meta["feat"], 2021 + 1000 + meta["n"]))
    return ref, ours, x, meta


def _logits_of(out):
    return out[0] if isinstance(out, tuple) else out


@pytest.mark.parametrize("hooked", [False, True])
@pytest.mark.parametrize("name", ["fc2048_n300", "mdmil_n300"])
def test_branch_models_fp32_logits_and_grads(name, hooked):
    """TransMIL(in_features=2048) (RCC _fc1: Linear+GELU+LayerNorm(1024)+Linear+GELU,
    code/models/TransMIL.py:100-111) and MDMIL (code/models/MDMIL.py:60-114) on the fused
    engine (and, ``hooked``, on the module-by-module path a hook on ``model.norm`` selects):
    fp32 logits within 1e-4 of the reference's fp64 fixture, the small gradients against the
    fixture and every gradient within 2e-3 (relative max) of the fp64 oracle."""
    fx = load(name)
    ref, ours, x, meta = _branch_pair(name, torch.float32)
    handle = ours.norm.register_forward_hook(lambda m, i, o: None) if hooked else None
    out = ours(x.float().to(DEV))
    if name.startswith("mdmil"):
        assert isinstance(out, tuple) and len(out) == 2      # (logits, attn2), MDMIL.py:114
    lo = _logits_of(out)
    loss = torch.nn.CrossEntropyLoss()(lo, torch.nn.functional.one_hot(
        torch.tensor([meta["label"]], device=DEV), 2).float())
    loss.backward()
    torch.cuda.synchronize()
    if handle is not None:
        handle.remove()
    np.testing.assert_allclose(lo.detach().cpu().numpy(), fx["logits.f64"], rtol=0, atol=1e-4)
    assert (lo.detach().cpu().numpy().argmax(1) == fx["logits"].argmax(1)).all()
    go = {n: p.grad.detach().cpu().double() for n, p in ours.named_parameters()}
    for k in fx:
        if k.startswith("grad.") and k.endswith(".f64"):
            g = torch.from_numpy(fx[k])
            err = ((go[k[5:-4]] - g).abs().max() / g.abs().max().clamp_min(1e-12)).item()
            assert err < 2e-3, (k, err)
    lr = _logits_of(_ref64(ref, x))
    torch.nn.CrossEntropyLoss()(lr, torch.nn.functional.one_hot(torch.tensor([meta["label"]]), 2).double()).backward()
    bad = []
    for n, p in ref.named_parameters():
        err = ((go[n] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-12)).item()
        if err > 2e-3:
            bad.append((n, err))
    assert not bad, bad


@pytest.mark.parametrize("name", ["fc2048_n300", "mdmil_n300"])
def test_branch_models_bf16_close_to_reference(name):
    """bf16 (bench) mode of the same two models: logits within 5e-2 of the reference fixture,
    one train-mode backward with every gradient finite and nonzero."""
    fx = load(name)
    _, ours, x, meta = _branch_pair(name, torch.bfloat16)
    with torch.no_grad():
        lo = _logits_of(ours(x.to(DEV))).cpu().numpy()
    np.testing.assert_allclose(lo, fx["logits.f64"], rtol=0, atol=5e-2)
    ours.train()
    loss = torch.nn.CrossEntropyLoss()(_logits_of(ours(x.to(DEV))), torch.nn.functional.one_hot(
        torch.tensor([1], device=DEV), 2).float())
    loss.backward()
    for n, p in ours.named_parameters():
        assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("train", [False, True])
def test_last_layer_class_row_path_equals_dense(dtype, tol, train, monkeypatch):
    """Layer 2 on the class rows only (clsrow.hip: A1 row + conv33, to_out, and their backward)
    against the same engine running layer 2 dense: logits and every parameter gradient, B = 2,
    eval and train mode (same dropout seed)."""
    from transmil_deepgraft_amd import engine as E
    _, ours = _pair(2, dtype=dtype)
    if train:
        ours.train()
    x = torch.from_numpy(bag_input(1000, 512, 5, 2))
    c0 = ours._dropout_counter.clone()
    outs = []
    for cls_only in (True, False):
        monkeypatch.setattr(E.TransMILEngine.__init__, "__defaults__", (torch.bfloat16, None, "_fc", cls_only))
        ours._dropout_counter.copy_(c0)
        ours.zero_grad(set_to_none=True)
        outs.append(_ours_forward_backward(ours, x, 1, 2))
    (lc, gc), (ld, gd) = outs
    assert ((lc - ld).abs().max() / ld.abs().max()).item() < tol
    bad = []
    for name, g in gd.items():
        err = ((gc[name].double() - g.double()).abs().max() / g.double().abs().max().clamp_min(1e-12)).item()
        if err > tol:
            bad.append((name, err))
    assert not bad, bad


@pytest.mark.parametrize("N,B", [(8192, 1), (1000, 2)])
def test_class_row_q_products_equal_dense_q_block(N, B, monkeypatch):
    """bf16 class-row layer 2: the q part of to_qkv's backward as two small products on
    tm_cls_q_rows' operands (dWq = scale Aq^T Xs, dxn += scale Aq Wq by segment in the LayerNorm
    backward; engine.CLS_Q_ROWS) against the dense q block of dqkv through the K = 3D GEMMs:
    logits bitwise (the forward is shared), every parameter gradient within 2e-2 of its largest
    entry (the dense path rounds dq and the q part of dxn to bf16; the products keep fp32)."""
    from transmil_deepgraft_amd import engine as E
    _, ours = _pair(2, dtype=torch.bfloat16)
    ours.train()
    x = torch.from_numpy(bag_input(N, 512, 9 + N, B))
    c0 = ours._dropout_counter.clone()
    outs = []
    for on in (True, False):
        monkeypatch.setattr(E, "CLS_Q_ROWS", on)
        ours._dropout_counter.copy_(c0)
        ours.zero_grad(set_to_none=True)
        outs.append(_ours_forward_backward(ours, x, 1, 2))
    (lq, gq), (ld, gd) = outs
    assert torch.equal(lq, ld)
    bad = []
    for name, g in gd.items():
        err = ((gq[name].double() - g.double()).abs().max() / g.double().abs().max().clamp_min(1e-12)).item()
        if err > 2e-2:
            bad.append((name, err))
    assert not bad, bad
