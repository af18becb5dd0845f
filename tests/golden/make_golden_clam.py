"""Golden fixtures for CLAM_MB, made by running the REFERENCE model file
``code/models/model_clam.py`` (loaded at run time from ``--reference-root``, never at import time).

Weights come from ``clam_ref.case_params_`` (``deterministic_params_(seed=2021)``), bags from numpy
PCG64 (``clam_ref.case_input``).  Stored per case, data only: the reference's fp32 and fp64 logits and
instance loss, ``idx`` / ``inst_preds`` / ``inst_targets`` ``[K, 2 k_sample]`` (-1 where nothing is
selected), ``gap`` (the smallest fp64 gap between neighbouring scores among the ``k_sample + 1``
extremes of every evaluated class and side), ``err32`` (the reference's own ``max |a_fp32 - a_fp64|``
over the raw scores), the input seed, the state dict's key names and shapes and, for N <= 1000, the
raw scores ``A_raw`` (fp32) / ``A_raw.f64``.

A seed is kept only if ``gap >= 256 err32``, the reference's fp32 and fp64 runs select the same
instances (the indices its ``index_select`` calls receive) and those are the contract's selection of
the fp64 raw scores; otherwise the next seed is tried (from 0, at most 64).  ``index.json`` is not
touched.

    python tests/golden/make_golden_clam.py --reference-root <checkout of the reference>
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for p in (REPO, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

MAX_SEEDS = 64
GAP_FACTOR = 256.0

# name -> (K, N, size, k_sample, subtyping, label)
CASES = {
    "clam_n8": (2, 8, "small", 8, False, 1),                  # N == k: every row selected twice
    "clam_n9": (2, 9, "small", 8, False, 0),
    "clam_n65_c3": (3, 65, "small", 8, False, 2),             # one row past a 64-row block
    "clam_n300": (2, 300, "small", 8, False, 1),
    "clam_n300_big": (2, 300, "big", 8, False, 0),            # D = 384
    "clam_n300_sub_c3": (3, 300, "small", 8, True, 1),
    "clam_n64_k3": (2, 64, "small", 3, True, 0),
    "clam_n1000_c3": (3, 1000, "small", 8, False, 0),
    "clam_n4100_c5": (5, 4100, "small", 8, False, 3),         # more row blocks than a wave, ragged tail
    "clam_n300_peaky": (2, 300, "small", 8, False, 1),        # scores near +-95 (clam_ref.case_params_)
}


def load_reference_class(root):
    path = os.path.join(root, "code", "models", "model_clam.py")
    spec = importlib.util.spec_from_file_location("reference_model_clam", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CLAM_MB


@contextlib.contextmanager
def recorded_index_select():
    """The index arguments of every ``torch.index_select`` call (the reference's selected rows)."""
    seen, orig = [], torch.index_select

    def spy(inp, dim, index, **kw):
        seen.append(index.detach().clone().numpy())
        return orig(inp, dim, index, **kw)

    torch.index_select = spy
    try:
        yield seen
    finally:
        torch.index_select = orig


@contextlib.contextmanager
def fp64_run():
    """The reference builds its logits with ``torch.empty(...).float()``: default dtype fp64 and
    ``.float()`` the identity keep an fp64 run in fp64."""
    orig, default = torch.Tensor.float, torch.get_default_dtype()
    torch.Tensor.float = lambda self, *a, **k: self
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(default)


def run_reference(model, x, label, K, k, subtyping):
    """-> (A_raw, logits, instance_loss, idx [K, 2k], preds [K, 2k]) of one reference run (numpy)."""
    with torch.no_grad(), recorded_index_select() as seen:
        A_raw = model(x, attention_only=True).numpy()
        logits, _, _, _, res = model(x, label=torch.tensor([label]), instance_eval=True)
    idx = np.full((K, 2 * k), -1, dtype=np.int64)
    preds = np.full((K, 2 * k), -1, dtype=np.int64)
    flat, calls = list(res["inst_preds"]), list(seen)
    for c in range(K):
        if c == label:
            idx[c] = np.concatenate([calls.pop(0), calls.pop(0)])
            preds[c], flat = flat[:2 * k], flat[2 * k:]
        elif subtyping:
            idx[c, :k] = calls.pop(0)
            preds[c, :k], flat = flat[:k], flat[k:]
    assert not calls and not flat
    return A_raw, logits.numpy(), float(res["instance_loss"]), idx, preds


def main():
    from clam_ref import case_input, case_params_, extreme_gap, ref_model, select, targets_of
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-root", default=os.environ.get("TRANSMIL_REFERENCE_ROOT"), required=False)
    args = ap.parse_args()
    if not args.reference_root:
        raise SystemExit("give --reference-root (the directory that holds code/models/model_clam.py)")
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    Reference = load_reference_class(args.reference_root)
    for name, case in CASES.items():
        K, N, size, k, subtyping, label = case
        ref32 = case_params_(Reference(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping), name).eval()
        sd = ref32.state_dict()
        ref64 = Reference(size_arg=size, k_sample=k, n_classes=K, subtyping=subtyping).double().eval()
        ref64.load_state_dict({kk: v.double() for kk, v in sd.items()}, strict=True)
        mine = ref_model(name, case)
        assert list(mine.state_dict()) == list(sd)
        assert all(torch.equal(v, sd[kk].double()) for kk, v in mine.state_dict().items())
        for seed in range(MAX_SEEDS):
            x = torch.from_numpy(case_input(N, seed))
            a32, l32, loss32, idx32, preds32 = run_reference(ref32, x, label, K, k, subtyping)
            with fp64_run():
                a64, l64, loss64, idx64, preds64 = run_reference(ref64, x.double(), label, K, k, subtyping)
            gap, err32 = extreme_gap(a64, label, k, subtyping), float(np.abs(a32.astype(np.float64) - a64).max())
            want = select(a64, label, k, subtyping)
            ok = gap >= GAP_FACTOR * err32 and np.array_equal(idx32, idx64) and np.array_equal(idx64, want)
            if ok:
                break
            print(f"  {name}: seed {seed} gap {gap:.3e} err32 {err32:.3e} same idx "
                  f"{np.array_equal(idx32, idx64)} contract idx {np.array_equal(idx64, want)}, next seed", flush=True)
        else:
            raise SystemExit(f"{name}: no seed below {MAX_SEEDS} met the condition")
        assert l64.dtype == np.float64 and np.array_equal(preds32, preds64)
        with torch.no_grad():
            r = mine(x.double(), label, instance_eval=True)
        assert np.abs(r["logits"].numpy() - l64).max() < 1e-12, "restatement != reference (logits)"
        assert abs(float(r["instance_loss"]) - loss64) < 1e-12, "restatement != reference (instance loss)"
        assert np.array_equal(r["idx"], idx64) and np.array_equal(r["inst_preds"], preds64)
        out = {"logits": l32.astype(np.float32), "logits.f64": l64, "instance_loss": np.float32(loss32),
               "instance_loss.f64": np.float64(loss64), "idx": idx64, "inst_preds": preds64,
               "inst_targets": targets_of(idx64, label, k), "gap": np.float64(gap), "err32": np.float64(err32),
               "seed": np.int64(seed), "keys": np.array(list(sd)),
               "shapes": np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])}
        if N <= 1000:
            out.update({"A_raw": a32.astype(np.float32), "A_raw.f64": a64})
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
        print(f"{name}: seed {seed} gap {gap:.3e} err32 {err32:.3e} ratio {gap / err32:.0f} "
              f"logits {l32.reshape(-1).tolist()} loss {loss32:.6f}", flush=True)


if __name__ == "__main__":
    main()
