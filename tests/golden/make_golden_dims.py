"""Golden logits for the TransMIL widths other than 512, from the REFERENCE.

Run once where the reference checkout that ``make_golden_branches.load_ref`` reads exists:
python tests/golden/make_golden_dims.py

  * ``dims256_fc2048_n300``: ``code/models/TransMIL.py`` TransMIL(2, in_features=2048,
    out_features=256): dim_head 32, 128 landmarks (DeepGraft/TransMIL_feat_norm_rest-gloms.yaml),
    N = 300, B = 1;
  * ``dims384_c3_n300_b2``: TransMIL(3, in_features=2048, out_features=384): dim_head 48, 192
    landmarks (DeepGraft/TransMIL_feat_norm_rej_rest.yaml), N = 300, B = 2.

Both import the reference file by path with ``sys.modules['nystrom_attention']`` = the restated
package (``oracle/nystrom_ref.py``) and ``.cuda()`` neutralised, exactly as
``make_golden_branches.py`` does.  Weights come from
``oracle.transmil_ref.deterministic_params_`` (seed 2021) and the bags from
``bag_input(n, F, 2021 + 1000 + n, batch)``, so a fixture holds only the expected outputs: logits
(fp32 and fp64), the CE loss (label 1 for every bag) and the gradients of the small parameters
(class token, the final norm, the head), eval mode -- and its own case metadata (``meta``, a JSON
string), so ``index.json`` is not touched.
"""
from __future__ import annotations

import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from oracle.transmil_ref import deterministic_params_  # noqa: E402
from make_golden import bag_input, cuda_noop  # noqa: E402
from make_golden_branches import load_ref, SMALL_GRADS  # noqa: E402

CASES = {
    "dims256_fc2048_n300": dict(n_classes=2, feat=2048, out=256, n=300, batch=1),
    "dims384_c3_n300_b2": dict(n_classes=3, feat=2048, out=384, n=300, batch=2),
}


def run(tm, n_classes, feat, out, n, batch, label=1, head="_fc"):
    payload = {}
    for dt, tag in ((torch.float32, ""), (torch.float64, ".f64")):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(open(os.devnull, "w")):
            model = tm.TransMIL(n_classes=n_classes, in_features=feat, out_features=out)
        deterministic_params_(model, 2021)
        model = model.to(dt).eval()
        x = torch.from_numpy(bag_input(n, feat, 2021 + 1000 + n, batch)).to(dt)
        with cuda_noop(dt == torch.float64):
            res = model(x)
            logits = res[0] if isinstance(res, tuple) else res
            target = torch.nn.functional.one_hot(torch.full((batch,), label), n_classes).to(dt)
            loss = torch.nn.CrossEntropyLoss()(logits, target)
            loss.backward()
        payload["logits" + tag] = logits.detach().numpy()
        payload["loss" + tag] = loss.detach().numpy().reshape(1)
        for pname, p in model.named_parameters():
            if pname in SMALL_GRADS or pname.startswith(head + "."):
                payload["grad." + pname + tag] = p.grad.detach().numpy().copy()
    return payload


def main():
    tm = load_ref("TransMIL.py", "ref_transmil")
    for name, case in CASES.items():
        payload = run(tm, **case)
        meta = dict(case, label=1, head="_fc", model=f"TransMIL(out_features={case['out']})",
                    weights="deterministic_params_(seed=2021)", input="bag_input(n, feat, seed=2021+1000+n, batch)",
                    source="reference import; see make_golden_dims.py")
        payload["meta"] = np.array(json.dumps(meta, sort_keys=True))
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **payload)
    print("wrote", sorted(CASES))


if __name__ == "__main__":
    main()
