"""TransMIL widths other than 512 (out_features 256 / 384: dim_head 32 / 48, 128 / 192 landmarks),
the part that needs no GPU: the module accepts the geometries, the parameter layout equals the
oracle's, forward_ce declines, the tm_nysg_* entry points refuse bad input before any device work,
and the two reference fixtures (tests/golden/make_golden_dims.py) are reproduced by the CPU oracle."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from golden_util import load, bag_input

GEOS = [(32, 128), (48, 192)]


def test_supported_geometries():
    from transmil_deepgraft_amd.nystrom_attention import NystromAttention
    for dim, dh, nl in ((256, 32, 128), (384, 48, 192), (512, 64, 256)):
        NystromAttention(dim=dim, dim_head=dh, heads=8, num_landmarks=nl)._supported(None)
    with pytest.raises(NotImplementedError, match=r"\(64, 256\), \(32, 128\), \(48, 192\)"):
        NystromAttention(dim=320, dim_head=40, heads=8, num_landmarks=160)._supported(None)
    with pytest.raises(NotImplementedError):
        NystromAttention(dim=256, dim_head=32, heads=8, num_landmarks=256)._supported(None)
    with pytest.raises(NotImplementedError, match="mask"):
        NystromAttention(dim=256, dim_head=32, heads=8, num_landmarks=128)._supported(torch.ones(1, 4).bool())


@pytest.mark.parametrize("ncls,feat,out", [(2, 2048, 256), (5, 384, 384), (3, 768, 384)])
def test_state_dict_layout_equals_the_oracle(ncls, feat, out):
    from oracle.transmil_ref import TransMIL as Ref
    from transmil_deepgraft_amd.models import TransMIL
    ref, ours = Ref(ncls, feat, out).state_dict(), TransMIL(ncls, feat, out).state_dict()
    assert list(ours) == list(ref)
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in ref.items()}


@pytest.mark.parametrize("out", [256, 384])
def test_forward_ce_declines_and_no_bucket_is_attached(out):
    """No GPU is touched: the answer depends on the width alone (a CPU bag would raise at 512)."""
    from transmil_deepgraft_amd.models import TransMIL
    m = TransMIL(3, 2048, out)
    assert m.forward_ce(torch.zeros(1, 4, 2048), torch.tensor([1])) is None
    m.attach_grad_bucket(object())
    assert m._grad_bucket is None
    with pytest.raises(RuntimeError, match="GPU tensor"):
        TransMIL(3, 512, 512).forward_ce(torch.zeros(1, 4, 512), torch.tensor([1]))


def _entry_calls(dh, nl, n, nbh=8, p=None):
    """name -> argument tuple of every tm_nysg_* launch entry point at (dh, nl, n); pointers ``p``."""
    f0 = C.c_float(0.0)
    return {
        "tm_nysg_landmarks": (dh, nl, p, p, nbh, n, p, p, None),
        "tm_nysg_a3_fwd": (dh, nl, p, p, p, nbh, n, p, p, p, None),
        "tm_nysg_a1_fwd": (dh, nl, p, p, p, p, p, nbh, 8, n, p, p, None),
        "tm_nysg_conv_bwd": (dh, nl, p, p, p, p, nbh, 8, n, p, p, p, p, None, None),
        "tm_nysg_a1_bwd": (dh, nl, p, p, p, p, p, p, nbh, 8, n, p, p, p, p, None, None),
        "tm_nysg_a3_bwd": (dh, nl, p, p, p, p, p, p, nbh, n, p, p, p, p, None, None),
        "tm_nysg_assemble_dqkv": (dh, nl, 0, p, p, p, p, p, 1, 8, n, f0, p, None),
        "tm_nysg_attn_row": (dh, nl, p, p, p, p, p, p, nbh, n, 0, p, None),
        # no n: these take the geometry and the head count only
        "tm_nysg_sim2_softmax": (dh, nl, p, p, nbh, p, None),
        "tm_nysg_softmax_bwd_rows": (dh, nl, p, p, p, nbh * nl, None),
        "tm_nysg_pinv_fwd": (dh, nl, p, nbh, 6, p, None),
        "tm_nysg_pinv_bwd": (dh, nl, p, nbh, 6, p, p, p, p, None),
        "tm_nysg_mm": (dh, nl, p, 0, p, p, f0, p, nbh, None),
    }


_WITH_N = ("tm_nysg_landmarks", "tm_nysg_a3_fwd", "tm_nysg_a1_fwd", "tm_nysg_conv_bwd", "tm_nysg_a1_bwd",
           "tm_nysg_a3_bwd", "tm_nysg_assemble_dqkv", "tm_nysg_attn_row")


def test_every_entry_point_is_bound():
    from transmil_deepgraft_amd import _lib
    launches = set(_entry_calls(32, 128, 128))
    queries = {n for n in _lib.EXPORTED if n.startswith("tm_nysg_")} - launches
    assert queries == {"tm_nysg_a3_workspace", "tm_nysg_conv_bwd_workspace", "tm_nysg_a1_bwd_workspace",
                       "tm_nysg_a3_bwd_workspace", "tm_nysg_pinv_saved_floats", "tm_nysg_pinv_bwd_workspace_floats"}


@pytest.mark.parametrize("dh,nl", [(64, 256), (40, 160), (32, 192), (48, 128), (0, 0)])
def test_entry_points_refuse_an_unsupported_geometry(dh, nl):
    """Before any device work (no GPU here, null pointers), with the message in tm_last_error."""
    from transmil_deepgraft_amd import _lib
    for name, args in _entry_calls(dh, nl, 2 * max(nl, 1)).items():
        with pytest.raises(RuntimeError, match=r"\(dh, nl\) must be \(32, 128\) or \(48, 192\)"):
            _lib.call(name, *args)
        assert "(32, 128) or (48, 192)" in _lib.last_error(), name
    assert _lib.query("tm_nysg_a3_workspace", dh, nl, 8, 2 * max(nl, 1)) == -1
    assert _lib.query("tm_nysg_conv_bwd_workspace", dh, nl, 1, 8, 2 * max(nl, 1)) == -1
    assert _lib.query("tm_nysg_a1_bwd_workspace", dh, nl, 8, 2 * max(nl, 1)) == -1
    assert _lib.query("tm_nysg_a3_bwd_workspace", dh, nl, 8, 2 * max(nl, 1)) == -1
    assert _lib.query("tm_nysg_pinv_saved_floats", dh, nl, 8, 6) == -1
    assert _lib.query("tm_nysg_pinv_bwd_workspace_floats", dh, nl, 8) == -1


@pytest.mark.parametrize("dh,nl", GEOS)
def test_entry_points_refuse_a_bad_length_and_null_pointers(dh, nl):
    from transmil_deepgraft_amd import _lib
    for n in (0, -nl, nl + 1, 256 if nl == 192 else 192, 100):
        for name in _WITH_N:
            with pytest.raises(RuntimeError, match="n must be a positive multiple of nl"):
                _lib.call(name, *_entry_calls(dh, nl, n)[name])
            assert "multiple of nl" in _lib.last_error(), name
        assert _lib.query("tm_nysg_a3_workspace", dh, nl, 8, n) == -1
    for name, args in _entry_calls(dh, nl, 2 * nl).items():    # a good shape, null pointers
        with pytest.raises(RuntimeError, match="null pointer"):
            _lib.call(name, *args)
        assert name[3:] in _lib.last_error(), name


@pytest.mark.parametrize("dh,nl", GEOS)
def test_workspace_queries(dh, nl):
    from transmil_deepgraft_amd import _lib
    nbh, n = 16, 5 * nl
    assert _lib.query("tm_nysg_a3_workspace", dh, nl, nbh, n) == 5 * nbh * nl * (dh + 2) * 4
    assert _lib.query("tm_nysg_conv_bwd_workspace", dh, nl, 2, 8, n) == 2 * (n // 32) * 8 * 33 * 4
    assert _lib.query("tm_nysg_a1_bwd_workspace", dh, nl, nbh, n) == 2 * 5 * nbh * nl * dh * 4
    assert _lib.query("tm_nysg_a3_bwd_workspace", dh, nl, nbh, n) == 5 * nbh * nl * dh * 4
    assert _lib.query("tm_nysg_pinv_saved_floats", dh, nl, nbh, 6) == 25 * nbh * nl * nl + 2 * nbh * nl + 8
    assert _lib.query("tm_nysg_pinv_bwd_workspace_floats", dh, nl, nbh) == 5 * nbh * nl * nl + 16 * nbh + 16


@pytest.mark.parametrize("name", ["dims256_fc2048_n300", "dims384_c3_n300_b2"])
def test_reference_fixtures_are_reproduced_by_the_oracle(name):
    """The fixtures come from the reference's own code/models/TransMIL.py; the CPU oracle gives the
    same logits: fp32 within 1e-5 of the fixture's fp32 logits, fp64 within 1e-9 of its fp64 ones."""
    from oracle.transmil_ref import TransMIL as Ref, deterministic_params_
    fx = load(name)
    meta = json.loads(str(fx["meta"]))
    n, feat, batch = meta["n"], meta["feat"], meta["batch"]
    assert fx["logits"].shape == fx["logits.f64"].shape == (batch, meta["n_classes"])
    assert fx["logits"].dtype == np.float32 and fx["logits.f64"].dtype == np.float64
    for k in ("cls_token", "norm.weight", "norm.bias", "_fc.weight", "_fc.bias"):
        assert fx["grad." + k].dtype == np.float32 and fx["grad." + k + ".f64"].dtype == np.float64
    x = torch.from_numpy(bag_input(n, feat, 2021 + 1000 + n, batch))
    torch.manual_seed(0)
    ref = deterministic_params_(Ref(meta["n_classes"], feat, meta["out"]), 2021).eval()
    with torch.no_grad():
        l32 = ref(x).numpy()
    np.testing.assert_allclose(l32, fx["logits"], rtol=0, atol=1e-5)
    ref = ref.double()
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            l64 = ref(x.double()).numpy()
    finally:
        torch.Tensor.float = orig
    np.testing.assert_allclose(l64, fx["logits.f64"], rtol=0, atol=1e-9)
