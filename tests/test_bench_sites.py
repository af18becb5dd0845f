"""bench.py's GEMM roofline sites against the GEMMs the fused engine actually launches (CPU: every
``_lib`` entry point replaced by a recorder, so the engine's host orchestration runs on CPU tensors
and no kernel executes).  Reference: code/models/TransMIL.py:26-34 (to_qkv / to_out), :128-133
(_fc1); the bench line's ``gemm_roofline`` credits each call site with 2 M N K flops and its
algorithmic bytes, so a site whose shape drifted from the launch would misstate its fraction.

Also the order of the bucket hooks against the launches: with a three-part bucket (world > 1)
part 1 (layer1) is announced after layer1's last parameter-gradient flush and before the _fc1
backward's first launch, part 2 at the end."""
import pytest

import engine_trace


def _run_engine(N, parts):
    """("gemm", site, M, N, K) / ("call", name) / ("ready", i) of one bf16 training step."""
    return engine_trace.run_transmil(N, parts=parts).log


@pytest.mark.parametrize("N", [8192, 1000])
def test_gemm_sites_match_the_engine_launches(N):
    import bench
    import math
    log = _run_engine(N, parts=2)
    G = math.ceil(math.sqrt(N))
    n = (G * G + 1 + 255) // 256 * 256
    launched = {}
    for e in log:
        if e[0] == "gemm" and e[1] in bench.GEMM_SITES:
            launched.setdefault(e[1], []).append(e[2:])
    assert set(launched) == set(bench.GEMM_SITES), set(launched) ^ set(bench.GEMM_SITES)
    for site, (layers, shape, _) in bench.GEMM_SITES.items():
        want = [shape(n, N, layer)[:3] for layer in layers]
        assert launched[site] == want, (site, launched[site], want)
    # layer 2 (the class-row layer) runs the k / v part of to_qkv's backward at K = 2D
    assert launched["dxn_gemm"][0] == (n, 512, 1024)
    assert launched["wgrad_qkv"][0] == (1024, 512, n)


def test_three_part_bucket_announces_layer1_before_the_fc1_backward():
    log = _run_engine(1000, parts=3)
    marks = [(i, e) for i, e in enumerate(log) if e[0] == "ready"]
    assert [e[1] for _, e in marks] == [0, 1, 2]
    i1, i2 = marks[1][0], marks[2][0]
    assert log[i1 - 1] == ("call", "tm_reduce_flush")          # layer1's gradients final
    after = log[i1 + 1:i2]
    assert after[0] == ("call", "tm_fc1_gelu_bwd")             # the _fc1 backward follows part 1
    assert any(e[0] == "gemm" and e[1] == "wgrad_fc1" for e in after)
    assert after[-1] == ("call", "tm_reduce_flush")
    # two parts: no flush between layer1's backward and the _fc1 backward
    log2 = _run_engine(1000, parts=2)
    assert [e[1] for e in log2 if e[0] == "ready"] == [0, 1]
    assert log2.count(("call", "tm_reduce_flush")) == log.count(("call", "tm_reduce_flush")) - 1


def test_grad_bucket_parts_split_layer1():
    from transmil_deepgraft_amd.models import TransMIL
    m = TransMIL(2, 512, 512)
    names = {id(p): n for n, p in m.named_parameters()}
    two, three = m.grad_bucket_parts(), m.grad_bucket_parts(split_layer1=True)
    assert three[0] == two[0]
    assert all(names[id(p)].startswith("layer1.") for p in three[1])
    assert {names[id(p)] for p in three[2]} == {"cls_token", "_fc1.0.weight", "_fc1.0.bias"}
    assert {id(p) for p in three[1] + three[2]} == {id(p) for p in two[1]}
