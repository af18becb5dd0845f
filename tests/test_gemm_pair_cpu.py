"""Where the engine opens and closes paired GEMM launches (CPU: every ``_lib`` entry point replaced by
a recorder, so the host orchestration runs on CPU tensors and no kernel executes).  In the bf16 step
the layer backward brackets a weight gradient with the data gradient of the same dY -- to_out and
to_qkv of layer 1 by default, on request also the k / v part of to_qkv of the class-row layer 2 -- and
nothing else; with a probe target set, or in fp32 parity mode, every product stays its own launch."""
import pytest
import torch

import engine_trace

BEGIN, END, FLUSH = ("call", "tm_gemm_pair_begin"), ("call", "tm_gemm_pair_end"), ("call", "tm_reduce_flush")


def _run_engine(N, dtype=torch.bfloat16, target=None, parts=2, pair_gemms=None):
    """("gemm", site, ...) / ("call", name) / ("ready", i) of one training step."""
    return engine_trace.run_transmil(N, dtype=dtype, target=target, parts=parts, pair_gemms=pair_gemms).log


def _brackets(log):
    """The entries between each begin and its end; begin / end must alternate."""
    out, cur = [], None
    for e in log:
        if e == BEGIN:
            assert cur is None, "begin inside an open pair"
            cur = []
        elif e == END:
            assert cur is not None, "end without begin"
            out.append(cur)
            cur = None
        elif cur is not None:
            cur.append(e)
    assert cur is None, "a pair left open"
    return out


ALL3 = ("out", "qkv", "kv")


@pytest.mark.parametrize("N", [8192, 1000])
@pytest.mark.parametrize("sel", [ALL3, None])
def test_begin_end_bracket_exactly_the_pairs(N, sel):
    """``sel`` None: the shipped default, layer 1's two pairs (the class-row layer's k / v pair
    measured slower than its two launches and is left unpaired); ALL3: every pair the engine can
    bracket, in backward order -- layer 2 (class rows: its to_out backward is no GEMM pair), then
    layer 1."""
    log = _run_engine(N, pair_gemms=sel)
    pairs = _brackets(log)
    gemms = [[e[1] for e in p if e[0] == "gemm"] for p in pairs]
    layer1 = [["wgrad_out", "dmerged_gemm"], ["wgrad_qkv", "dxn_gemm"]]
    assert gemms == ([["wgrad_qkv", "dxn_gemm"]] if sel else []) + layer1
    if not sel:
        from transmil_deepgraft_amd import engine
        assert engine.PAIR_SITES == ("out", "qkv") and engine.TransMILEngine.pair_gemms is True
        # the unpaired k / v products of layer 2 come before the first bracket
        first = log.index(BEGIN)
        assert [e[1] for e in log[:first] if e[0] == "gemm" and e[1] in ("wgrad_qkv", "dxn_gemm")] == \
            ["wgrad_qkv", "dxn_gemm"]
    # inside a pair nothing else launches: only the weight gradient's deferred slab sums are queued
    for p in pairs:
        others = {e[1] for e in p if e[0] == "call"}
        assert others <= {"tm_splitk_reduce", "tm_splitk_reduce_bf16"}, others
        assert not [e for e in p if e[0] == "ready"]
    # the same products, in the same order, as with pairing off
    off = _run_engine(N, pair_gemms=False)
    assert BEGIN not in off and END not in off
    assert [e for e in log if e not in (BEGIN, END)] == off


def test_no_pair_with_a_probe_target_set():
    for target in ("wgrad_out", {"dxn_gemm", "fc1_gemm"}):
        log = _run_engine(1000, target=target)
        assert BEGIN not in log and END not in log
    assert _run_engine(1000).count(BEGIN) == 2
    for target in ("wgrad_out", {"dxn_gemm"}):
        log = _run_engine(1000, target=target, pair_gemms=ALL3)
        assert BEGIN not in log and END not in log


def test_no_pair_in_fp32_mode():
    for sel in (None, ALL3):
        log = _run_engine(1000, dtype=torch.float32, pair_gemms=sel)
        assert BEGIN not in log and END not in log
    assert [e for e in log if e[0] == "gemm" and e[1] == "dxn_gemm"]


def test_last_end_precedes_layer1_flush():
    log = _run_engine(1000, parts=3)
    marks = [i for i, e in enumerate(log) if e[0] == "ready"]
    assert [log[i][1] for i in marks] == [0, 1, 2]
    i0, i1 = marks[0], marks[1]
    assert log[i1 - 1] == FLUSH
    layer1 = log[i0 + 1:i1 - 1]                    # layer 1's backward, up to its flush
    assert layer1.count(BEGIN) == 2 and layer1.count(END) == 2
    last_end = max(i for i, e in enumerate(log[:i1]) if e == END)
    assert last_end < i1 - 1
    assert not any(FLUSH in p for p in _brackets(log))     # no flush while a pair is open
