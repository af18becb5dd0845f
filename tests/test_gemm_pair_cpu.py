"""Where the engine opens and closes paired GEMM launches (CPU: every ``_lib`` entry point replaced by
a recorder, so the host orchestration runs on CPU tensors and no kernel executes).  In the bf16 step
the layer backward brackets a weight gradient with the data gradient of the same dY -- to_out and
to_qkv of layer 1 by default, on request also the k / v part of to_qkv of the class-row layer 2 -- and
nothing else; with a probe target set, or in fp32 parity mode, every product stays its own launch."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BEGIN, END, FLUSH = ("call", "tm_gemm_pair_begin"), ("call", "tm_gemm_pair_end"), ("call", "tm_reduce_flush")


class _Probe:
    """Stands in for engine.probe: records the site stack, carries a ``target`` like the real one."""

    def __init__(self, rec, target):
        self.rec, self.target = rec, target

    def __call__(self, name):
        rec = self.rec

        class _Ctx:
            def __enter__(self):
                rec.site.append(name)

            def __exit__(self, *exc):
                rec.site.pop()
                return False
        return _Ctx()


class _Recorder:
    def __init__(self):
        self.site = []
        self.log = []          # ("gemm", site) / ("call", name) / ("ready", i)

    def call(self, name, *args):
        if name == "tm_gemm":
            self.log.append(("gemm", self.site[-1] if self.site else None))
        else:
            self.log.append(("call", name))

    def query(self, name, *args):
        return 1 << 24


def _run_engine(monkeypatch, N, dtype=torch.bfloat16, target=None, parts=2, pair_gemms=None):
    from transmil_deepgraft_amd import engine
    from transmil_deepgraft_amd.models import TransMIL
    rec = _Recorder()

    class _FakeQueue:
        handle = C.c_void_p(0)

        def pending(self):
            return 1

        def flush(self):
            rec.log.append(FLUSH)

        def close(self):
            pass

    monkeypatch.setattr(engine._lib, "call", rec.call)
    monkeypatch.setattr(engine._lib, "query", rec.query)
    monkeypatch.setattr(engine._lib, "lib", lambda: None)
    monkeypatch.setattr(engine, "ReduceQueue", _FakeQueue)
    monkeypatch.setattr(engine, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(engine, "probe", _Probe(rec, target))
    torch.manual_seed(0)
    model = TransMIL(2, 512, 512).train()
    names, params = model._engine_params(model._fc1_layout())
    prm = dict(zip(names, [p.detach() for p in params]))
    eng = engine.TransMILEngine(dtype, fc1=engine.FC1_PLAIN, head="_fc")
    if pair_gemms is not None:
        eng.pair_gemms = pair_gemms
    x = torch.zeros(1, N, 512)
    seed_dev = torch.zeros(1, dtype=torch.int64)
    ce = (torch.zeros(1, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int32))
    logits, ctx = eng.forward(x, prm, 0.7, seed_dev=seed_dev, counter=torch.zeros(1, dtype=torch.int64), ce=ce)
    out = {n: torch.empty_like(p) for n, p in prm.items()}
    eng.backward(None, ctx, prm, out=out, ready=lambda i: rec.log.append(("ready", i)), gloss=torch.ones(()),
                 parts=parts)
    return rec.log


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
def test_begin_end_bracket_exactly_the_pairs(monkeypatch, N, sel):
    """``sel`` None: the shipped default, layer 1's two pairs (the class-row layer's k / v pair
    measured slower than its two launches and is left unpaired); ALL3: every pair the engine can
    bracket, in backward order -- layer 2 (class rows: its to_out backward is no GEMM pair), then
    layer 1."""
    log = _run_engine(monkeypatch, N, pair_gemms=sel)
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
    off = _run_engine(monkeypatch, N, pair_gemms=False)
    assert BEGIN not in off and END not in off
    assert [e for e in log if e not in (BEGIN, END)] == off


def test_no_pair_with_a_probe_target_set(monkeypatch):
    for target in ("wgrad_out", {"dxn_gemm", "fc1_gemm"}):
        log = _run_engine(monkeypatch, 1000, target=target)
        assert BEGIN not in log and END not in log
    assert _run_engine(monkeypatch, 1000).count(BEGIN) == 2
    for target in ("wgrad_out", {"dxn_gemm"}):
        log = _run_engine(monkeypatch, 1000, target=target, pair_gemms=ALL3)
        assert BEGIN not in log and END not in log


def test_no_pair_in_fp32_mode(monkeypatch):
    for sel in (None, ALL3):
        log = _run_engine(monkeypatch, 1000, dtype=torch.float32, pair_gemms=sel)
        assert BEGIN not in log and END not in log
    assert [e for e in log if e[0] == "gemm" and e[1] == "dxn_gemm"]


def test_last_end_precedes_layer1_flush(monkeypatch):
    log = _run_engine(monkeypatch, 1000, parts=3)
    marks = [i for i, e in enumerate(log) if e[0] == "ready"]
    assert [log[i][1] for i in marks] == [0, 1, 2]
    i0, i1 = marks[0], marks[1]
    assert log[i1 - 1] == FLUSH
    layer1 = log[i0 + 1:i1 - 1]                    # layer 1's backward, up to its flush
    assert layer1.count(BEGIN) == 2 and layer1.count(END) == 2
    last_end = max(i for i, e in enumerate(log[:i1]) if e == END)
    assert last_end < i1 - 1
    assert not any(FLUSH in p for p in _brackets(log))     # no flush while a pair is open
