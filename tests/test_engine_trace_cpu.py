"""The engine's host orchestration against its golden launch traces (CPU: every way out of
``engine.py`` is a recorder, tests/engine_trace.py).  One forward + backward per case must issue the
same ``_lib`` calls as the trace under tests/golden/engine_trace/, in the same order, with the same
scalars and struct fields, and with every pointer in the same buffer at the same byte offset --
exact equality, floats included: they are host-side constants, not device results."""
import json
import os

import pytest

import engine_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_trace")


def _load(name):
    with open(os.path.join(GOLDEN, f"{name}.json")) as f:
        return json.load(f)


def test_every_case_has_a_golden_file_and_the_reverse():
    have = {f[:-5] for f in os.listdir(GOLDEN) if f.endswith(".json")} - {"entries"}
    assert have == set(engine_trace.CASES), have ^ set(engine_trace.CASES)


@pytest.mark.parametrize("case", sorted(engine_trace.CASES))
def test_trace_matches_golden(case):
    want, entries = _load(case), _load("entries")
    want["trace"] = [entries[i] for i in want["trace"]]
    got = json.loads(json.dumps(engine_trace.record(case)))      # tuples -> lists, as the files hold them
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        if g != w:
            print(f"{case}: first differing entry is #{i}\n  got   {json.dumps(g, sort_keys=True)}\n"
                  f"  want  {json.dumps(w, sort_keys=True)}")
            break
    else:
        if len(got["trace"]) != len(want["trace"]):
            i = min(len(got["trace"]), len(want["trace"]))
            longer, which = (got, "got") if len(got["trace"]) > i else (want, "want")
            print(f"{case}: {len(got['trace'])} entries, golden has {len(want['trace'])}; the first one only in "
                  f"{which} is #{i}: {json.dumps(longer['trace'][i], sort_keys=True)}")
    assert got["trace"] == want["trace"]
    assert got["buffers"] == want["buffers"]


def test_two_runs_give_the_same_trace():
    """Buffer ids follow first appearance, not addresses: a repeat in the same process (other
    addresses, every earlier buffer released) records the same trace."""
    assert engine_trace.record("bf16_n300") == engine_trace.record("bf16_n300")


def test_an_unknown_pointer_is_an_error():
    import ctypes as C
    rec = engine_trace.Tracer()
    with pytest.raises(AssertionError, match="no buffer"):
        rec.call("tm_anything", C.c_void_p(0x1000))
