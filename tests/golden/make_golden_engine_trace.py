"""Golden launch traces of the engine's host orchestration (``transmil_deepgraft_amd/engine.py``).

Run on any machine (no GPU, no library needed: every way out of the engine is a recorder):
python tests/golden/make_golden_engine_trace.py

``tests/engine_trace.record(case)`` gives, for one forward + backward, every ``_lib.call`` in order
with the open probe site and every argument (its module docstring has the encoding), every
``_lib.query``, ``ready(i)`` and ``tm_reduce_flush``, and each buffer's dtype and byte size.  The cases
(``tests/engine_trace.CASES``) share most of their entries, so each distinct entry is stored once, one
per line of ``engine_trace/entries.json``, and ``engine_trace/<case>.json`` holds the case's buffers
and its trace as indices into that list.  They were recorded BEFORE the core's orchestration was split
by compute mode, so ``tests/test_engine_trace_cpu.py`` pins that split -- and any later edit of the
host path -- to the same launches, in the same order, with the same arguments, into the same buffers.
Regenerate only when a change is meant to alter what is launched, and say so in that change.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import engine_trace  # noqa: E402

OUT = os.path.join(HERE, "engine_trace")


def main():
    os.makedirs(OUT, exist_ok=True)
    pool = {}       # entry text -> index, in order of first use
    for name in sorted(engine_trace.CASES):
        rec = engine_trace.record(name)
        lines = [json.dumps(e, sort_keys=True, separators=(",", ":")) for e in rec["trace"]]
        rec["trace"] = [pool.setdefault(t, len(pool)) for t in lines]
        with open(os.path.join(OUT, f"{name}.json"), "w") as f:
            f.write(json.dumps(rec, sort_keys=True, separators=(",", ":")) + "\n")
        print(f"{name}: {len(lines)} entries")
    with open(os.path.join(OUT, "entries.json"), "w") as f:
        f.write("[\n" + ",\n".join(pool) + "\n]\n")
    print(f"{len(pool)} distinct entries")


if __name__ == "__main__":
    main()
