#!/usr/bin/env python
"""
Fixture generator for `--save-ctc`'s chunking (`read_chunks` / `ReadChunk`, ub-bonito/bonito/fast5.py:131-146,207-219).

Run in the BUILD container only.  It imports the reference's fast5.py BY FILE PATH, as make_sam_golden.py does -- modules that
file imports and no image has (ont_fast5_api) or that read_chunks never touches at call time are placeholders in sys.modules
-- and calls `read_chunks(read, chunksize, overlap)` as reference code on reads whose signal is np.arange(length), so that a
chunk's first and last value ARE its first and last sample index.  What is stored in tests/golden/savectc.json is DATA: per
case the inputs (length, chunksize, overlap) and what the reference returned -- the number of chunks, their ids, the first and
last sample index of each, and the metadata a ReadChunk copies from its read.  Lengths below and equal to the chunksize, with
and without an offset, one and several chunks.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ub-bonito/bonito"

CASES = [(999, 1000, 100), (1000, 1000, 100), (1001, 1000, 100), (1899, 1000, 100), (1900, 1000, 100), (2800, 1000, 100),
         (3333, 1000, 100), (3600, 3600, 500), (6700, 3600, 500), (9999, 3600, 500), (12345, 4000, 400), (400, 200, 0),
         (777, 200, 0), (50, 64, 8)]


def load_reference():
    for name, attrs in (("ont_fast5_api", {}), ("ont_fast5_api.fast5_interface", {"get_fast5_file": None})):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
    spec = importlib.util.spec_from_file_location("ref_bonito_fast5", os.path.join(REF, "fast5.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    rfast5 = load_reference()
    cases = []
    for length, chunksize, overlap in CASES:
        read = types.SimpleNamespace(read_id="read-%d" % length, run_id="runA", filename="batch_0.fast5", mux=3, channel=211,
                                     start=12.5, duration=length / 4000.0, signal=np.arange(length, dtype=np.float32))
        got = list(rfast5.read_chunks(read, chunksize=chunksize, overlap=overlap))
        assert all(len(c.signal) == chunksize for c in got)
        cases.append({"length": length, "chunksize": chunksize, "overlap": overlap, "count": len(got),
                      "ids": [c.read_id for c in got], "first": [int(c.signal[0]) for c in got],
                      "last": [int(c.signal[-1]) for c in got],
                      "meta": [[c.run_id, c.filename, c.mux, c.channel, c.start, c.duration, c.template_start,
                                c.template_duration] for c in got[:1]]})
    out = {"note": "what the reference's read_chunks returned on reads whose signal is np.arange(length): chunk counts, ids, first "
                   "and last sample index of every chunk, and the metadata of the first ReadChunk",
           "read": {"run_id": "runA", "filename": "batch_0.fast5", "mux": 3, "channel": 211, "start": 12.5},
           "cases": cases}
    with open(os.path.join(HERE, "savectc.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote savectc.json: %d cases, %s chunks" % (len(cases), [c["count"] for c in cases]))


if __name__ == "__main__":
    main()
