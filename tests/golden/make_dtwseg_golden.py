#!/usr/bin/env python
"""
Fixture generator for the host side of `segment` (xna_basecaller_amd/segment.py): the expected levels of a reference
sequence and the naive breakpoints, as the reference's src/tools/dtw_segmentation.py computes them.

Run in the BUILD container only.  It imports, BY FILE PATH and as reference code, src/tools/dtw_segmentation.py
(get_kmers_model, dtw_segmentation with naive=True -- the path that runs without dtw-python), src/misc/utils.py
(normalize_med_mad_squiggly) and src/misc/data_io.py (load_kmer_poremodel).  Modules those functions never touch (dtw, h5py,
Levenshtein, Bio) are placeholders in sys.modules; data_io.py probes the authors' project directories at import time -- the
probe is answered and the import runs with the reference tree as working directory; nothing is written there.

Stored in tests/golden/dtwseg.json, DATA only:
  * the pore-model rows the chosen targets need (k-mer, level_mean, level_stdv as the reference's loader returns them);
  * targets (CTC labels) with and without X / Y, with a ubs_map, one shorter than k (k = 9), their (means, stdvs) from
    get_kmers_model and their normalised levels from normalize_med_mad_squiggly, drawn one after the other from the GLOBAL
    np.random seeded once with SEED -- what an explicit RandomState(SEED) must reproduce;
  * the reference's own naive breakpoints for a small ctc-data directory.
The generator itself confirms that segment.reference_levels on RandomState(SEED) reproduces the stored levels as float64
(`levels_equal`), or else stores the measured difference for the test to assert.
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REFTREE = "/root/reference"
MODEL = os.path.join(REFTREE, "ub-bonito", "bonito", "data", "r9.4_450bps.nucleotide.6mer.XNA-Px_Ds.template.model")
SEED = 25
BASE_MAP = ["N", "A", "C", "G", "T", "X", "Y"]


def load_reference():
    for name in ("h5py", "Levenshtein", "Bio", "Bio.SeqIO", "Bio.Seq", "Bio.SeqRecord", "Bio.Align", "dtw"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    sys.modules["Bio"].Align = sys.modules["Bio.Align"]
    sys.modules["Bio.Seq"].Seq = object
    sys.modules["Bio.SeqRecord"].SeqRecord = object
    sys.modules["dtw"].dtw = None
    sys.modules["dtw"].StepPattern = None
    sys.path.insert(0, os.path.join(REFTREE, "src"))
    real_exists, cwd = os.path.exists, os.getcwd()
    os.path.exists = lambda q: True if ("GIS" in str(q) or "xna_basecallers" in str(q)) else real_exists(q)
    os.chdir(REFTREE)
    try:
        import misc.data_io as data_io
        import misc.utils as utils
        spec = importlib.util.spec_from_file_location("ref_dtw_segmentation", os.path.join(REFTREE, "src", "tools", "dtw_segmentation.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        os.path.exists = real_exists
        os.chdir(cwd)
    return data_io, utils, tool


def cases():
    rng = np.random.default_rng(11)
    out = []
    for name, length, letters, ubs_map, k in (("natural", 40, [1, 2, 3, 4], None, 6), ("ends_in_A", 25, [1, 2, 3, 4], None, 6),
                                              ("with_xy", 48, [1, 2, 3, 4, 5, 6], None, 6), ("ubs_map", 48, [1, 2, 3, 4, 5, 6], "GT", 6),
                                              ("one_base", 1, [3], None, 6), ("shorter_than_k", 2, [1, 4], None, 9)):
        target = rng.choice(letters, length).astype(np.uint8)
        if name == "ends_in_A":
            target[-1] = 1
        if name in ("with_xy", "ubs_map"):                  # the model knows k-mers with ONE unnatural base
            target[target > 4] = rng.choice([1, 2, 3, 4], int((target > 4).sum()))
            target[10], target[30] = 5, 6
        padded = np.concatenate([target, np.zeros(5, np.uint8)])
        out.append(dict(name=name, target=padded.tolist(), length=length, ubs_map=ubs_map, k=k))
    return out


def main():
    from xna_basecaller_amd import segment as seg
    data_io, utils, tool = load_reference()
    poremodel = data_io.load_kmer_poremodel(MODEL)
    np.random.seed(SEED)
    needed = {}
    cases_ = cases()
    for c in cases_:
        target = np.array(c["target"])[:c["length"]]
        if c["ubs_map"] is not None:                        # segment_read :137-141
            target = target.copy()
            target[target == 5] = BASE_MAP.index(c["ubs_map"][0])
            target[target == 6] = BASE_MAP.index(c["ubs_map"][1])
        s = "".join(BASE_MAP[i] for i in target)
        means, stdvs = tool.get_kmers_model(s, poremodel, k=c["k"])
        levels = utils.normalize_med_mad_squiggly(means, stdvs)
        c.update(means=[float(v) for v in means], stdvs=[float(v) for v in stdvs], levels=[float(v) for v in levels])
        if len(s) + 5 >= c["k"] == 6:
            tail = s + ("ATATA" if s[-1] != "A" else "TATAT")
            for i in range(len(tail) - 5):
                needed[tail[i:i + 6]] = [float(v) for v in poremodel[tail[i:i + 6]]]
    # what this package computes from the same stream
    mine = dict(needed)
    rng = np.random.RandomState(SEED)
    worst = 0.0
    for c in cases_:
        got = seg.reference_levels(np.array(c["target"]), c["length"], {k: tuple(v) for k, v in mine.items()}, ubs_map=c["ubs_map"],
                                   k=c["k"], rng=rng, chunk=c["name"])
        worst = max(worst, float(np.max(np.abs(got - np.array(c["levels"])))) if len(got) else 0.0)
        assert len(got) == len(c["levels"])
    print("max |levels - reference| over the cases: %g" % worst)
    # the reference's naive path on a small directory
    tmp = tempfile.mkdtemp()
    try:
        lengths = np.array([7, 100, 33, 64, 1], np.uint16)
        targets = np.zeros((5, 104), np.uint8)
        for i, n in enumerate(lengths):
            targets[i, :n] = 1 + (np.arange(n) % 4)
        np.save(os.path.join(tmp, "chunks.npy"), np.zeros((5, 1000), np.float32))
        np.save(os.path.join(tmp, "references.npy"), targets)
        np.save(os.path.join(tmp, "reference_lengths.npy"), lengths)
        bkps, success = tool.dtw_segmentation(tmp, naive=True, ref_filepath=MODEL, parallel=False)
        assert np.array_equal(bkps, np.load(os.path.join(tmp, "breakpoints-naive.npy")))
    finally:
        shutil.rmtree(tmp)
    out = {"note": "inputs: pore-model rows of the reference's model file, CTC label targets; outputs: what the reference's "
                   "get_kmers_model / normalize_med_mad_squiggly (global np.random seeded once with `seed`, cases in order) and its "
                   "naive segmentation computed",
           "seed": SEED, "poremodel_rows": [[k] + v for k, v in sorted(needed.items())], "cases": cases_,
           "levels_equal": worst == 0.0, "levels_max_abs_diff": worst,
           "naive": {"chunksize": 1000, "lengths": lengths.tolist(), "width": 104, "dtype": str(bkps.dtype), "breakpoints": bkps.tolist()}}
    with open(os.path.join(HERE, "dtwseg.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote dtwseg.json: %d cases, %d pore-model rows, levels_equal = %s" % (len(cases_), len(needed), worst == 0.0))


if __name__ == "__main__":
    main()
