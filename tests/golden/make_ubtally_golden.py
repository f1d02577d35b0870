#!/usr/bin/env python
"""
Fixture generator for xb_ub_tally's contract (the per-read half of the reference's `analyze_paf.py -p`).

Run in the BUILD container only.  It imports the reference's src/misc/utils.py BY FILE PATH, as make_savectc_golden.py does --
modules that file imports and no image has (Levenshtein, Bio) are placeholders in sys.modules, and misc.data_io is a
placeholder whose get_read_seq is backed by a dictionary of strings and does what data_io.py:215-223 does (the aligned slice
of the read, reverse-complemented with the reference's own table on strand '-') -- and calls
`compute_error_rate_per_pos_paf(paf_df, None, reads_dict=..., targets=...)` as reference code on a synthetic PAF table.
src/tools/analyze_paf.py is loaded the same way for `compute_read_confusion_matrix` (its Bio.SeqIO, misc.* and XNA_refs
imports are placeholders; sklearn's confusion_matrix and tqdm are the installed ones); where that import fails the fixture
says so ("confusion": null) and the matrix is pinned to the restatement (tests/ubtally_ref.py) alone.

The alignments are tests/map_ref.py's (this package's mapper contract on the CPU) and the cs strings are the product's host
formatter's (aligner.Mapping), so they are what this package writes.  What is stored in tests/golden/ubtally.json is DATA: the
templates, the calls, the PAF fields and what the reference returned -- per read the error vector, n_matches and the UB-area
metrics, per (template, strand) the error-rate vector, and the confusion matrix per read.

Every UB sits at least 6 letters from both ends, where the reference's own code has no end-of-array quirks.  Between them the
cases cover the polish branches (a)-(d), both strands, a template without a UB site, two UBs whose areas overlap, and
alignments with r_st > 0 and r_en < L.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
REF = "/root/reference/src"

import map_ref  # noqa: E402

TEMPLATES = {
    "T1": "GATTACAGGCTTAACGNCTGAGTCCATGCAAGT",                       # one UB at 16
    "T2": "CCATGGTACGATNGCANTTCGAGGCTAAGCTTGACC",                    # two UBs, 12 and 16: their areas overlap
    "T3": "TGCATGCCAGTTGACCATAGGCTAAC",                              # no UB site
}


def revcomp_call(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def calls():
    t1, t2, t3 = TEMPLATES["T1"], TEMPLATES["T2"], TEMPLATES["T3"]
    x1 = t1.replace("N", "X")
    out = [
        ("a_plus", x1),                                               # (a) the UB called X
        ("a_minus", revcomp_call(x1)),
        ("sub_plus", t1.replace("N", "G")),                           # the UB called a natural letter
        ("x_for_two", t1[:15] + "X" + t1[17:]),                       # one X for the UB and the letter before: the mapper's tie
                                                                      # order puts it on the UB, a deletion before: (a)
        ("b_right", t1[:16] + "X" + t1[18:]),                         # (b) the UB deleted, X one late (the arm of (b) that the
                                                                      # mapper's tie order can produce; tests/test_gpu_ubtally.py
                                                                      # builds the left arm by hand)
        ("c_case", t1[:15] + "TX" + t1[18:]),                         # (c) a letter at the UB, X one late, a deletion before
        ("d_case", t1[:15] + "XT" + t1[18:]),                         # (d) X one early, a letter at the UB, a deletion behind
        ("c_case_minus", revcomp_call(t1[:15] + "TX" + t1[18:])),
        ("two_ubs", t2.replace("N", "X")),
        ("two_ubs_minus", revcomp_call(t2.replace("N", "X", 1).replace("N", "A"))),
        ("y_call", t2.replace("N", "Y", 1).replace("N", "X")),
        ("no_ub", t3),
        ("no_ub_errors_minus", revcomp_call(t3[:8] + "A" + t3[9:14] + t3[16:])),
        ("inner_plus", "TTTT" + x1[5:28] + "GGGG"),                   # r_st > 0 and r_en < L, flanks that do not align
        ("inner_minus", revcomp_call("AC" + x1[7:25])),
        ("insertions", x1[:10] + "AC" + x1[10:22] + "G" + x1[22:]),
    ]
    return out


def load_reference():
    for name in ("Levenshtein", "Bio", "Bio.Align", "Bio.SeqIO", "misc"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["Bio"].Align = sys.modules["Bio.Align"]
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    data_io = types.ModuleType("misc.data_io")

    def get_read_seq(read_id, reads_filepath, read_info=None, reads_dict=None):
        seq = str(reads_dict[read_id])
        if read_info is not None:
            assert len(seq) == read_info.read_length
            seq = seq[read_info.read_start:read_info.read_end]
            if read_info.strand in ["-", "R"]:
                seq = sys.modules["misc.utils"].reverse_complement(seq)
        return seq

    data_io.get_read_seq = get_read_seq
    for name in ("index_reads_file", "get_read_qual", "read_multiple_pafs", "read_sam", "read_tsv"):
        setattr(data_io, name, None)
    sys.modules["misc.data_io"] = data_io
    spec = importlib.util.spec_from_file_location("misc.utils", os.path.join(REF, "misc", "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    sys.modules["misc.utils"] = utils
    spec.loader.exec_module(utils)
    tool = None
    try:
        refs = types.ModuleType("misc.xna_refs")
        refs.XNA_refs, refs.EXP_REF_MAP, refs.REF_EXP_MAP, refs.VALID_REFS = None, {}, {}, []
        sys.modules["misc.xna_refs"] = refs
        spec = importlib.util.spec_from_file_location("ref_analyze_paf", os.path.join(REF, "tools", "analyze_paf.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    except Exception as e:  # noqa: BLE001 -- recorded in the fixture
        print("analyze_paf.py did not load: %r" % (e,))
        tool = None
    return utils, tool


def main():
    utils, tool = load_reference()
    names, templates = list(TEMPLATES), list(TEMPLATES.values())
    rows, reads = [], {}
    for read_id, call in calls():
        m = map_ref.map_read(call, templates)
        mp = map_ref.to_mapping(m, names, templates, call)
        assert mp is not None, read_id
        reads[read_id] = call
        rows.append(dict(read_id=read_id, call=call, read_length=len(call), read_start=mp.q_st, read_end=mp.q_en,
                         strand="+" if mp.strand == 1 else "-", target_id=mp.ctg, target_length=mp.ctg_len, target_start=mp.r_st,
                         target_end=mp.r_en, n_matches=mp.mlen, block_length=mp.blen, mapping_quality=mp.mapq, cs=mp.cs,
                         tmpl=int(m["tmpl"]), q_st_aligned=int(m["q_st"]), ops=m["ops"].decode()))
    paf = pd.DataFrame(rows)
    targets = dict(TEMPLATES)
    error_rate, n_matches, metrics = utils.compute_error_rate_per_pos_paf(paf, None, reads_dict=reads, targets=targets)
    ref_info = types.SimpleNamespace(targets=targets)
    keep = ("ub_area_acc", "ub_area_matches", "ub_area_len", "ub_acc", "ub_matches", "ub_len", "ub_area_acc_plus", "non_ub_area_acc",
            "non_ub_area_matches", "non_ub_area_len", "fdr", "fpr", "true_pos", "false_neg", "true_neg", "false_pos")
    cases = []
    for k, row in enumerate(rows):
        info = paf.iloc[k]
        target = targets[row["target_id"]].replace("N", "X")
        errors, matches = utils.compute_errors_paf(info, target, read_seq=data_seq(utils, reads, info), return_target_matches=True)
        case = dict(row)
        case["errors"] = [int(e) for e in errors]
        case["polished"] = "".join(matches)
        case["n_matches"] = float(n_matches[k])
        ubs_detected = int(np.isin(matches, ["X", "Y"]).sum())
        case["ubs_detected"] = ubs_detected
        for key in keep:
            v = metrics[key][k]
            case[key] = None if isinstance(v, float) and np.isnan(v) else (float(v) if isinstance(v, (float, np.floating)) else int(v))
        case["confusion"] = (None if tool is None else
                             np.asarray(tool.compute_read_confusion_matrix(info, ref_info, reads_dict=reads)).astype(int).tolist())
        cases.append(case)
    rates = [{"target_id": t, "strand": s, "error_rate": [float(v) for v in vec]} for (t, s), vec in error_rate.items()]
    out = {"note": "what the reference's compute_error_rate_per_pos_paf / compute_errors_paf / compute_read_confusion_matrix returned "
                   "for calls aligned by tests/map_ref.py; errors are on the read's strand (reversed on '-'), polished is forward",
           "templates": TEMPLATES, "cases": cases, "error_rates": rates, "confusion_labels": ["ATCGXY", "ATCGXY-"]}
    with open(os.path.join(HERE, "ubtally.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote ubtally.json: %d cases; confusion from the reference: %s" % (len(cases), tool is not None))
    for c in cases:
        print(c["read_id"], c["strand"], c["target_id"], c["target_start"], c["target_end"], c["cs"], c["polished"])


def data_seq(utils, reads, info):
    return sys.modules["misc.data_io"].get_read_seq(info.read_id, None, read_info=info, reads_dict=reads)


if __name__ == "__main__":
    main()
