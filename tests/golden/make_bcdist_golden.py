#!/usr/bin/env python
"""
Fixture generator for xb_barcode_dist's contract (the per-row half of the reference's `analyze_paf.py -d`).

Run in the BUILD container only.  It imports the reference's src/misc/utils.py BY FILE PATH, as make_ubtally_golden.py does --
modules that file imports and no image has (Levenshtein, Bio, misc.data_io) are placeholders in sys.modules -- and calls
`get_barcode_match_score(read_info, read_seq, left_primer, barcode, n_relax_bases)` as reference code on synthetic PAF rows.

The Levenshtein package is in no image.  The placeholder's `distance` is the plain unit-cost dynamic programme written below;
the definition of that distance has no freedom, so the placeholder decides nothing, and the fixture's note says so.

What is stored in tests/golden/bcdist.json is DATA: the templates, the calls, the PAF fields (read_start / read_end on the read
as it was made, as minimap2 and `basecaller --paf` write them), the barcode geometry, and what the reference returned -- the
start, the end, the distance and the detected length.

Cases: both strands; X and Y inside the window on the reverse strand; target_start above and below left_primer; a start
clamped to 0; windows clipped at 0; a window that runs off the read's end; a homopolymer stretch where several windows tie (the
first must win); barcodes of 24 and of 30 letters.  No case makes the reference slice an empty best window (len(None)), and
every call is in upper case: the contract folds a-z of a row to upper case as xb_ub_tally does, the reference compares bytes.
"""
import importlib.util
import json
import os
import sys
import types

import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"

P5 = "GATTACAGGCTTAACGTCTGAGTCC"                # 25 letters: the POC geometry, barcode at 25, 24 letters
BC24 = ["ACGTTGCAAGCTTCGATCCGATAG", "TTGACCGTAGGCTAACGTCAGTCA", "AAAAAAAAAAAAAAAAAAAAAAAA"]
P3 = "CATGNCAAGTTGCATGCCAGTTGAC"                # the UB k-mer and the right primer
Q5 = "GATTACAGGCTTAACGTCTGAGT"                  # 23 letters: the CPLX geometry, barcode at 23, 30 letters
BC30 = ["ACGTTGCAAGCTTCGATCCGATAGCTTGCA", "TTGACCGTAGGCTAACGTCAGTCAGGATCC"]
TEMPLATES = {
    "P0": P5 + BC24[0] + P3, "P1": P5 + BC24[1] + P3, "PH": P5 + BC24[2] + P3,
    "C0": Q5 + BC30[0] + P3, "C1": Q5 + BC30[1] + P3,
    "XB": P5 + "ACGTTGCANGCTTCGATCNGATAG" + P3,  # an unnatural position inside the barcode itself
    "XL": P5 + "ACGTTGCAXGCTTCGATCYGATAG" + P3,  # ... spelled out as the letters a call carries
}
GEOMETRY = {"P0": (25, 24), "P1": (25, 24), "PH": (25, 24), "XB": (25, 24), "XL": (25, 24), "C0": (23, 30), "C1": (23, 30)}


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[len(b)]


def revcomp_call(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def rows():
    """(name, template, call as it was made, strand, q_st on the ALIGNED strand, q_en there, target_start, relax)."""
    t = {k: v.replace("N", "X") for k, v in TEMPLATES.items()}
    out = []

    def add(name, tid, aligned, strand, q_st, r_st, relax=3, q_en=None):
        call = aligned if strand == "+" else revcomp_call(aligned)
        out.append((name, tid, call, strand, q_st, len(aligned) if q_en is None else q_en, r_st, relax))

    add("exact_plus", "P0", t["P0"], "+", 0, 0)
    add("exact_minus", "P0", t["P0"], "-", 0, 0)
    add("wrong_barcode", "P1", t["P0"], "+", 0, 0)                              # P0's call scored against P1's barcode
    add("sub_and_del", "P0", t["P0"][:30] + "T" + t["P0"][31:40] + t["P0"][41:], "+", 0, 0)
    add("ins_before", "P0", t["P0"][:10] + "GG" + t["P0"][10:], "+", 0, 0)         # the barcode two letters late: a later window wins
    add("del_before", "P0", t["P0"][:8] + t["P0"][11:], "-", 0, 0)                  # three letters early, reverse strand
    add("shift_past_relax", "P0", t["P0"][:5] + "ACGTA" + t["P0"][5:], "+", 0, 0)  # five late: out of reach of relax 3
    add("xy_in_window_minus", "XB", t["XB"], "-", 0, 0)                            # X in the barcode, called on the reverse strand
    add("xy_swapped_minus", "XB", t["XB"].replace("X", "Y", 1), "-", 0, 0)
    add("y_called_plus", "XB", t["XB"].replace("X", "Y"), "+", 0, 0)
    add("xy_letters_minus", "XL", t["XL"], "-", 0, 0)                              # the reverse strand's Y is this strand's X
    add("xy_letters_swapped_minus", "XL", t["XL"].translate(str.maketrans("XY", "YX")), "-", 0, 0)
    add("xy_letters_plus", "XL", t["XL"], "+", 0, 0)
    add("target_start_below", "P0", "TT" + t["P0"][12:], "+", 2, 12)               # target_start < left_primer, a soft clip of 2
    add("target_start_above", "P0", t["P0"][31:], "+", 0, 31)                      # target_start > left_primer: start clamped to 0
    add("target_start_above_minus", "P0", t["P0"][31:], "-", 0, 31)
    add("target_start_above_inner", "P0", "GGGGGGGG" + t["P0"][31:], "+", 8, 31)    # second branch, not clamped: 8 - 6 = 2
    add("windows_clipped_at_0", "P0", t["P0"][24:], "+", 0, 24)                    # start 1: windows 0 .. 4
    add("start_exactly_0", "P0", t["P0"][25:], "-", 0, 25)
    add("off_the_end", "P0", t["P0"][:40], "+", 0, 0)                              # the barcode cut after 15 letters
    add("off_the_end_minus", "P0", t["P0"][:47], "-", 0, 0)                        # ... after 22
    add("last_window_short", "P0", t["P0"][:51], "+", 0, 0)                        # start 25, window 28 has 23 letters
    add("homopolymer_tie", "PH", P5 + "A" * 34 + P3.replace("N", "X"), "+", 0, 0)  # every window reads 24 A: the first wins
    add("homopolymer_tie_minus", "PH", "A" * 60, "-", 0, 0)
    add("relax_0", "P0", t["P0"][:10] + "G" + t["P0"][10:], "+", 0, 0, relax=0)
    add("relax_5", "P0", t["P0"][:5] + "ACGTA" + t["P0"][5:], "+", 0, 0, relax=5)  # five late, within reach now
    add("len30_exact", "C0", t["C0"], "+", 0, 0)
    add("len30_minus_indel", "C0", t["C0"][:30] + t["C0"][31:45] + "A" + t["C0"][45:], "-", 0, 0)
    add("len30_wrong_barcode", "C1", t["C0"], "+", 0, 0)
    add("len30_off_the_end", "C1", t["C1"][:48], "-", 0, 0)
    return out


def load_reference():
    for name in ("Levenshtein", "Bio", "Bio.Align", "Bio.SeqIO", "misc", "misc.data_io"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["Levenshtein"].distance = levenshtein
    sys.modules["Bio"].Align = sys.modules["Bio.Align"]
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    for name in ("get_read_seq", "index_reads_file", "get_read_qual", "read_multiple_pafs", "read_sam", "read_tsv"):
        setattr(sys.modules["misc.data_io"], name, None)
    spec = importlib.util.spec_from_file_location("misc.utils", os.path.join(REF, "misc", "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    sys.modules["misc.utils"] = utils
    spec.loader.exec_module(utils)
    return utils


def main():
    utils = load_reference()
    cases = []
    for name, tid, call, strand, q_st, q_en, r_st, relax in rows():
        n = len(call)
        # the PAF's read_start / read_end are on the read as it was made
        read_start, read_end = (q_st, q_en) if strand == "+" else (n - q_en, n - q_st)
        info = pd.Series(dict(read_id=name, read_length=n, read_start=read_start, read_end=read_end, strand=strand,
                              target_id=tid, target_start=r_st))
        bc_pos, bc_len = GEOMETRY[tid]
        barcode = TEMPLATES[tid][bc_pos:bc_pos + bc_len]
        got = utils.get_barcode_match_score(info, call, bc_pos, barcode, n_relax_bases=relax)
        cases.append(dict(read_id=name, target_id=tid, call=call, strand=strand, read_start=read_start, read_end=read_end,
                          q_st_aligned=q_st, target_start=r_st, bc_pos=bc_pos, bc_len=bc_len, relax=relax,
                          barcode_start=int(got["barcode_start"]), barcode_end=int(got["barcode_end"]),
                          barcode_distance=int(got["barcode_distance"]), barcode_detected_len=int(got["barcode_detected_len"]),
                          barcode_detected=str(got["barcode_detected"])))
    out = {"note": "what the reference's get_barcode_match_score returned; Levenshtein.distance was a placeholder (the package is "
                   "in no image): the plain unit-cost dynamic programme of make_bcdist_golden.py, a definition without freedom. "
                   "The barcode passed in is the template's letters as they are (an unnatural position is 'N' there, 'X' or 'Y' "
                   "in a call, so it never matches), the call is compared byte for byte",
           "templates": TEMPLATES, "cases": cases}
    with open(os.path.join(HERE, "bcdist.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote bcdist.json: %d cases" % len(cases))
    for c in cases:
        print(c["read_id"], c["strand"], c["target_id"], c["barcode_start"], c["barcode_end"], c["barcode_distance"],
              c["barcode_detected_len"])


if __name__ == "__main__":
    main()
