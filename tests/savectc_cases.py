"""Test infrastructure: seeded reads off a template library for the `--save-ctc` kernel tests.  The mutation rates straddle the
default thresholds (accuracy 0.95, coverage 0.90); they were chosen with tests/map_ref.py and tests/savectc_ref.py on the CPU
(test_savectc_host.py::test_mutated_reads_reach_every_verdict holds them to it) so that every verdict bit and verdict 0 occur."""
import numpy as np

RATES = (0.0, 0.01, 0.03, 0.06, 0.12)          # per-letter error rate: a third substitutions, a third deletions, a third insertions
LETTERS = np.array(list("ACGT"))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def mutated_reads(templates, count, rng):
    """Reads of whole templates or pieces of them (pieces may miss every unnatural position), errors at one of RATES, the
    template's N called X (or Y on the reverse strand's complement, a natural letter now and then), unaligned random flanks
    of 0 to 40 letters (coverage), both strands; now and then an empty row and a row of ambiguous letters only."""
    reads = []
    for k in range(count):
        u = rng.random()
        if u < 0.03:
            reads.append("")
            continue
        if u < 0.06:
            reads.append("N" * int(rng.integers(1, 30)))
            continue
        t = templates[rng.integers(len(templates))]
        if rng.random() < 0.3:
            a = int(rng.integers(0, len(t) - 30))
            t = t[a:a + int(rng.integers(25, len(t) - a + 1))]
        rate = RATES[rng.integers(len(RATES))]
        out = []
        for c in t:
            if c not in "ACGT":
                c = "X" if rng.random() < 0.9 else str(rng.choice(LETTERS))
            v = rng.random()
            if v < rate / 3:
                c = str(rng.choice(LETTERS))
            elif v < 2 * rate / 3:
                c = ""
            elif v < rate:
                c = c + str(rng.choice(LETTERS))
            out.append(c)
        flank = int(rng.choice([0, 0, 3, 10, 40]))
        s = "".join(rng.choice(LETTERS, flank)) + "".join(out) + "".join(rng.choice(LETTERS, int(rng.integers(0, flank + 1))))
        reads.append(revcomp(s) if rng.random() < 0.5 else s)
    return reads
