"""CPU: the table of the refusal tests (tests/refusal_cases.py) covers what tests/test_gpu_refusals.py takes it to cover -- every
exported entry point of the families on chunks and score tensors has rows (one added later fails here until it has some, or a
reason in EXCLUDED), in the signature the binding declares, and the rows are what they are named after."""
import collections

import refusal_cases as rc
from xna_basecaller_amd import _lib


def family_exports():
    return {name for name in _lib.EXPORTS if name.startswith(rc.FAMILIES)}


def test_every_exported_entry_point_of_the_families_has_rows():
    exported = family_exports()
    assert len(exported) > 30
    assert not set(rc.EXCLUDED) & set(rc.SIGNATURES) and set(rc.EXCLUDED) <= exported
    assert set(rc.SIGNATURES) == exported - set(rc.EXCLUDED)
    single = collections.Counter(r.fn for r in rc.ROWS[:rc.SINGLE])
    assert set(single) == set(rc.SIGNATURES) and min(single.values()) >= 4, single


def test_signatures_are_the_bindings():
    lib = _lib.load()
    for fn, names in rc.SIGNATURES.items():
        assert len(getattr(lib, fn).argtypes) == 1 + len(names), fn


def test_rows_are_what_they_say():
    seen = set()
    for i, r in enumerate(rc.ROWS):
        assert (r.fn, r.fault) not in seen, r
        seen.add((r.fn, r.fault))
        assert r.ctx in ("bare", "loaded", "both") and r.code in (rc.INVALID, rc.STATE)
        if i < rc.SINGLE:
            assert isinstance(r.message, str) and (len(r.args) <= 1 or r.fault == "no output"), r
        else:
            assert len(r.args) >= 2 and len(r.message) == 2 and r.message[0] != r.message[1], r
    faults = {r.fault for r in rc.ROWS[:rc.SINGLE]}
    # the single faults the table is to hold: both ends of n and T, a null pointer, no output, both alphabet faults, both beam
    # widths, no positions, a short length, a high label, no weights, both slots
    assert {"n=0", "n=%d" % (rc.MAX_BATCH + 1), "T=0", "T=%d" % (rc.T + 1), "null scores", "no output", "alphabet short",
            "alphabet missing", "beam width 0", "beam width 33", "no positions", "short length", "high label", "no weights",
            "slot -1", "slot %d" % rc.SLOTS} <= faults
    # every entry point that takes T or n is refused at both ends of each
    for fn, names in rc.SIGNATURES.items():
        mine = {r.fault for r in rc.ROWS[:rc.SINGLE] if r.fn == fn}
        for name, ends in (("n", (0, rc.MAX_BATCH + 1)), ("T", (0, rc.T + 1))):
            if name in names:
                assert {"%s=%d" % (name, e) for e in ends} <= mine, fn
