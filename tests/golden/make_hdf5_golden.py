#!/usr/bin/env python
"""
Fixture generator for the libhdf5 interoperability tests of tests/test_host.py: files written by the REAL libhdf5 (through
ctypes, tests/h5lib.py; HDF5 1.10.6 made the stored ones), so that hdf5_lite meets files its author did not lay out byte by
byte (tests/h5write.py is the same reading of the format specification as hdf5_lite).  libhdf5 is a library of the machine
that runs this script, not of the project: the tests read the stored files and need no libhdf5 themselves.

    python tests/golden/make_hdf5_golden.py          (needs libhdf5: tests/h5lib.py finds it, XB_LIBHDF5 overrides)

Writes tests/golden/libhdf5_{classic,latest}.h5 (chunked + shuffle + deflate and fletcher32 datasets, 1-D and 2-D, contiguous
datasets, scalar / array / fixed- and variable-length string attributes, a group with many links; the classic and the 1.10
"latest" formats), libhdf5_dense.h5 (1.10 dense link storage, which hdf5_lite refuses) and libhdf5_multi_read.fast5 (the
ont_fast5_api multi-read layout of test_host._fast5_records(7)).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_container(path, latest):
    import h5lib
    x = (np.arange(70000) % 3000 - 1500).astype(np.int16)
    z = np.arange(24, dtype=np.int32).reshape(4, 6)
    w = h5lib.Writer(path, latest=latest)
    g = w.group(w.file, "grp")
    # 1.10 format: chunked datasets get data-layout version 4 (fixed-array / extensible-array chunk indexes), which
    # hdf5_lite refuses (no fast5 writer produces it); contiguous datasets and everything else are read
    w.dataset(g, "x", x, chunks=None if latest else 4096, shuffle=True, deflate=4)
    w.dataset(g, "y", np.linspace(0, 1, 11))
    w.dataset(g, "z", z, chunks=None if latest else (2, 3), deflate=1, fletcher32=True)
    if latest:
        w.dataset(g, "v4", x[:5000], chunks=1000, deflate=1)
    w.attr(g, "note", ("vlen", "variable text"))
    w.attr(g, "fixed", "fixed text")
    w.attr(g, "n", np.int64(-3))
    w.attr(g, "f", np.float32(2.5))
    w.attr(g, "arr", np.arange(5, dtype=np.uint16))
    many = w.group(w.file, "many")
    nsub = 60 if not latest else 6          # 1.10 format: more than 8 links switch to dense storage (fractal heap): unsupported
    for i in range(nsub):
        sub = w.group(many, "sub%03d" % i)
        w.attr(sub, "i", np.int32(i))
    w.close()


def write_dense(path):
    import h5lib
    w = h5lib.Writer(path, latest=True)
    for i in range(20):
        w.group(w.file, "g%02d" % i)
    w.close()


def main():
    import h5lib
    from test_host import _fast5_records
    if h5lib.find() is None:
        raise SystemExit("no libhdf5 found (set XB_LIBHDF5 to its path)")
    write_container(os.path.join(HERE, "libhdf5_classic.h5"), latest=False)
    write_container(os.path.join(HERE, "libhdf5_latest.h5"), latest=True)
    write_dense(os.path.join(HERE, "libhdf5_dense.h5"))
    h5lib.write_multi_fast5(os.path.join(HERE, "libhdf5_multi_read.fast5"), _fast5_records(7), vlen_strings=True, chunk=1000,
                            fillers=53)
    print("wrote tests/golden/libhdf5_{classic,latest,dense}.h5, libhdf5_multi_read.fast5 with", h5lib.find())


if __name__ == "__main__":
    main()
