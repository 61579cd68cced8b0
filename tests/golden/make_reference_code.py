"""Writes tests/golden/reference_code/*.npz: what the reference's own code
(oracle/_ref/libptref.so, built by `make -C oracle` with the reference tree
present) returns for the fixed inputs of tests/reference_code_cases.py.

    python tests/golden/make_reference_code.py

Each file also holds a digest of its inputs; the tests refuse a recording made
for other inputs, and with the library present they require recording ==
library."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import reference_code_cases as C  # noqa: E402
from oracle import reference_code as R  # noqa: E402


def main():
    if not R.available():
        sys.exit(f"{R.LIB_PATH} is not built: run `make -C oracle` with the reference tree present")
    C.RECORD = True
    C.reference_u01()
    for it in C.ITERS:
        C.reference_shade(it)
    for kind in C.SCATTER_KINDS:
        C.reference_scatter(kind)
    C.reference_transforms()
    C.reference_grid()
    for name in list(C.BATCHES) + C.DEGENERATE:
        C.reference_hits(name)
    for case in C.RENDERS:
        C.reference_render(case)
    total = 0
    for f in sorted(os.listdir(C.RECORDINGS)):
        size = os.path.getsize(os.path.join(C.RECORDINGS, f))
        total += size
        print(f"{size:8d}  {f}")
    print(f"{total:8d}  total")


if __name__ == "__main__":
    main()
