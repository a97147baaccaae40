#!/usr/bin/env python3
"""Write tests/golden/accumulator_<curve>.json from the pure-Python reference tests/accumulator_ref.py:

    python tools/gen_golden_accumulator.py

Each file: the sha256 of the default Rescue parameters, 10 elems (0 first, r - 1 last, 8 seeded random between), every node of their
accumulator of height 3 level by level, its root, the paths of uids 0, 4 and 9 (sib1, sib2, positions per level from the leaves up), and the
root of the same elems at height 32.  Residues are hex strings."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import accumulator_ref as A  # noqa: E402
import rescue_ref as R  # noqa: E402

HEIGHT, TALL, PATH_UIDS = 3, 32, (0, 4, 9)


def fixture(curve: str) -> dict:
    elems = A.fixture_elems(curve)
    levels = A.acc_nodes(curve, HEIGHT, elems)
    h = lambda xs: [hex(x) for x in xs]
    paths = {}
    for uid in PATH_UIDS:
        sib1, sib2, pos = A.acc_path(levels, uid)
        paths[str(uid)] = {"sib1": h(sib1), "sib2": h(sib2), "positions": pos}
    return {
        "curve": curve,
        "params_sha256": R.params_sha256(curve),
        "elems": h(elems),
        "height": HEIGHT,
        "levels": [h(l) for l in levels],
        "root": hex(levels[-1][0]),
        "paths": paths,
        "tall_height": TALL,
        "tall_root": hex(A.acc_nodes(curve, TALL, elems)[-1][0]),
    }


if __name__ == "__main__":
    for curve in A.CURVES:
        path = os.path.join(ROOT, "tests", "golden", f"accumulator_{curve}.json")
        with open(path, "w") as fh:
            json.dump(fixture(curve), fh, indent=1)
            fh.write("\n")
        print("wrote", path)
