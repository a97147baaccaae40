#!/usr/bin/env python3
"""Write tests/golden/rescue_<curve>.json from the pure-Python reference tests/rescue_ref.py:

    python tools/gen_golden_rescue.py

Each file: the sha256 of the 116 default parameters (32 bytes little-endian each, M row-major then the round keys), 8 input / output state
pairs (all-zero, all r - 1, (1, 0, 0, 0) and 5 seeded random) and the root of the tree over 8 seeded leaves.  Residues are hex strings."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rescue_ref as R  # noqa: E402


def fixture(curve: str) -> dict:
    states, leaves = R.fixture_inputs(curve)
    h = lambda xs: [hex(x) for x in xs]
    return {
        "curve": curve,
        "params_sha256": R.params_sha256(curve),
        "states": [{"in": h(s), "out": h(R.permute(curve, s))} for s in states],
        "leaves": h(leaves),
        "root": hex(R.merkle(curve, leaves)[0]),
    }


if __name__ == "__main__":
    for curve in R.CURVES:
        path = os.path.join(ROOT, "tests", "golden", f"rescue_{curve}.json")
        with open(path, "w") as fh:
            json.dump(fixture(curve), fh, indent=1)
            fh.write("\n")
        print("wrote", path)
