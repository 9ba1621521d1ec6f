#!/usr/bin/env python
"""Writes the SHA-256 digests tests/test_wino_resident_gpu.py compares against (tests/golden/wino_resident_digests.json).

    python scripts/gen_golden_wino_resident.py [--tree CHECKOUT] [--out FILE]

Run on an MI355X with the library of the commit whose bits are the reference: --tree names a built checkout of that commit
(default: this one).  The cases, their inputs and the calls are the test file's own (run_case); this script only records what
they return.  The committed file was written with --tree at the commit before ResidentFilter / the 16-byte rows of variant 3."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wino_resident_digests.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "cv-ssl-mis_amd"))
    import test_wino_resident_gpu as t
    from mis_hip import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(args.tree)), ops.__file__
    golden = {}
    for cid in list(t.RF_GEOMETRIES) + list(t.V3_CASES):
        golden[cid] = {name: t.digest(v) for name, v in t.run_case(ops, cid).items()}
        print(cid, "ok", flush=True)
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
