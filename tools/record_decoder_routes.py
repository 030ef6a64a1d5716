#!/usr/bin/env python3
"""Record the decoder routes of the whole sweep of tests/test_decoder_route.py into tests/golden/decoder_routes.json (DESIGN.md
section 24):
    python tools/record_decoder_routes.py --tree PATH --rev REVISION [--out FILE.json]
--tree is a built checkout of the revision to record from; its library is the one asked.  The sweep -- configurations, batches, calls,
levels, flags, capacities -- and the digest are tests/test_decoder_route.py's of THIS checkout.  No GPU needed: one child process per
capacity (INET_CHAIN_CUS).  The file holds, per capacity and per "V Z H chains", the SHA-256 over the 13 integers of every route in sweep
order and their count -- no routes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_decoder_route as TR                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--rev", required=True, help="the revision --tree is a checkout of (recorded in the file)")
    ap.add_argument("--out", default=TR.ROUTES_FIXTURE)
    a = ap.parse_args()
    res = {"revision": a.rev, "BS": list(TR.BS), "capacities": {}}
    for cap in TR.CAPACITIES:
        _, digests = TR.sweep_in_child(cap, tree=a.tree, check=False)
        res["capacities"][str(cap)] = digests
        print(f"{cap} CUs: {sum(n for _, n in digests.values())} routes", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
