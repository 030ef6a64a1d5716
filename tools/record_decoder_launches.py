#!/usr/bin/env python3
"""Record which launches the decoder calls make, forward and backward, and what the forward returns bit for bit, into
tests/golden/decoder_launches.json:
    python tools/record_decoder_launches.py --tree PATH --rev REVISION [--out FILE.json] [--only CASE]
--tree is a built checkout of the revision to record from; it goes first on sys.path, so `inpaintnet_amd` is that checkout's.  The
cases, the inputs and the digest are tests/decoder_launches.py's of THIS checkout.  Every case runs twice: one whose two digests differ
(a call whose products are split over K with atomics) keeps its labels alone, "digest": null.  The file holds labels, digests and the
revision -- no tensors.  --only CASE records that case alone into the existing file, next to the others, with the revision it came from
(a case added later than the rest: case 16)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decoder_launches as DL                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--rev", required=True, help="the revision --tree is a checkout of (recorded in the file)")
    ap.add_argument("--out", default=DL.FIXTURE)
    ap.add_argument("--only", help="record this case alone and keep the file's other cases")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("record_decoder_launches.py records on the GPU; none found")
    sys.path.insert(0, os.path.abspath(a.tree))
    from inpaintnet_amd import ops, synthetic
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(a.tree) + os.sep), ops.__file__
    res = {"revision": a.rev, "device": torch.cuda.get_device_name(0), "cases": {}}
    if a.only:
        assert a.only in dict(DL.CASES), a.only
        with open(a.out) as f:
            res = json.load(f)
    for name, run in DL.cases():
        if a.only and name != a.only:
            continue
        (f1, b1, d1), (f2, b2, d2) = run(ops, synthetic), run(ops, synthetic)
        assert f1 == f2 and b1 == b2, f"{name}: two runs, two lists of launches"
        res["cases"][name] = {"labels": f1, "bwd_labels": b1, "digest": d1 if d1 == d2 else None}
        if a.only:
            res["cases"][name]["revision"] = a.rev
        print(f"{name}: {len(f1)} + {len(b1 or [])} launches{'' if d1 == d2 else ', digests differ: labels only'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
