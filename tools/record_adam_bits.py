#!/usr/bin/env python3
"""Record what the optimizer step computes, bit for bit, into tests/golden/adam_step_bits.json:
    python tools/record_adam_bits.py --tree PATH --rev REVISION [--out FILE.json]
--tree is a built checkout of the revision to record from; it goes first on sys.path, so `inpaintnet_amd` is that checkout's.  The
inputs, forms, sizes and the digest are tests/adam_bits.py's of THIS checkout.  Only ops.adam_step, ops.adam_step_clip, ops.adamw_step
(with eight-word records), ops.grad_sqnorm and ops.pack_decay_mask are called.  While recording, the plain forms are run through
ops.adamw_step as well and must give the same digests: the fixture is then something the one kernel behind every entry point already
reproduces.  The file holds digests, clip_half's max_norm values and the revision -- no tensors."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import adam_bits as AB                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--rev", required=True, help="the revision --tree is a checkout of (recorded in the file)")
    ap.add_argument("--out", default=AB.FIXTURE)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("record_adam_bits.py records on the GPU; none found")
    sys.path.insert(0, os.path.abspath(a.tree))
    from inpaintnet_amd import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(a.tree) + os.sep), ops.__file__
    res = {"revision": a.rev, "device": torch.cuda.get_device_name(0), "inputs": {}, "max_norm_half": {},
           "digests": {f: {} for f in AB.FORMS}}
    for n in AB.SIZES:
        res["inputs"][str(n)] = AB.inputs_digest(n)
        halves = [AB.half_norm(n, *c) for c in AB.combos(n)]
        res["max_norm_half"][str(n)] = halves
        for form in AB.FORMS:
            d = AB.digest(ops, form, n, halves)
            if form in AB.PLAIN:
                assert AB.digest(ops, form, n, halves, through_w=True) == d, f"{form} at n = {n}: ops.adamw_step computes other bits"
            res["digests"][form][str(n)] = d
        print(f"n = {n}: recorded", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        # one line per digest; a size's list of max_norm values on one line
        f.write(re.sub(r"\[\s+([^\]]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", json.dumps(res, indent=1)) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
