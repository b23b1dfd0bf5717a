"""Write tests/golden/step_bits.json: for every launch of
tests/step_bits_cases.py, the sha256 of the raw bytes of each output array
(pred, h, metrics; A and cost where the case asks for them; the gradient row
in train mode), as the library in the tree computes them on the GPU.

    python tools/make_step_bits.py [--lib LIB.so] [--out FILE] [--check]

Run it on the commit whose bits are the reference (the parent of a change
that must not move them).  --check compares with the committed file instead
of writing it and exits 1 on a difference.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime per process)
from multimodaltraj_2_amd import _lib  # noqa: E402
from tests import step_bits_cases as sb  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_bits.json")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libg2k_hip.so")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args(argv)
    if args.lib:
        _lib._lib = _lib.load(args.lib)
    dev = torch.device("cuda:0")
    got = {c.id: sb.run_case(c, dev) for c in sb.CASES}
    if args.check:
        with open(GOLDEN) as f:
            want = json.load(f)
        bad = [(k, n) for k in got for n in got[k] if want.get(k, {}).get(n) != got[k][n]]
        bad += [(k, "(missing)") for k in want if k not in got]
        for k, n in bad:
            print(f"DIFF {k} {n}")
        print(f"{len(got)} cases, {len(bad)} differences")
        return 1 if bad else 0
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(got)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
