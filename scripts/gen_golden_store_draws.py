"""Writes tests/golden/store_draws.npz: the tables and the draws of the three small CPU stores (``tests/store_draws_ref.py`` says which),
as the code at hand computes them, with the SHA-256 of the synthetic recordings that went in (``inputs_sha256``).  Run it at the commit
whose behaviour is to be frozen -- before a change of the stores or their loaders that must change nothing:

    python scripts/gen_golden_store_draws.py [--out tests/golden/store_draws.npz]

``tests/test_cpu_store_frozen.py`` rebuilds all of it and compares every array exactly.  No device is needed."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
sys.dont_write_bytecode = True

import store_draws_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'store_draws.npz'))
    args = ap.parse_args()
    out = store_draws_ref.record()
    again = store_draws_ref.record()
    assert list(out) == list(again) and all(np.array_equal(out[k], again[k]) and out[k].dtype == again[k].dtype for k in out)
    np.savez_compressed(args.out, inputs_sha256=np.array(store_draws_ref.inputs_digest()), **out)
    print(args.out, len(out), 'arrays', os.path.getsize(args.out), 'bytes')
    assert os.path.getsize(args.out) < 100 * 1024


if __name__ == '__main__':
    main()
