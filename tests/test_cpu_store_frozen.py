"""The tables and the draws of the stores against a frozen record (``tests/golden/store_draws.npz``, written by
``scripts/gen_golden_store_draws.py``): ``store.host``, ``owned_samples``, ``sample_rank``, ``raw_labels`` and the loaders' ``batches`` of
the three small CPU stores, whole and sharded, rebuilt here and compared array for array -- names, dtypes, shapes, values.  Everything
is an integer table, a float32 copy of an input or a draw from a seeded state: every comparison is exact."""
import os

import numpy as np

from conftest import ROOT

import store_draws_ref


def test_stores_and_draws_equal_the_frozen_record():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'store_draws.npz')) as z:
        want = {k: z[k] for k in z.files}
    digest = str(want.pop('inputs_sha256'))
    assert store_draws_ref.inputs_digest() == digest, (
        'the synthetic recordings differ from those the record was made of: the generators (synth_gen1_recordings, synth_gen4_recordings, '
        'synth_ncaltech_recordings) or the numpy under them changed, not the stores -- nothing below can be judged')
    got = store_draws_ref.record()
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    assert len(got) > 300
    for k, a in got.items():
        a, w = np.asarray(a), want[k]
        assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a, w), k
