"""What ``tests/golden/store_draws.npz`` freezes, computed from the code at hand: the three small CPU stores of
``test_cpu_store_ranks`` (``gen1_store``, ``gen4_store``, ``atis_store``), each whole and as the shards (0, 2) and (1, 2).  Per store: every
array of ``store.host``, ``owned_samples``, ``sample_rank`` (a sharded store), ``raw_labels`` of the first owned sample, and ``batches(0)``
/ ``batches(1)`` of its training loader at batch 2, seed 7; for the whole store also the batches of rank 1 of a world of 2.
``scripts/gen_golden_store_draws.py`` writes the fixture from ``record()``; ``test_cpu_store_frozen`` compares ``record()`` against it.

``inputs_digest()`` is the SHA-256 over the synthetic recordings that go in (every array's dtype, shape and bytes, every name), so that a
numpy whose generators draw differently shows as that and not as a change of the stores."""
import hashlib

import numpy as np

import test_cpu_store_ranks as small

VARIANTS = {'whole': None, 'shard0of2': (0, 2), 'shard1of2': (1, 2)}
RECORDINGS = {'gen1': small.gen1_recs, 'gen4': small.gen4_recs, 'atis': small.atis_recs}


def inputs_digest():
    h = hashlib.sha256()
    for kind in sorted(RECORDINGS):
        for rec in RECORDINGS[kind]():
            for v in rec:
                if isinstance(v, str):
                    h.update(v.encode())
                else:
                    a = np.ascontiguousarray(v)
                    h.update(f'{a.dtype.str if a.dtype.names is None else a.dtype.descr}{a.shape}'.encode())
                    h.update(a.tobytes())
    return h.hexdigest()


def record():
    """{key: array} of everything frozen, in a fixed order"""
    out = {}
    for kind in sorted(small.KINDS):
        build, Loader = small.KINDS[kind]
        exp = small.kind_exp(kind)
        for variant, shard in VARIANTS.items():
            store = build() if shard is None else build(shard=shard)
            at = f'{kind}/{variant}'
            for k, v in store.host.items():
                out[f'{at}/host/{k}'] = v
            out[f'{at}/owned_samples'] = store.owned_samples
            if store.sample_rank is not None:
                out[f'{at}/sample_rank'] = store.sample_rank
            out[f'{at}/raw_labels'] = store.raw_labels(int(store.owned_samples[0]))
            loaders = {'loader': Loader(exp, 2, store=store, seed=7)}
            if shard is None:
                loaders['rank1of2'] = Loader(exp, 2, store=store, seed=7, rank=1, world=2)
            for name, loader in loaders.items():
                for epoch in (0, 1):
                    for i, draws in enumerate(loader.batches(epoch)):
                        for j, a in enumerate(draws):
                            out[f'{at}/{name}/epoch{epoch}/batch{i}/{j}'] = a
    return out
