#!/usr/bin/env python3
"""What every rank of a world of N holds and runs with the stores of ``--train-input`` (``dat_store``, ``hist_store``, ``atis_store``;
``--store-records windows`` for the Gen1 store that keeps only the records its samples read): the ranks are built one after the other in
this one process, by ``data.*_store_for`` with the launcher's answers (``yolox.utils.get_rank`` / ``get_world_size``) replaced, from
``--data-dir`` or, without one, from the seeded synthetic recordings (``--recordings``, default 16 x 16 labels x 200 000 events for
``dat_store``, 16 x 48 representations for ``hist_store``, 64 x 20 000 events for ``atis_store``; the canvas is ``--size``, default 256 x 320).

Per world size in ``--world`` (default 1 2 4 8) and rank, one line:

  recordings   recordings of the rank that carry samples / owned samples of all samples
  held         bytes of ``records`` (``sums`` for ``hist_store``) the rank holds with ``store_shard = 'recordings'``
  build        host clock around the construction of the rank's store, ended by a device synchronise.  The synthetic recordings are
               generated once and kept (every rank is handed all of them, as a rank that reads a directory lists all of it), and the
               world-1 store is built once before it is timed (code objects, allocator), so the figure is the store's own work: parsing,
               the tables, the upload, and for ``hist_store`` / ``windows`` the device passes over the records
  steps        steps per epoch at the global batch ``--batch`` (default 16): replica mode (``store_shard = 'none'``, every rank holds the
               world-1 store) / shard mode; ``-`` where the batch does not divide or a rank owns fewer samples than one batch

Development tool; ``--device cpu`` where the store builds there (not ``--store-records windows``)."""
import argparse
import functools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from eas_snn_amd import data
import yolox.utils
from yolox.exp import get_exp

ap = argparse.ArgumentParser()
ap.add_argument('--train-input', default='dat_store', choices=['dat_store', 'hist_store', 'atis_store'])
ap.add_argument('--store-records', default='all', choices=list(data.STORE_RECORDS))
ap.add_argument('--data-dir', default='')
ap.add_argument('--recordings', type=int, nargs='+', default=None)
ap.add_argument('--size', type=int, nargs=2, default=(256, 320))
ap.add_argument('--world', type=int, nargs='+', default=[1, 2, 4, 8])
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--device', default='cuda:0')
opt = ap.parse_args()

dev = torch.device(opt.device)
store_for = {'dat_store': data.gen1_store_for, 'hist_store': data.hist_store_for, 'atis_store': data.ncaltech_store_for}[opt.train_input]
Loader = {'dat_store': data.Gen1StoreLoader, 'hist_store': data.Gen4StoreLoader, 'atis_store': data.NCaltechStoreLoader}[opt.train_input]
recordings = tuple(opt.recordings) if opt.recordings else {'dat_store': (16, 16, 200_000), 'hist_store': (16, 48), 'atis_store': (64, 20_000)}[opt.train_input]


for name in ('synth_gen1_recordings', 'synth_gen4_recordings', 'synth_ncaltech_recordings'):
    setattr(data, name, functools.lru_cache(maxsize=None)(getattr(data, name)))


def experiment(shard):
    e = get_exp(None, 'e-yolox-s')
    e.train_input, e.store_records, e.store_shard, e.data_dir = opt.train_input, opt.store_records, shard, opt.data_dir
    e.store_recordings = e.atis_store_recordings = recordings
    e.merge(['input_size', str(tuple(opt.size)), 'test_size', str(tuple(opt.size)), 'num_classes', '2'])
    return e


def as_rank(rank, world):
    yolox.utils.get_rank, yolox.utils.get_world_size = (lambda: rank), (lambda: world)


def built(e):
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = store_for(e, 'train', dev)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return store, time.perf_counter() - t0


def held(store):
    if opt.train_input == 'hist_store':
        return int(store.held_offsets[-1]) * 2 * store.sensor_hw[0] * store.sensor_hw[1] * 2
    return store.records.numel()


def recordings_of(store):
    own = store.owned_samples
    if opt.train_input == 'atis_store':
        return len(own)
    file_of = store.group_file if opt.train_input == 'hist_store' else store.host['group_file']
    return len(set(np.asarray(file_of)[own].tolist()))


def steps(make):
    try:
        return str(len(make()))
    except (ValueError, AssertionError):
        return '-'


print(f'{opt.train_input} ({opt.store_records}), ' + (f'data_dir {opt.data_dir}' if opt.data_dir else f'synthetic recordings {recordings}')
      + f', canvas {tuple(opt.size)}, global batch {opt.batch}, {dev}')
as_rank(0, 1)
built(experiment('none'))                                                  # warm-up; the store goes with its experiment
whole, took = built(experiment('none'))
print(f'world 1 rank 0: recordings {recordings_of(whole):4d}   samples {len(whole):6d} / {len(whole):6d}   held {held(whole) / 1e6:10.2f} MB   '
      f'build {took:7.3f} s   steps {steps(lambda: Loader(experiment("none"), opt.batch, store=whole))} / -')
for world in opt.world:
    if world == 1:
        continue
    for rank in range(world):
        as_rank(rank, world)
        e = experiment('recordings')
        store, took = built(e)
        ok = opt.batch % world == 0
        replica = steps(lambda: Loader(e, opt.batch // world, store=whole, rank=rank, world=world)) if ok else '-'
        shard = steps(lambda: Loader(e, opt.batch // world, store=store)) if ok else '-'
        print(f'world {world} rank {rank}: recordings {recordings_of(store):4d}   samples {len(store.owned_samples):6d} / {len(store):6d}   '
              f'held {held(store) / 1e6:10.2f} MB   build {took:7.3f} s   steps {replica} / {shard}')
        del store, e
