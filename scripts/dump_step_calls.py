#!/usr/bin/env python3
"""Every C-ABI call of one eager training step as text, one call per line (development tool): the record two commits are compared by
when a change of the operator layer must leave the calls as they are (profiles/bn_host_ab.txt).  The step is the bench's own step object
at the bench batch, built like tests/test_gpu_bench_shapes.py builds it.  Integer and float arguments are printed as they are, pointer
arguments as null / ptr (addresses differ from run to run), structs and problem arrays field by field.  Behind the calls: calls and
algorithmic bytes per kernel family as the KernelTimer of one more step saw them, and the library's launch counter over the traced step.
usage: dump_step_calls.py OUT.txt [config ...]      (default: 2 3 4 5)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import eas_snn_amd  # noqa: F401
from eas_snn_amd import _lib, ops, workloads


def _is_pointer(ctype):
    return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def _fmt(v, ctype=None):
    if hasattr(v, '_obj'):                       # C.byref(struct)
        return _fmt(v._obj)
    if isinstance(v, C.Structure):
        return '{' + ' '.join(f'{f}={_fmt(getattr(v, f), t)}' for f, t in v._fields_) + '}'
    if isinstance(v, C.Array):
        return '[' + ' '.join(_fmt(e) for e in v) + ']'
    if ctype is not None and _is_pointer(ctype):
        return 'ptr' if v else 'null'
    return repr(v)


def dump_config(config, out):
    dev = torch.device('cuda:0')
    w = workloads.get(config)
    trainer, model, step = workloads.build_trainer(w, w['batch'], dev, events=200_000)
    L = _lib.lib()
    with ops.no_state_writeback():
        step.eager()                                  # allocator / lazily built state
        torch.cuda.synchronize()
        c0 = L.eas_launch_counter()
        with ops.kernel_trace() as tr:
            step.eager()
        torch.cuda.synchronize()
        launches = int(L.eas_launch_counter() - c0)
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        try:
            step.eager()
        finally:
            ops.set_timer(None)
        torch.cuda.synchronize()
    assert torch.isfinite(step.loss)
    out.write(f'== config {config}: {len(tr.calls)} calls, eas_launch_counter +{launches}\n')
    for name, args in tr.calls:
        types = _lib.PROTOTYPES[name][1]
        types = types if len(types) == len(args) else [None] * len(args)      # (a hand-written log entry: values only)
        out.write(name + ' ' + ' '.join(_fmt(a, t) for a, t in zip(args, types)) + '\n')
    for fam, v in sorted(timer.summary().items()):
        out.write(f"timer {fam}: calls {v['calls']} bytes {v['bytes']}\n")
    del trainer, model, step
    torch.cuda.empty_cache()


def main():
    configs = [int(a) for a in sys.argv[2:]] or [2, 3, 4, 5]
    with open(sys.argv[1], 'w') as out:
        for config in configs:
            dump_config(config, out)


if __name__ == '__main__':
    main()
