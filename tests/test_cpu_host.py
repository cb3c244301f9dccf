"""CPU-only tests: the C-ABI library loads and exports what include/eas_hip.h declares, host-side logic
(experiment options, module tree rewrite, checkpoint keys), and the multi-process path on gloo (world_size 2)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, split_cases

import eas_snn_amd  # noqa: E402  (puts compat/ on sys.path)

README_OPTS = ['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum',
               'embedding_depth', '2', 'embedding_ksize', '5', 'write_zero', 'True', 'use_spike', 'True', 'spike_fn', 'atan',
               'input_size', '(256,320)', 'test_size', '(256,320)']


def _header_functions():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    path = eas_snn_amd.build()
    assert os.path.exists(path)
    eas_snn_amd._lib._bind_host_hip_runtime()      # the library binds to the host process's HIP runtime
    handle = ctypes.CDLL(path)
    names = _header_functions()
    assert len(names) >= 17
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eas_hip.h but not exported'
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == names           # ctypes table covers exactly the header
    lib = eas_snn_amd.hip_library()
    assert lib.eas_abi_version() == eas_snn_amd._lib.ABI_VERSION == 9
    assert lib.eas_status_string(-1).decode().startswith('invalid argument')
    assert lib.eas_bn_workspace_doubles(32) > 0 and lib.eas_reduce_workspace_floats(1 << 20) > 0


def test_weight_gradient_queries_say_zero_where_the_launch_refuses():
    """eas_conv_wgrad_workspace_floats and eas_conv_wgrad_parts ask the rule eas_conv_wgrad launches by (conv_wgrad_mfma.hip wg_support;
    the queries need no GPU: an instance then counts as one resident block per CU): 0 for 3x3 problems it refuses -- output channels or input
    channels that are no multiple of 8, an odd input width, an odd output width (6 columns at stride 2), and the two 3x3 rows of CONV_CASES
    the GPU test names as the library's (Cout = 5; Ho * Wo = 30, no multiple of 4) -- and a plan for every other 3x3 row of the
    fp64-compared GPU cases, in each input form the row's shape allows."""
    from test_gpu_kernels import CONV_CASES, WGRAD_INSTANCE_CASES, WGRAD_LIBRARY_CASES
    lib = eas_snn_amd.hip_library()
    refused = [(2, 16, 5, 8, 10, 1), (2, 12, 16, 8, 10, 1), (2, 16, 16, 8, 9, 1), (2, 16, 16, 8, 6, 2)]
    refused += [(NI, Cin, Cout, H, W, s) for NI, Cin, Cout, H, W, k, s, _ in WGRAD_LIBRARY_CASES]
    for NI, Cin, Cout, H, W, s in refused:
        for xt in (1, 2, 3):
            assert lib.eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, 3, s, xt) == 0, (NI, Cin, Cout, H, W, s, xt)
            assert lib.eas_conv_wgrad_parts(NI, Cin, Cout, H, W, s, xt) == 0, (NI, Cin, Cout, H, W, s, xt)
    rows = [c for c in CONV_CASES + WGRAD_INSTANCE_CASES if c[5] == 3 and c not in WGRAD_LIBRARY_CASES]
    assert len(rows) >= 30 and all(c[5] == 3 for c in WGRAD_LIBRARY_CASES)
    for NI, Cin, Cout, H, W, k, s, spikes in rows:
        for xt in ((1, 2) if spikes else (3,)):
            floats = lib.eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, 3, s, xt)
            assert floats > 0 and floats % (Cout * Cin * 9) == 0, (NI, Cin, Cout, H, W, s, xt)
            assert 1 <= lib.eas_conv_wgrad_parts(NI, Cin, Cout, H, W, s, xt) <= 8, (NI, Cin, Cout, H, W, s, xt)


def test_1x1_weight_gradient_query_says_zero_where_the_launch_refuses():
    """the 1x1 branch of eas_conv_wgrad_workspace_floats (conv1x1_mfma.hip eas_conv1x1_wgrad_slices; no GPU needed): 0 for maps whose pixel
    count is no multiple of 16 in every input form, and for spike planes whose channels are not whole 8-groups -- what
    eas_conv1x1_wgrad_dispatch refuses; whole slabs of Cout * Cin floats otherwise."""
    lib = eas_snn_amd.hip_library()
    for xt in (1, 2, 3):
        assert lib.eas_conv_wgrad_workspace_floats(2, 16, 24, 5, 7, 1, 1, xt) == 0, xt          # HW = 35
        assert lib.eas_conv_wgrad_workspace_floats(2, 16, 24, 6, 8, 1, 2, xt) == 0, xt          # no stride-2 1x1
        floats = lib.eas_conv_wgrad_workspace_floats(2, 16, 24, 6, 8, 1, 1, xt)
        assert floats > 0 and floats % (24 * 16) == 0, xt
    assert lib.eas_conv_wgrad_workspace_floats(2, 12, 24, 6, 8, 1, 1, 2) == 0
    assert lib.eas_conv_wgrad_workspace_floats(2, 12, 24, 6, 8, 1, 1, 3) > 0 and lib.eas_conv_wgrad_workspace_floats(2, 12, 24, 6, 8, 1, 1, 1) > 0


def test_stride2_input_gradient_query_is_the_launch_rule_and_the_route_follows_it():
    """eas_conv_dgrad_s2_supported is the plan eas_conv_dgrad_s2 launches by (conv_s2d.hip; no GPU needed): 1 for every row of the
    fp64-compared GPU cases, 0 for an odd output width (Wo = 5), output channels that are no multiple of 8 (Cout = 12), rows wider than the
    widest tile (Wo = 260 > 256) and NI * Ho beyond the range of the kernels' multiply-shift division (2^20; arguments only, nothing is
    allocated).  ops.conv_route names the stride-2 kernel exactly where the query says 1."""
    from test_gpu_kernels import S2_DGRAD_CASES
    from eas_snn_amd import ops
    lib = eas_snn_amd.hip_library()
    refused = [(1, 8, 8, 4, 10), (1, 8, 12, 4, 8), (1, 8, 8, 2, 520), (1 << 19, 8, 8, 4, 8)]
    assert len(S2_DGRAD_CASES) >= 13
    for NI, Cin, Cout, H, W in S2_DGRAD_CASES:
        assert lib.eas_conv_dgrad_s2_supported(NI, Cin, Cout, H, W) == 1, (NI, Cin, Cout, H, W)
    for NI, Cin, Cout, H, W in refused:
        assert lib.eas_conv_dgrad_s2_supported(NI, Cin, Cout, H, W) == 0, (NI, Cin, Cout, H, W)
    for NI, Cin, Cout, H, W in S2_DGRAD_CASES + refused:
        want = 2 if lib.eas_conv_dgrad_s2_supported(NI, Cin, Cout, H, W) else None
        assert ops.conv_route((NI, Cin, H, W), Cout, 3, 2, 3).dgrad == want, (NI, Cin, Cout, H, W)


def _hist_plan(lib, nev, B, Tm, H, W, aligned16, _out=(ctypes.c_int(), ctypes.c_int(), ctypes.c_int64())):
    rows, nbands, lds = _out
    form = lib.eas_event_histogram_plan(nev, B, Tm, H, W, aligned16, ctypes.byref(rows), ctypes.byref(nbands), ctypes.byref(lds))
    return form, rows.value, nbands.value, lds.value


def test_event_histogram_plan_query_is_the_launch_rule(monkeypatch):
    """eas_event_histogram_plan answers by the code eas_event_histogram / eas_event_frames launch by (events.hip hist_form / hist_band_plan;
    no GPU needed, arguments only).  Every band plan over H 1..1200 x W 1..2048, both counter widths, asks for at most 150 KB of dynamic LDS
    (what the kernels declare), has at most 8 bands, and its bands cover the frame with none of them empty; the plans of the sensors the
    project names; 74 x 1024, where an odd 16-bit row capacity (37) once gave 2 bands of 37 rows and 155 648 B; and the form choice."""
    monkeypatch.delenv('EAS_HIST_FORM', raising=False)
    lib = eas_snn_amd.hip_library()
    dense = 1 << 40
    rows, nbands, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    out = (ctypes.byref(rows), ctypes.byref(nbands), ctypes.byref(lds))
    query, nplans = lib.eas_event_histogram_plan, [0, 0]
    for aligned16 in (1, 0):
        for H in range(1, 1201):
            for W in range(1, 2049):
                form = query(dense, 1, 1, H, W, aligned16, *out)
                if form == 0:
                    continue
                r, n = rows.value, nbands.value
                assert form == (2 if aligned16 else 1) and lds.value <= 150 * 1024 and 1 <= n <= 8 and r * n >= H > r * (n - 1), (H, W, aligned16)
                nplans[aligned16] += 1
    assert nplans[1] > nplans[0] > 100_000                   # a 16-bit band is at least as tall: no frame has a 32-bit plan only
    assert _hist_plan(lib, dense, 1, 1, 240, 304, 1) == (2, 120, 2, 145920) and _hist_plan(lib, dense, 1, 1, 240, 304, 0)[:3] == (1, 60, 4)
    assert _hist_plan(lib, dense, 1, 1, 480, 640, 1) == (2, 60, 8, 153600) and _hist_plan(lib, dense, 1, 1, 480, 640, 0) == (0, 0, 0, 0)
    assert _hist_plan(lib, dense, 1, 1, 720, 1280, 1) == _hist_plan(lib, dense, 1, 1, 720, 1280, 0) == (0, 0, 0, 0)
    assert _hist_plan(lib, dense, 1, 1, 74, 1024, 1)[:3] == (2, 25, 3)
    # the choice: density nev >= 2048 * B * Tm, 16-bit counters only for aligned event arrays, B * Tm < 2^24
    assert _hist_plan(lib, 64 * 4 * 2048 - 1, 64, 4, 240, 304, 1)[0] == 0 and _hist_plan(lib, 64 * 4 * 2048, 64, 4, 240, 304, 1)[0] == 2
    assert _hist_plan(lib, 64 * 4 * 2048, 64, 4, 240, 304, 0)[0] == 1 and _hist_plan(lib, dense, 1 << 22, 4, 240, 304, 1)[0] == 0
    assert lib.eas_event_histogram_plan(dense, 1, 1, 0, 304, 1, None, None, None) < 0          # invalid argument; NULL outputs are allowed
    monkeypatch.setenv('EAS_HIST_FORM', 'banded32')           # the development switch holds for the query as for the launch
    assert _hist_plan(lib, 0, 1, 1, 240, 304, 1)[:3] == (1, 60, 4)


def test_gfx950_code_object_only():
    out = subprocess.run(['/opt/rocm/lib/llvm/bin/clang-offload-bundler', '--list', '--type=o',
                          f'--input={eas_snn_amd._lib.LIB_PATH}'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    if 'gfx' in out:
        assert 'gfx950' in out and 'gfx90a' not in out and 'gfx942' not in out


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from eas_snn_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.EasHipError, match='no CPU fallback'):
        _lib.lib()


def test_no_cpu_fallback_for_neurons_and_sampler():
    from spikingjelly.activation_based import neuron, surrogate
    from yolox.models.embedding import AdaptiveRSNNEmbedding
    from yolox.models.activation import Rectangle
    node = neuron.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=None, surrogate_function=surrogate.ATan(), step_mode='m')
    with pytest.raises(eas_snn_amd.EasHipError):
        node(torch.zeros(3, 1, 2, 4, 4))
    emb = AdaptiveRSNNEmbedding(5, nb_steps=4, thresh=1.0, vreset=0.0, spike_fn=Rectangle)
    with pytest.raises(eas_snn_amd.EasHipError):
        emb(torch.zeros(1, 1, 4, 2, 8, 8))
    assert emb(torch.zeros(1, 2, 8, 8)).shape == (1, 1, 2, 8, 8)         # registration passthrough needs no kernel


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, 'eas_snn_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(base, f)).read()
                if re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M):
                    bad.append(os.path.join(base, f))
    assert not bad, bad


def test_exp_merge_type_coercion_quirks():
    from yolox.exp import get_exp
    exp = get_exp(None, 'e-yolox-s')
    assert (exp.depth, exp.width, exp.max_epoch) == (0.33, 0.50, 60)
    exp.merge(README_OPTS + ['alpha', '1.5', 'abs', 'False', 'nonexistent_key', '1'])
    assert exp.T == 3 and isinstance(exp.T, int)
    assert exp.input_size == (256, 320) or list(exp.input_size) == [256, 320]
    assert exp.use_spike == 'True' and isinstance(exp.use_spike, str)       # a string option
    assert exp.abs is True                                                   # bool("False") is True, as upstream
    assert exp.alpha == 1.5 and not hasattr(exp, 'nonexistent_key')
    assert exp.get_slice_args()['window'] == (-200000, 0)


def test_exp_merge_equals_the_reference_merge():
    """``BaseExp.merge`` against the results of the reference's own method (yolox/exp/base_exp.py:67-90), recorded by oracle/gen_golden.py
    (tests/golden/exp_merge.npz) on the same defaults and overrides: ints, floats, strings, the ``bool('False')`` quirk, None defaults,
    tuples / lists (brackets or not, empty defaults), unknown keys, a literal_eval fallback, and overrides that raise -- same value, same
    type, same exception"""
    import ast
    from yolox.exp.base_exp import BaseExp as Ours
    O = type('X', (Ours,), {n: (lambda self, *a, **k: None) for n in getattr(Ours, '__abstractmethods__', ())})
    rec = split_cases(load_golden('exp_merge'))
    dflt = rec.pop('defaults')
    defaults = {str(k): ast.literal_eval(str(v)) for k, v in zip(dflt['keys'], dflt['repr'])}
    assert len(defaults) == 11 and len(rec) == 20
    for name in sorted(rec):
        case = rec[name]
        cs = [str(t) for t in case['override']]
        o = O()
        for key, v in defaults.items():
            setattr(o, key, v)
        try:
            o.merge(list(cs))
            err = ''
        except Exception as exc:
            err = type(exc).__name__
        assert err == str(case['error']), (cs, err, str(case['error']))
        assert sorted(set(cs[0::2])) == [str(k) for k in case['keys']]
        for key, r, t in zip(case['keys'], case['repr'], case['type']):
            vo = getattr(o, str(key), '<absent>')
            if str(t) == '<absent>':
                assert vo == '<absent>', (cs, key, vo)
            else:
                assert vo == ast.literal_eval(str(r)) and type(vo).__name__ == str(t), (cs, key, vo, str(r), str(t))
    with pytest.raises(AssertionError):
        O().merge(['a'])


@pytest.mark.parametrize('name,use_spike,extra', [('model_s_true_64', 'True', []), ('model_s_full_64', 'full_spike', []),
                                                  ('model_s_fullv2_64', 'full_spike_v2', []), ('model_s_false_64', 'False', []),
                                                  ('model_m_fullv2_t5_64x96', 'full_spike_v2', ['T', '5']),
                                                  ('model_s_true_patan_64', 'True', ['spike_fn', 'patan'])])
def test_model_tree_and_checkpoint_keys_match_reference(name, use_spike, extra):
    from spikingjelly.activation_based import layer, neuron
    from yolox.exp import get_exp
    g = load_golden(name)
    exp = get_exp(None, 'e-yolox-m' if '_m_' in name else 'e-yolox-s')
    exp.merge([o if o != 'True' or README_OPTS[i - 1] != 'use_spike' else use_spike for i, o in enumerate(README_OPTS)] + extra)
    model = exp.get_model()
    assert [str(k) for k in g['keys']] == list(model.state_dict().keys())
    assert sum(p.numel() for p in model.parameters()) == int(g['nparam'])
    n_plif = sum(isinstance(m, neuron.ParametricLIFNode) for m in model.modules())
    assert n_plif == {'True': 34, 'full_spike': 58, 'full_spike_v2': 73, 'False': 0}[use_spike] or '_m_' in name
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert (m.eps, m.momentum) == (1e-3, 0.03)
        if isinstance(m, layer.BatchNorm2d):
            assert isinstance(m, torch.nn.BatchNorm2d) and m.step_mode == 'm'
    if use_spike == 'True':
        assert type(model.backbone.backbone.stem).__name__ == 'SeqToANNContainer'
        assert isinstance(model.backbone.backbone.stem[0].conv.act, torch.nn.SiLU)          # stem stays ANN
        opt = exp.get_optimizer(64)
        if 'patan' in name:     # every neuron also owns the learnable slope ...surrogate_function.inv_sg.alpha (activation.py:121-124)
            assert [len(g_['params']) for g_ in opt.param_groups] == list(g['optimizer_group_sizes']) == [74, 83, 83, 68, 8]
            assert sum(k.endswith('act.surrogate_function.inv_sg.alpha') for k in model.state_dict()) == 34
        else:
            assert [len(g_['params']) for g_ in opt.param_groups] == [74, 83, 83, 34, 8]


def test_neuron_state_and_reset_semantics():
    from spikingjelly.activation_based import functional, neuron, surrogate
    node = neuron.ParametricLIFNode(init_tau=2.0, decay_input=False, v_threshold=1.0, v_reset=None,
                                    surrogate_function=surrogate.ATan(2.0), step_mode='m', backend='torch')
    assert node.v == 0. and float(node.w) == 0.0 and list(node.state_dict()) == ['w']
    node.v = torch.ones(2, 2)
    import copy
    c = copy.deepcopy(node)
    assert torch.equal(c.v, node.v) and c.v is not node.v
    functional.reset_net(torch.nn.Sequential(node))
    assert node.v == 0.
    with pytest.raises(NotImplementedError):
        node.backend = 'cupy'


# ------------------------------------------------------------------------------------------------ multi-process (gloo)
def _worker_main(tag, out_dir):
    import torch.distributed as dist
    import yolox.utils as U
    from yolox.utils.allreduce_norm import all_reduce_norm
    lazy = os.environ.get('EAS_LAZY_PG') == 'all'
    assert dist.is_initialized() == (not lazy)          # deferred launch: the first use of the default group below creates it
    rank, world = U.get_rank(), U.get_world_size()
    assert world == 2 and U.get_local_rank() == rank and U.get_local_size() == 2
    if lazy and tag == 'ddp_first':
        # what tools/eval_event.py does right after launch: a DistributedDataParallel constructor reaches for the default group
        torch.nn.parallel.DistributedDataParallel(torch.nn.Linear(3, 1, bias=False), broadcast_buffers=False)
        assert dist.is_initialized()
    torch.manual_seed(rank)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 4, 1), torch.nn.BatchNorm2d(4))
    with torch.no_grad():
        net[1].running_mean.fill_(float(rank + 1))
        net[1].weight.fill_(float(10 * (rank + 1)))
    all_reduce_norm(net)
    assert dist.is_initialized() and U.get_rank() == rank and U.get_local_rank() == rank
    assert torch.allclose(net[1].running_mean, torch.full((4,), 1.5)) and torch.allclose(net[1].weight, torch.full((4,), 15.0))
    # weak-scaling bookkeeping used by bench.py: value = all ranks' units / max-over-ranks time
    el = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    assert float(el) == 2.0
    # DDP gradient averaging over the process group (the one hot collective)
    ddp = torch.nn.parallel.DistributedDataParallel(torch.nn.Linear(3, 1, bias=False), broadcast_buffers=False)
    with torch.no_grad():
        ddp.module.weight.fill_(1.0)
    ddp(torch.full((1, 3), float(rank + 1))).sum().backward()
    assert torch.allclose(ddp.module.weight.grad, torch.full((1, 3), 1.5))
    # the flat gradient all-reduce bench.py uses at N > 1 (eas_snn_amd/parallel.py): parameters broadcast from rank 0, gradients
    # averaged with one collective, identical to DDP's result
    from eas_snn_amd.parallel import FlatGradAllReduce
    torch.manual_seed(100 + rank)                       # different initial weights per rank: the constructor must equalise them
    mlp = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.ReLU(), torch.nn.Linear(4, 2))
    sync = FlatGradAllReduce(mlp)
    w0 = [p.detach().clone() for p in mlp.parameters()]
    gathered = [torch.zeros_like(w0[0]) for _ in range(world)]
    dist.all_gather(gathered, w0[0])
    assert torch.equal(gathered[0], gathered[1])
    x = torch.arange(6, dtype=torch.float32).view(2, 3) * (rank + 1)
    mlp(x).square().sum().backward()
    local = [p.grad.clone() for p in mlp.parameters()]
    sync.sync()
    for p, g in zip(mlp.parameters(), local):
        both = [torch.zeros_like(g) for _ in range(world)]
        dist.all_gather(both, g)
        assert torch.allclose(p.grad, (both[0] + both[1]) / 2, rtol=1e-6, atol=1e-7)
    open(os.path.join(out_dir, f'ok_{tag}_{rank}'), 'w').write('ok')


@pytest.mark.parametrize('lazy,tag', [('0', 't'), ('all', 't'), ('all', 'ddp_first')])
def test_launch_two_ranks_gloo(tmp_path, lazy, tag):
    """yolox.core.launch with world_size 2 on the gloo backend (the RCCL path differs only in the backend string).  lazy: the launcher
    defers the process group (its default on RCCL): rank / world size answer from the rendezvous parameters, and the first thing that
    reaches for the default group -- a collective, or a DistributedDataParallel constructor -- creates it."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import eas_snn_amd\n"
        "from yolox.core import launch\n"
        "from test_cpu_host import _worker_main\n"
        "if __name__ == '__main__':\n"
        "    launch(_worker_main, 2, 1, 0, backend='gloo', dist_url='auto', args=(%r, %r))\n"
    ) % (ROOT, os.path.join(ROOT, 'tests'), tag, str(tmp_path))
    script = tmp_path / 'run_launch.py'
    script.write_text(code)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', EAS_LAZY_PG=lazy)
    r = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert (tmp_path / f'ok_{tag}_0').exists() and (tmp_path / f'ok_{tag}_1').exists()


def test_model_ema_and_exp_lookup(tmp_path):
    """ModelEMA: floating entries follow keep*avg + (1-keep)*live with keep = decay*(1-exp(-n/2000)), integer buffers are left
    alone, DDP-style wrappers are looked through; get_exp: file wins over name, a broken file raises ImportError."""
    import math
    from yolox.exp import get_exp
    from yolox.utils import ModelEMA, is_parallel
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 1), torch.nn.BatchNorm2d(3))
    ema = ModelEMA(net, 0.9998)
    assert not is_parallel(net) and not ema.ema.training and not any(p.requires_grad for p in ema.ema.parameters())
    before = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
        net[1].running_mean.add_(0.5)
        net[1].num_batches_tracked.add_(7)
    ema.update(net)
    keep = 0.9998 * (1.0 - math.exp(-1 / 2000))
    assert ema.updates == 1 and abs(ema.decay(1) - keep) < 1e-15
    live = net.state_dict()
    for k, v in ema.ema.state_dict().items():
        if v.is_floating_point():
            torch.testing.assert_close(v, keep * before[k] + (1.0 - keep) * live[k], rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(v, before[k])

    good = tmp_path / 'my_exp_file.py'
    good.write_text('class Exp:\n    tag = "from-file"\n')
    assert get_exp(str(good), 'e-yolox-s').tag == 'from-file'
    bad = tmp_path / 'my_bad_exp_file.py'
    bad.write_text('x = 1\n')
    with pytest.raises(ImportError):
        get_exp(str(bad), None)
    with pytest.raises(AssertionError):
        get_exp(None, None)
    assert type(get_exp(None, 'e-yolox-s')).__name__ == 'Exp'


def test_no_file_is_a_token_level_copy_of_its_reference_namesake():
    """Copy check that survives reformatting: python tokens (comments, blank lines and indentation dropped) of every file under
    eas_snn_amd/ against each same-named file of the reference; the share of our tokens lying in common runs of >= 6 tokens must
    stay below 0.72 (the closest files are name-and-topology contracts: darknet constructor 0.69, Exp.merge 0.67, launch 0.65).
    Runs only where the reference tree exists (this container); nothing of it is read on the GPU box."""
    import difflib
    import io
    import tokenize
    ref_root = '/root/reference'
    if not os.path.isdir(ref_root):
        pytest.skip('reference tree not present')
    skip = {tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING, tokenize.ENDMARKER}

    def toks(path):
        with open(path, 'rb') as fh:
            return [t.string for t in tokenize.tokenize(io.BytesIO(fh.read()).readline) if t.type not in skip]
    ref = {}
    for d, _, fs in os.walk(ref_root):
        for f in fs:
            if f.endswith('.py'):
                ref.setdefault(f, []).append(os.path.join(d, f))
    worst = []
    for d, _, fs in os.walk(os.path.join(ROOT, 'eas_snn_amd')):
        for f in fs:
            if not f.endswith('.py') or f not in ref:
                continue
            a = toks(os.path.join(d, f))
            if len(a) < 30:
                continue
            for r in ref[f]:
                sm = difflib.SequenceMatcher(None, a, toks(r), autojunk=False)
                share = sum(b.size for b in sm.get_matching_blocks() if b.size >= 6) / len(a)
                worst.append((share, os.path.relpath(os.path.join(d, f), ROOT), os.path.relpath(r, ref_root)))
    worst.sort(reverse=True)
    assert worst and worst[0][0] < 0.72, f'token-level similarity to the reference too high: {worst[:3]}'


def _run_bench(argv, env_extra=None, drop=('WORLD_SIZE', 'RANK', 'LOCAL_RANK')):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_bench_gpus_2_starts_two_ranks_by_itself():
    """`python bench.py --gpus 2` (no WORLD_SIZE): the parent starts two children, they rendezvous (gloo here, RCCL on the GPU box),
    exchange gradients through FlatGradAllReduce and rank 0 prints ONE line reporting two ranks (reference: the tools spawn
    their workers, yolox/core/launch.py:59-98)."""
    import json
    r = _run_bench(['--gpus', '2', '--selftest-cpu', '--steps', '3', '--warmup', '1'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['rccl_ranks'] == 2 and rec['spawned_by_bench'] and rec['gradient_exchange'] == '2 buckets'
    assert rec['config']['config'] == 2
    # the order of the GPU path at N > 1: record with restore, THEN init_process_group, bind, steps -- and the first three losses equal
    # those of the group-first order of earlier rounds (bench.py selftest_cpu compares them on every rank)
    assert rec['order'].startswith('record (restore) -> init_process_group') and rec['same_losses_as_group_first_order'] is True
    assert len(rec['first_losses']) == 3


def test_bench_selftest_takes_the_other_baseline_configs():
    """`bench.py --selftest-cpu --config 3 --gpus 2`: the same verb selects BASELINE configs 3..5 (the line names the workload)"""
    import json
    r = _run_bench(['--gpus', '2', '--selftest-cpu', '--config', '3', '--steps', '2', '--warmup', '1'])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
    assert rec['config']['config'] == 3 and 'SYOLOX-M' in rec['config']['workload'] and 'T=5' in rec['config']['workload']
    from eas_snn_amd import workloads
    for c, gpus in ((2, 1), (3, 2), (4, 8), (5, 4)):
        w = workloads.get(c)
        assert w['baseline_gpus'] == gpus
        exp = workloads.build_exp(w)
        assert tuple(exp.input_size) == tuple(w['canvas']) and exp.Tm == w['Tm']
    with pytest.raises(KeyError):
        workloads.get(1)


def test_bench_refuses_a_rank_count_that_differs_from_gpus():
    r = _run_bench(['--gpus', '2', '--selftest-cpu'], env_extra={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'}, drop=())
    assert r.returncode != 0 and 'rank' in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith('{')]


def test_bench_launcher_reports_a_failing_rank():
    """a rank that dies takes the launch down with a non-zero code instead of leaving the others in a collective"""
    r = _run_bench(['--gpus', '2', '--selftest-cpu', '--steps', '1', '--warmup', '0'], env_extra={'EAS_BENCH_SELFTEST_FAIL_RANK': '1'})
    assert r.returncode != 0


def test_sampler_split_option_builds_the_reference_parameter_set():
    """split=True adds two convolutions the reference's forward never calls (embedding.py:100-102); they must exist so that
    checkpoints and optimizer groups of such a configuration match (key order = construction order of the reference)."""
    from yolox.models.activation import Rectangle
    from yolox.models.embedding import AdaptiveRSNNEmbedding
    m = AdaptiveRSNNEmbedding(5, split=True, depth=2, nb_steps=4, thresh=1.0, vreset=0.0, spike_fn=Rectangle)
    assert list(m.state_dict()) == ['gate_conv.0.weight', 'gate_conv.0.bias', 'gate_conv.2.weight', 'gate_conv.2.bias', 'input_conv.0.weight',
                                    'input_conv.0.bias', 'input_conv.2.weight', 'input_conv.2.bias', 'gate_conv_agg.weight', 'gate_conv_agg.bias',
                                    'input_conv_agg.weight', 'input_conv_agg.bias']
    assert m.gate_conv_agg.weight.shape == (4, 2, 5, 5) and m.input_conv_agg.weight.shape == (4, 2, 5, 5)


def test_convolution_statistics_slot_is_only_taken_by_the_tensor_it_belongs_to():
    """Host logic of the conv -> BN hand-over (ops.conv_stats_scope, ops._take_conv_stats): the statistics of a convolution are used
    only by a BN call on exactly that output (same storage address, channel count and element count per channel), a first of two
    consumers may leave them in place, anything else (another tensor, an output modified in place since) gets None and clears the slot -- a BN on an unrelated tensor falls back to its own
    statistics pass."""
    from eas_snn_amd import ops
    y = torch.zeros(6, 8, 4, 5)
    stats = torch.zeros(8 * 3 * 2, dtype=torch.float64)
    try:
        ops._CONV_STATS_SLOT = (y, 3, stats, y._version)
        assert ops._take_conv_stats(y.data_ptr(), 6 * 20, 8, keep=True) == (stats, 3)      # first consumer of a pair
        assert ops._take_conv_stats(y.data_ptr(), 6 * 20, 8) == (stats, 3)                 # second one clears
        assert ops._CONV_STATS_SLOT is None and ops._take_conv_stats(y.data_ptr(), 6 * 20, 8) is None
        other = torch.zeros(6, 8, 4, 5)
        for args in ((other.data_ptr(), 6 * 20, 8), (y.data_ptr(), 6 * 20, 4), (y.data_ptr(), 3 * 20, 8)):
            ops._CONV_STATS_SLOT = (y, 3, stats, y._version)
            assert ops._take_conv_stats(*args) is None and ops._CONV_STATS_SLOT is None
        ops._CONV_STATS_SLOT = (y, 3, stats, y._version)
        y.add_(1.0)                                                                         # modified in place after the convolution summed it
        assert ops._take_conv_stats(y.data_ptr(), 6 * 20, 8) is None and ops._CONV_STATS_SLOT is None
        ops._CONV_STATS_SLOT = (y, 3, stats, y._version)
        ops.clear_conv_stats()                                                              # end of a model forward: nothing stays pinned
        assert ops._CONV_STATS_SLOT is None
        with ops.conv_stats_scope(True):
            assert ops._WANT_CONV_STATS == ops.CONV_STATS
            with ops.conv_stats_scope(False):
                assert not ops._WANT_CONV_STATS
            assert ops._WANT_CONV_STATS == ops.CONV_STATS
        assert not ops._WANT_CONV_STATS
    finally:
        ops._CONV_STATS_SLOT = None


# ------------------------------------------------------------------------------------------------ the drop-in trainer on gloo
class _ToyStateful(torch.nn.Module):
    """a module with reset(): counts how often the trainer resets the network"""

    def __init__(self):
        super().__init__()
        self.resets = 0

    def reset(self):
        self.resets += 1

    def forward(self, x):
        return x


class _ToyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embedding = torch.nn.Sequential(torch.nn.Linear(6, 6), torch.nn.BatchNorm1d(6))    # (below the cut: the lower bucket)
        self.backbone = torch.nn.Module()
        self.backbone.backbone = torch.nn.Sequential(torch.nn.Linear(6, 6), _ToyStateful())
        self.head = torch.nn.Linear(6, 3)

    def forward(self, x, targets=None):
        h = torch.tanh(self.backbone.backbone(self.embedding(x)))
        return {'total_loss': ((self.head(h) - targets) ** 2).mean()}


class _ToyExp:
    max_epoch, ema, input_size, test_size, exp_name, use_spike = 1, True, (8, 8), (8, 8), 'toy', 'True'
    basic_lr_per_img, print_interval, eval_interval = 1e-2 / 4, 1, 1

    class _Evaluator:
        """records what Trainer.after_epoch hands to ``exp.eval`` (the real loop: test_evaluator_walks_the_eval_tool_sequence)"""

        def __init__(self):
            self.calls = []

        def evaluate(self, model, distributed=False, half=False, trt_file=None, decoder=None, test_size=None, return_outputs=False):
            self.calls.append(dict(training=model.training, distributed=distributed, bn_mean=model.embedding[1].running_mean.clone()))
            return ((0.25, 0.5, 'toy summary'), {0: {}}) if return_outputs else (0.25, 0.5, 'toy summary')

    def get_evaluator(self, batch_size, is_distributed, testdev=False, legacy=False):
        return self._Evaluator()

    def eval(self, model, evaluator, is_distributed, half=False, return_outputs=False):
        return evaluator.evaluate(model, is_distributed, half, return_outputs=return_outputs)

    def __init__(self, out):
        self.output_dir, self.model = out, None

    def get_model(self):
        if self.model is None:
            torch.manual_seed(3)
            self.model = _ToyNet()
        return self.model

    def get_optimizer(self, batch_size):
        return torch.optim.Adam(self.model.parameters(), lr=self.basic_lr_per_img * batch_size)

    def get_data_loader(self, batch_size, is_distributed, no_aug=False, cache_img=None):
        from yolox.utils import get_rank           # (answers from the launcher's parameters while the process group is still deferred)
        g = torch.Generator().manual_seed(100 + get_rank())
        return [(torch.randn(4, 6, generator=g), torch.randn(4, 3, generator=g)) for _ in range(3)]

    def get_lr_scheduler(self, lr, iters_per_epoch):
        from yolox.utils import LRScheduler
        return LRScheduler('yoloxwarmcos', lr, iters_per_epoch, self.max_epoch, warmup_epochs=0, warmup_lr_start=0, no_aug_epochs=0, min_lr_ratio=0.05)

    def preprocess(self, inputs, targets, tsize):
        return inputs, targets


def _trainer_worker(tag, out_dir):
    """yolox.core.Trainer (the drop-in training loop, compat/yolox/core/trainer.py) for one epoch of three iterations on every rank:
    bucketed gradient exchange with the split backward, Adam, reset_net, EMA, LR schedule, checkpoint."""
    import types
    import torch.distributed as dist
    from yolox.core import Trainer
    from yolox.utils import dist as comm
    from yolox.utils import get_local_rank, get_rank, get_world_size
    lazy = os.environ.get('EAS_LAZY_PG') == 'all'
    # deferred launch: no process group yet, but rank / world size are known from the launcher's parameters
    assert comm.process_group_deferred() == lazy and dist.is_initialized() == (not lazy)
    rank, world = get_rank(), get_world_size()
    assert world == 2 and rank in (0, 1) and get_local_rank() == rank
    exp = _ToyExp(out_dir)
    tr = Trainer(exp, types.SimpleNamespace(batch_size=8, fp16=False, experiment_name=f'toy_{tag}', ckpt=None, resume=False))
    seen = []
    join = tr.join_ranks
    tr.join_ranks = lambda: (seen.append((dist.is_initialized(), tr.step is not None, tr.exchange.bound)), join())
    tr.train()
    # the group comes into being inside join_ranks -- after the step object exists (on the GPU: after its graphs are recorded) -- and the
    # exchange binds to it there
    assert seen == [(not lazy, True, not lazy)] and dist.is_initialized() and tr.exchange.bound and tr.exchange.world == 2
    assert tr.exchange is not None and tr.exchange.nbuckets == 2 and tr.step.cut == ('backbone.backbone',)
    assert tr.step.graphs is None and len(tr.log) == 3                      # CPU: eager launches; one log row per iteration
    assert tr.bare_model.backbone.backbone[1].resets == 3 and tr.ema_model.updates == 3
    # after the epoch: all_reduce_norm made the per-rank BatchNorm statistics equal, THEN the evaluator saw the EMA model in eval mode
    # (trainer.py:243-248, 354-386 of the reference), the training model is back in training mode, and 'last_epoch' + best are saved
    rm = [torch.zeros(6) for _ in range(world)]
    dist.all_gather(rm, tr.bare_model.embedding[1].running_mean)
    assert torch.equal(rm[0], rm[1]) and float(rm[0].abs().sum()) > 0
    (call,) = tr.evaluator.calls
    assert call['training'] is False and call['distributed'] is True and tr.bare_model.training and tr.best_ap == 0.25
    assert tr.eval_log[0]['ap50'] == 0.5 and tr.eval_log[0]['summary'] == 'toy summary'
    if rank == 0:
        for name in ('last_epoch_ckpt.pth', 'best_ckpt.pth'):
            assert os.path.exists(os.path.join(out_dir, f'toy_{tag}', name)), name
    # every rank ends with the same parameters (same averaged gradients) that differ from the start
    torch.manual_seed(3)
    fresh = _ToyNet()
    for (n, p), q in zip(tr.bare_model.named_parameters(), fresh.parameters()):
        both = [torch.zeros_like(p) for _ in range(world)]
        dist.all_gather(both, p.detach())
        assert torch.equal(both[0], both[1]), n
        assert not torch.equal(p.detach(), q.detach()), n
    # and they are what a single process computes from the two ranks' batches with plain backward + averaged gradients
    opt = torch.optim.Adam(fresh.parameters(), lr=exp.basic_lr_per_img * 8)
    loaders = []
    for r in range(world):
        g = torch.Generator().manual_seed(100 + r)
        loaders.append([(torch.randn(4, 6, generator=g), torch.randn(4, 3, generator=g)) for _ in range(3)])
    sched = exp.get_lr_scheduler(exp.basic_lr_per_img * 8, 3)
    for it in range(3):
        grads = None
        for r in range(world):
            fresh.zero_grad(set_to_none=True)
            fresh(*loaders[r][it])['total_loss'].backward()
            gs = [p.grad.clone() for p in fresh.parameters()]
            grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
        for p, g_ in zip(fresh.parameters(), grads):
            p.grad = g_ / world
        opt.step()
        for gr in opt.param_groups:
            gr['lr'] = sched.update_lr(it + 1)
    # (the BatchNorm running statistics of ``fresh`` saw both ranks' batches in turn: only parameters are compared)
    for (n, p), q in zip(tr.bare_model.named_parameters(), fresh.parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6, msg=n)
    if rank == 0:
        assert os.path.exists(os.path.join(out_dir, f'toy_{tag}', 'latest_ckpt.pth'))
    open(os.path.join(out_dir, f'ok_{tag}_{rank}'), 'w').write('ok')


@pytest.mark.parametrize('lazy', ['0', 'all'])
def test_trainer_runs_two_ranks_on_gloo(tmp_path, lazy):
    """The drop-in Trainer at world size 2 (gloo): its TrainStep -- the object bench.py measures -- with the bucketed exchange and the
    backward pass split at the backbone, against a single-process restatement (plain backward, gradients averaged by hand).  Both launch
    orders: the reference's (process group first) and the deferred one the RCCL backend uses (``yolox.core.launch`` hands the rendezvous
    to ``defer_process_group``; the Trainer creates the group in ``join_ranks``, after its step is built / recorded) -- same result."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import eas_snn_amd\n"
        "from yolox.core import launch\n"
        "from test_cpu_host import _trainer_worker\n"
        "if __name__ == '__main__':\n"
        "    launch(_trainer_worker, 2, 1, 0, backend='gloo', dist_url='auto', args=('t', %r))\n"
    ) % (ROOT, os.path.join(ROOT, 'tests'), str(tmp_path))
    script = tmp_path / 'run_trainer.py'
    script.write_text(code)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', EAS_LAZY_PG=lazy)
    r = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert (tmp_path / 'ok_t_0').exists() and (tmp_path / 'ok_t_1').exists()


# ------------------------------------------------------------------------------------------------ the evaluation side of the boundary
class _ToyDetector(torch.nn.Module):
    """eval-mode forward: frames [B,1,Tm,2,H,W] -> decoded predictions [B, A, 5 + classes] (cx, cy, w, h, obj, class scores)"""

    def __init__(self, anchors=24, classes=2):
        super().__init__()
        self.anchors, self.classes = anchors, classes
        self.proj = torch.nn.Linear(2 * 4, anchors * (5 + classes))
        self.neuron = _ToyStateful()

    def forward(self, x, targets=None):
        f = x.float().mean(dim=(-1, -2)).flatten(1)                          # [B, Tm * 2]
        r = self.neuron(self.proj(f)).view(-1, self.anchors, 5 + self.classes)
        box = torch.cat([r[..., :2].sigmoid() * 200.0 + 20.0, r[..., 2:4].sigmoid() * 60.0 + 8.0], -1)
        return torch.cat([box, r[..., 4:].sigmoid()], -1)


class _ToyEvalLoader:
    """the tuple the reference's evaluation loader yields, on the CPU: sample i is the same on every rank"""

    def __init__(self, batch_size, indices, sensor=(240, 304)):
        self.batch_size, self.indices, self.sensor = batch_size, list(indices), sensor
        self.dataset = type('D', (), {'map_val': True, 'random_aug': False, 'class_names': ['a', 'b']})()

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    @staticmethod
    def sample(i):
        return torch.rand(1, 4, 2, 8, 10, generator=torch.Generator().manual_seed(500 + i)) * 3

    def __iter__(self):
        H, W = self.sensor
        for b in range(len(self)):
            ids = self.indices[b * self.batch_size:(b + 1) * self.batch_size]
            yield (torch.stack([self.sample(i) for i in ids]), [torch.tensor([[10., 20., 30., 40., float(i % 2)]]) for i in ids],
                   (torch.full((len(ids),), H), torch.full((len(ids),), W)), torch.tensor(ids))


def _toy_eval_exp(out_dir, n_samples=10):
    """the real EventExp (options, get_evaluator, eval) with a CPU model and a CPU loader in place of the GPU ones"""
    from yolox.exp import get_exp

    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['num_classes', '2', 'use_spike', 'True', 'test_size', '(256,320)', 'test_conf', '0.3', 'nmsthre', '0.5'])
    exp.output_dir = out_dir

    def get_model():
        torch.manual_seed(11)
        exp.model = _ToyDetector()
        return exp.model

    def get_eval_loader(batch_size, is_distributed, **kwargs):
        import torch.distributed as dist
        assert kwargs == {'testdev': False, 'legacy': False}
        batch_size *= 2                                                      # event_yolox_base.py:489-491 of the reference
        rank, world = (dist.get_rank(), dist.get_world_size()) if is_distributed else (0, 1)
        return _ToyEvalLoader(batch_size // world, range(rank, n_samples, world))

    exp.get_model, exp.get_eval_loader = get_model, get_eval_loader
    return exp


def _oracle_postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
    from oracle import postprocess_ref
    out = postprocess_ref.postprocess(prediction.cpu().numpy(), num_classes, conf_thre, nms_thre, class_agnostic)
    return [None if o is None else torch.from_numpy(o) for o in out]


def _eval_tool_main(tag, out_dir, num_gpu):
    """the call sequence of tools/eval_event.py::main (:124-211) against the mirror; returns what rank 0 got"""
    import types
    import yolox.evaluators.event_evaluator as EV
    from yolox.utils import configure_nccl, fuse_model, get_local_rank, get_model_info, setup_logger
    EV.postprocess = _oracle_postprocess               # CPU: the checker's NMS stands in for eas_postprocess (which has no CPU form)
    args = types.SimpleNamespace(batch_size=4, test=False, legacy=False, fp16=False, fuse=True, conf=None, nms=None, tsize=None,
                                 experiment_name=f'eval_{tag}')
    exp = _toy_eval_exp(out_dir)
    is_distributed = num_gpu > 1
    configure_nccl()
    rank = get_local_rank()
    file_name = os.path.join(exp.output_dir, args.experiment_name)
    if rank == 0:
        os.makedirs(file_name, exist_ok=True)
    setup_logger(file_name, distributed_rank=rank, filename='val_log.txt', mode='a')
    model = exp.get_model()
    assert 'Params' in get_model_info(model, exp.test_size)
    evaluator = exp.get_evaluator(args.batch_size, is_distributed, args.test, args.legacy)
    evaluator.per_class_AP = True
    evaluator.per_class_AR = True
    model.eval()
    model = fuse_model(model)
    *_, summary = evaluator.evaluate(model, is_distributed, args.fp16, None, None, exp.test_size)
    return exp, model, evaluator, summary


def _expected_detections(exp, model, n_samples=10):
    """every sample on its own through the model and the checker's NMS, boxes scaled back to the sensor"""
    want = {}
    scale = min(exp.test_size[0] / 240.0, exp.test_size[1] / 304.0)
    with torch.no_grad():
        for i in range(n_samples):
            (det,) = _oracle_postprocess(model(_ToyEvalLoader.sample(i)[None]), 2, exp.test_conf, exp.nmsthre)
            if det is not None:
                box = det[:, :4] / scale
                want[i] = sorted((round(float(s), 5), int(c), [round(float(v), 3) for v in (b[0], b[1], b[2] - b[0], b[3] - b[1])])
                                 for b, s, c in zip(box, det[:, 4] * det[:, 5], det[:, 6]))
    return want


def _check_eval_result(exp, model, evaluator, summary, world):
    import yolox.utils as U
    if U.get_rank() != 0:
        assert summary is None
        return
    assert summary.startswith('Average forward time:') and 'Average NMS time:' in summary and 'Average inference time:' in summary
    # 10 samples, batch 8 / world: the last (short) batch is not timed; statistics = (inference s, NMS s, timed batches) summed over ranks
    per_rank_batches = {1: 2, 2: 2}[world]
    st = evaluator.last_statistics.tolist()
    assert st[2] == world * (per_rank_batches - 1) and st[0] > 0 and st[1] > 0
    assert model.neuron.resets >= per_rank_batches            # reset_net after every forward (snn_reset = use_spike)


def test_evaluator_walks_the_eval_tool_sequence(tmp_path):
    """tools/eval_event.py::main's calls -- get_model, get_model_info, get_evaluator, fuse_model, evaluator.evaluate(model, distributed,
    fp16, trt_file, decoder, test_size) -- on the mirror at world size 1: every detection record equals the per-sample restatement."""
    import yolox.evaluators.event_evaluator as EV
    saved = EV.postprocess
    try:
        exp, model, evaluator, summary = _eval_tool_main('w1', str(tmp_path), 1)
        _check_eval_result(exp, model, evaluator, summary, 1)
        (ap50_95, ap50, _), outputs = evaluator.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
        want = _expected_detections(exp, model)
        assert len(want) >= 8 and sum(len(v) for v in want.values()) >= 20         # the toy detector fires on nearly every sample
        got = {i: sorted((round(s_, 5), c, [round(v, 3) for v in (b_[0], b_[1], b_[2] - b_[0], b_[3] - b_[1])])
                         for b_, s_, c in zip(o['bboxes'], o['scores'], o['categories'])) for i, o in outputs.items()}
        assert got == want
        # the COCO-style records of one hand-made image: xyxy on the canvas -> xywh on the sensor, score = obj * class confidence
        recs = evaluator.convert_to_coco_format([torch.tensor([[32., 64., 96., 192., 0.5, 0.8, 1.]]), None], (torch.tensor([128, 128]), torch.tensor([160, 160])),
                                                torch.tensor([7, 8]))
        assert recs == [{'image_id': 7, 'category_id': 1, 'bbox': [16.0, 32.0, 32.0, 64.0], 'score': pytest.approx(0.4), 'segmentation': []}]
        assert ap50_95 is None or ap50_95 >= 0          # no pycocotools here: AP fields None, detections + timings delivered
        with pytest.raises(NotImplementedError):
            evaluator.evaluate(model, False, True)
    finally:
        EV.postprocess = saved


def _eval_worker(tag, out_dir):
    import torch.distributed as dist
    exp, model, evaluator, summary = _eval_tool_main(tag, out_dir, dist.get_world_size())
    _check_eval_result(exp, model, evaluator, summary, dist.get_world_size())
    (_, _, _), outputs = evaluator.evaluate(model, True, False, None, None, exp.test_size, return_outputs=True)
    if dist.get_rank() == 0:
        want = _expected_detections(exp, model)
        assert sorted(outputs) == sorted(want)                                   # rank 0 holds every rank's images
        for i, recs in want.items():
            assert sorted(round(s, 5) for s in outputs[i]['scores']) == sorted(r[0] for r in recs)
    open(os.path.join(out_dir, f'ok_{tag}_{dist.get_rank()}'), 'w').write('ok')


def test_evaluator_two_ranks_on_gloo(tmp_path):
    """the same sequence at world size 2 (gloo): samples rank, rank + 2, ... per rank, detections gathered to rank 0, statistics reduced"""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import eas_snn_amd\n"
        "from yolox.core import launch\n"
        "from test_cpu_host import _eval_worker\n"
        "if __name__ == '__main__':\n"
        "    launch(_eval_worker, 2, 1, 0, backend='gloo', dist_url='auto', args=('e', %r))\n"
    ) % (ROOT, os.path.join(ROOT, 'tests'), str(tmp_path))
    script = tmp_path / 'run_eval.py'
    script.write_text(code)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    r = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert (tmp_path / 'ok_e_0').exists() and (tmp_path / 'ok_e_1').exists()


def test_graph_capture_is_only_used_with_capturable_optimizers():
    """SGD passes the learning rate as a host number (a device-scalar lr would synchronise inside the capture)"""
    from yolox.core.trainer import optimizer_capturable
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert optimizer_capturable(torch.optim.Adam(p, lr=1e-3)) and optimizer_capturable(torch.optim.AdamW(p, lr=1e-3))
    assert not optimizer_capturable(torch.optim.SGD(p, lr=1e-3, momentum=0.9, nesterov=True))
    assert not optimizer_capturable(torch.optim.RMSprop(p, lr=1e-3))


def test_eval_proph_is_announced_not_silently_substituted():
    """README eval line (readme.md:157-160 of the reference, --eval_proh): the reference builds PSEEEvaluator for gen* data
    (event_yolox_base.py:512-523); the mirror has no Prophesee metric code and says so with a RuntimeWarning while handing out
    EventEvaluator (same inference loop and records)"""
    import warnings
    from yolox.evaluators import EventEvaluator
    from yolox.exp import get_exp
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['num_classes', '2', 'data_name', 'gen1', 'eval_proph', 'True', 'input_size', '(64,96)', 'test_size', '(64,96)'])
    with pytest.warns(RuntimeWarning, match='PSEEEvaluator'):
        ev = exp.get_evaluator(2, False)
    assert isinstance(ev, EventEvaluator)
    exp = get_exp(None, 'e-yolox-s')            # (a fresh one: merge coerces with bool(str), so 'False' would switch the flag ON -- base_exp.py of the reference)
    exp.merge(['num_classes', '2', 'data_name', 'gen1', 'input_size', '(64,96)', 'test_size', '(64,96)'])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert isinstance(exp.get_evaluator(2, False), EventEvaluator)


def test_checkpoint_carries_best_ap_and_resume_restores_it(tmp_path):
    """reference checkpoint format (trainer.py:393-400: start_epoch, model, optimizer, best_ap, curr_ap) and resume (trainer.py:331): a
    resumed run keeps its best AP, so its first evaluation cannot overwrite best_ckpt.pth with a worse model"""
    import types
    from yolox.core.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    net = torch.nn.Linear(4, 2)
    tr.device, tr.rank, tr.use_model_ema, tr.bare_model = 'cpu', 0, False, net
    tr.optimizer = torch.optim.SGD(net.parameters(), lr=0.1)
    tr.epoch, tr.best_ap, tr.file_name = 3, 0.4321, str(tmp_path)
    tr.save_ckpt('latest', ap=0.25)
    ck = torch.load(os.path.join(str(tmp_path), 'latest_ckpt.pth'), map_location='cpu')
    assert set(ck) == {'start_epoch', 'model', 'optimizer', 'best_ap', 'curr_ap'}
    assert ck['best_ap'] == 0.4321 and ck['curr_ap'] == 0.25 and ck['start_epoch'] == 4
    tr2 = Trainer.__new__(Trainer)
    tr2.device, tr2.file_name, tr2.best_ap, tr2.start_epoch = 'cpu', str(tmp_path), 0, 0
    tr2.args = types.SimpleNamespace(ckpt=None, resume=True)
    tr2.optimizer = torch.optim.SGD(net.parameters(), lr=0.1)
    tr2.resume_train(torch.nn.Linear(4, 2))
    assert tr2.best_ap == 0.4321 and tr2.start_epoch == 4


def test_workload_2b_is_config_2_at_the_readme_canvas():
    """the reference's published commands train at the default input_size (640, 640) (event_yolox_base.py:66,137) through the letterbox
    resize (gen1.py:438-455): workload '2b' = config 2's options at that canvas, 304x240 -> 640x505 pasted top-left"""
    from eas_snn_amd import data, workloads
    w2, wb = workloads.get(2), workloads.get('2b')
    assert wb['config'] == '2b' and wb['canvas'] == (640, 640) and wb['opts'] == w2['opts'] and wb['exp'] == w2['exp']
    assert data.letterbox_params(*wb['sensor'], *wb['canvas']) == (640, 505, 0, 0, 0)
    exp = workloads.build_exp(wb)
    assert tuple(exp.input_size) == (640, 640) and tuple(exp.test_size) == (640, 640)
    with pytest.raises(KeyError):
        workloads.get(7)


def test_graft_entry_build_runs_on_a_machine_without_a_gpu():
    """__graft_entry__.build() -- what the driver calls on the CPU container each round: compiles (here: finds up to date) every HIP source for
    gfx950, builds the oracle's C restatement, imports the package and the compat namespaces.  (It once pinned the ABI number of a past round.)"""
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    entry = importlib.import_module('__graft_entry__')
    entry.build()
    assert callable(entry.smoke)

