"""CPU: the host side of the range guard of the split-fp16 products.

* rlg_range_scan, rlg_adam_step_guarded, rlg_adam_pack_guarded and rlg_mlp_dw_launch_form reject malformed calls with
  hipErrorInvalidValue before they ask the HIP runtime for anything.  As in tests/test_optim_entry_errors_cpu.py the
  table runs in a child process that sees no GPU, with small fake aligned addresses that the host code never
  dereferences (the pointer / count / tag tables it does read are real host arrays).
* `split_range` / `chain_products` accept their documented values only.
* The collective verdict (world size 2, gloo): one rank tripped, both report a trip.
* ops.MlpChain(products='exact') answers False from lean_used / split_products at every row count at which an 'auto'
  chain takes the fp16-plane kernels, and asks for no planes and no fragments.
"""
import ctypes
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
A = 0x10000000                    # fake 16-byte aligned device addresses at 1 MiB steps
N = 12 * 64 + 64 + 64 * 32 + 32   # the [12 -> 64 -> 32] net of the pack rows, every matrix followed by its bias


def _adam_args(desc=True, **over):
    """[address of an rlg_adam_desc (desc=False: NULL), guard record]"""
    kw = dict(params=A, grads=A + 0x100000, exp_avg=A + 0x200000, exp_avg_sq=A + 0x300000, n=N,
              norm_partials=A + 0x400000, norm_blocks=4, grad_scale=1.0, max_norm=1.0, lr_slots=A + 0x500000,
              step_counter=A + 0x500100, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, schedule_kind=1,
              kl=A + 0x500200, kl_scale=1.0, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5,
              stats_out=A + 0x500300, skip_flag=None, guard=A + 0x500400)
    assert not set(over) - set(kw)
    kw.update(over)
    guard = kw.pop('guard')
    if not desc:
        return [None, guard]
    from test_optim_entry_errors_cpu import adam_desc
    d = adam_desc(kw)
    _KEEP.append(d)
    return [ctypes.addressof(d), guard]


_KEEP = []                        # the descriptors of the rows stay alive until the table has run


def _pack_side(planes=A + 0x600000, num_layers=2):
    offs = (0, 12 * 64 + 64)
    return [num_layers, (ctypes.c_void_p * 8)(*[A + 4 * o for o in offs]), (ctypes.c_int * 8)(12, 64),
            (ctypes.c_int * 8)(64, 32), planes]


def _scan_args(num=2, record=A + 0x500400, counts=(100, 7), tags=(1, 2), arrays=(A, A + 0x100000), tables=True):
    n = max(len(arrays), 1)
    if not tables:
        return [num, None, None, None, record]
    return [num, (ctypes.c_void_p * n)(*arrays), (ctypes.c_longlong * n)(*counts), (ctypes.c_int * n)(*tags), record]


_MAXIMA = dict(maxima_or_null=A + 0x400000, maxima_stride=64, maxima_rows_per_entry=64, dz_slot=0, x_scale=16.0)


def _dw_args(form, desc=True, **over):
    """[form, address of an rlg_mlp_dw_desc (desc=False: NULL)]: one [64 x 60] layer over 4,096 rows, no maxima"""
    if not desc:
        return [form, None]
    from rl_games_amd._lib import MlpDwDesc
    P, I = ctypes.c_void_p * 1, ctypes.c_int * 1
    kw = dict(num_layers=1, rows=4096, dz=P(A), x=P(A + 0x100000), partial=P(A + 0x200000), grad=P(A + 0x300000),
              out_features=I(64), in_features=I(60), plans4=(ctypes.c_int * 4)(0, 1, 1, 8), grad_scale=1.0)
    kw.update(over)
    for name, ctype in (('dz_slot', ctypes.c_int), ('x_scale', ctypes.c_float)):
        if name in kw:
            kw[name] = (ctype * 1)(kw[name])
    _KEEP.extend(v for v in kw.values() if isinstance(v, ctypes.Array))
    d = MlpDwDesc(**{k: ctypes.addressof(v) if isinstance(v, ctypes.Array) else v for k, v in kw.items()})
    _KEEP.append(d)
    return [form, ctypes.addressof(d)]


def _rows():
    """(id, entry, arguments without the stream)"""
    t = [('range_scan: no record', 'range_scan', _scan_args(record=None)),
         ('range_scan: a record that is not 16-byte aligned', 'range_scan', _scan_args(record=A + 0x500404)),
         ('range_scan: a negative count', 'range_scan', _scan_args(counts=(100, -1))),
         ('range_scan: a count past the 32-bit index word', 'range_scan', _scan_args(counts=(1 << 32, 7))),
         ('range_scan: nine arrays', 'range_scan',
          _scan_args(num=9, counts=(4,) * 9, tags=tuple(range(1, 10)), arrays=tuple(A + 0x1000 * k for k in range(9)))),
         ('range_scan: a negative array count', 'range_scan', _scan_args(num=-1)),
         ('range_scan: a tag of 0', 'range_scan', _scan_args(tags=(1, 0))),
         ('range_scan: a NULL array of 100 elements', 'range_scan', _scan_args(arrays=(0, A))),
         ('range_scan: an array that is not 4-byte aligned', 'range_scan', _scan_args(arrays=(A + 2, A + 0x100000))),
         ('range_scan: arrays without their tables', 'range_scan', _scan_args(tables=False))]
    for entry, tail in (('adam_step_guarded', []), ('adam_pack_guarded', _pack_side())):
        t.append((f'{entry}: NULL descriptor', entry, _adam_args(desc=False) + tail))
        t.append((f'{entry}: no guard record', entry, _adam_args(guard=None) + tail))
        t.append((f'{entry}: no norm partials (nothing to watch)', entry, _adam_args(norm_partials=None, norm_blocks=0) + tail))
        t.append((f'{entry}: n 0', entry, _adam_args(n=0) + tail))
        t.append((f'{entry}: no step counter', entry, _adam_args(step_counter=None) + tail))
        t.append((f'{entry}: adaptive schedule without a KL', entry, _adam_args(kl=None) + tail))
        t.append((f'{entry}: params not 16-byte aligned', entry, _adam_args(params=A + 4) + tail))
    t.append(('adam_pack_guarded: no planes', 'adam_pack_guarded', _adam_args() + _pack_side(planes=None)))
    t.append(('adam_pack_guarded: no layers', 'adam_pack_guarded', _adam_args() + _pack_side(num_layers=0)))
    t.append(('mlp_dw_launch_form: form 3', 'mlp_dw_launch_form', _dw_args(3)))
    t.append(('mlp_dw_launch_form: form -2', 'mlp_dw_launch_form', _dw_args(-2)))
    t.append(('mlp_dw_launch_form: the fp16 form without its maxima', 'mlp_dw_launch_form', _dw_args(2)))
    t.append(('mlp_dw_launch_form: NULL descriptor', 'mlp_dw_launch_form', _dw_args(1, desc=False)))
    # the maxima fields are read only with maxima; a bad one is rejected whatever the form
    for what, bad in (('16 or 64 rows per entry only', dict(maxima_rows_per_entry=32)), ('a stride of 0', dict(maxima_stride=0)),
                      ('a dz slot of 8', dict(dz_slot=8)), ('a negative dz slot', dict(dz_slot=-1)),
                      ('an x scale of 0', dict(x_scale=0.0)), ('an x scale that is NaN', dict(x_scale=float('nan')))):
        t.append((f'mlp_dw_launch_form: maxima, {what}', 'mlp_dw_launch_form', _dw_args(1, **dict(_MAXIMA, **bad))))
    # too few entries for the rows (4,096 rows want 64 entries of 64 rows) count as no maxima
    t.append(('mlp_dw_launch_form: the fp16 form with maxima of too short a stride', 'mlp_dw_launch_form',
              _dw_args(2, **dict(_MAXIMA, maxima_stride=63))))
    # nothing stays armed between calls: maxima of a call that is rejected at its top (no rows) do not serve the next one
    t.append(('mlp_dw_launch_form: the fp16 form without maxima, behind a rejected call that had them', 'mlp_dw_launch_form',
              (_dw_args(2, rows=0, **_MAXIMA), _dw_args(2))))
    return t


def run_table():
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, entry, args in _rows():
        assert name not in codes, name
        for call in (args if isinstance(args, tuple) else (args,)):      # (a tuple: a sequence of calls, the last one answers)
            codes[name] = getattr(lib, 'rlg_' + entry)(*call, None)
    # a scan of nothing is no error and no launch
    codes['range_scan: zero arrays'] = lib.rlg_range_scan(0, None, None, None, A + 0x500400, None)
    return codes


def test_malformed_guard_calls_are_rejected_before_any_launch():
    env = dict(os.environ)
    env['HIP_VISIBLE_DEVICES'] = '-1'            # no device for the child: a row that validation let through by mistake
    env['CUDA_VISIBLE_DEVICES'] = '-1'           # must not reach one
    env.pop('RLG_DW_F16_AMAX_DZ', None)          # (tools only: host-side maxima of the fp16 weight-gradient form)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    assert codes.pop('range_scan: zero arrays') == 0
    names = [name for name, _, _ in _rows()]
    assert len(names) == 38 and set(codes) == set(names)
    wrong = {name: codes[name] for name in names if codes[name] != INVALID}
    assert not wrong, f'rows that were not answered with hipErrorInvalidValue: {wrong}'


def test_policy_keys_take_their_documented_values_only():
    import rl_games_amd
    from rl_games_amd import range_guard as rg
    assert rg.policy_from_config({}) == ('warn', 'auto')
    for policy in ('warn', 'raise', 'exact'):
        for products in ('auto', 'exact'):
            assert rg.policy_from_config({'split_range': policy, 'chain_products': products}) == (policy, products)
    for bad in ({'split_range': 'ignore'}, {'split_range': True}, {'split_range': None}, {'chain_products': 'fp32'},
                {'chain_products': False}, {'split_range': 'exact', 'chain_products': 'split'}):
        with pytest.raises(ValueError):
            rg.policy_from_config(bad)
    assert issubclass(rl_games_amd.SplitRangeError, RuntimeError) and rl_games_amd.SplitRangeError is rg.SplitRangeError
    e = rg.SplitRangeError(rg.describe('rollout', rg.TAG_POLICY, 37, 'auto'), 'rollout', rg.TAG_POLICY, 37)
    assert (e.phase, e.tag, e.index) == ('rollout', rg.TAG_POLICY, 37)
    # the error names the phase, what tripped, where, and the two limits
    for word in ('rollout', 'mus / logits', 'flat index 37', '1023', '4094'):
        assert word in str(e), word
    step = rg.describe('update', rg.TAG_ADAM, 5, 'auto')
    assert 'update' in step and 'optimiser step 5' in step and '1023' in step and '4094' in step
    assert 'inputs' in rg.describe('update', rg.TAG_ADAM, 5, 'exact')


def test_tags_and_limits_have_one_definition_each_side_of_the_c_boundary():
    """The Adam tag is RLG_GUARD_TAG_ADAM of include/rlg_hip.h on the C side and range_guard.TAG_ADAM on the Python side
    (ops.py takes it from there); the two limits are range_guard's."""
    import re
    from rl_games_amd import ops, range_guard as rg
    header = open(os.path.join(ROOT, 'include', 'rlg_hip.h')).read()
    tag = int(re.search(r'#define RLG_GUARD_TAG_ADAM (0x[0-9a-fA-F]+)', header).group(1), 16)
    assert tag == rg.TAG_ADAM == ops.GUARD_TAG_ADAM
    assert (rg.LIMIT_WEIGHT, rg.LIMIT_HIDDEN) == (1023.0, 4094.0)
    assert len({rg.TAG_VALUES, rg.TAG_NEGLOGPS, rg.TAG_POLICY, rg.TAG_CRITIC_VALUES, rg.TAG_RETURNS, rg.TAG_ADAM, 0}) == 7
    assert set(rg.TAG_NAMES) == {rg.TAG_VALUES, rg.TAG_NEGLOGPS, rg.TAG_POLICY, rg.TAG_CRITIC_VALUES, rg.TAG_RETURNS, rg.TAG_ADAM}


def test_verdict_helper_raises_or_hands_back_the_notice():
    """range_guard.verdict on host records: clean - None; tripped - SplitRangeError under 'raise' and on exact products,
    the sentence for the notice under 'exact'."""
    from rl_games_amd import range_guard as rg

    def read(rec):
        return rec
    assert rg.verdict((0, 0), 'rollout', 'raise', 'auto', False, 'cpu', read) is None
    with pytest.raises(rg.SplitRangeError) as e:
        rg.verdict((rg.TAG_RETURNS, 44), 'rollout', 'raise', 'auto', False, 'cpu', read)
    assert (e.value.phase, e.value.tag, e.value.index) == ('rollout', rg.TAG_RETURNS, 44) and 'returns' in str(e.value)
    what = rg.verdict((rg.TAG_ADAM, 9), 'update', 'exact', 'auto', False, 'cpu', read)
    assert 'optimiser step 9' in what and '4094' in what
    with pytest.raises(rg.SplitRangeError, match='inputs'):
        rg.verdict((rg.TAG_ADAM, 9), 'update', 'exact', 'exact', False, 'cpu', read)


# ----------------------------------------------------------------------------- collective verdict

def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _verdict_entry(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from rl_games_amd.range_guard import collective_trip
        got = [collective_trip(False), collective_trip(rank == 1), collective_trip(rank == 0), collective_trip(True)]
        with open(os.path.join(out_dir, f'rank{rank}.json'), 'w') as f:
            json.dump(got, f)
    finally:
        dist.destroy_process_group()


def test_one_tripped_rank_means_every_rank_reports_a_trip(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_verdict_entry, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in (0, 1):
        assert json.load(open(tmp_path / f'rank{rank}.json')) == [False, True, True, True], rank


# ----------------------------------------------------------------------------- MlpChain(products='exact')

class _Lib:
    """Stands in for the host queries of librlg_hip.so that MlpChain's helpers ask (it loads on the CPU, but its chain
    set-up asks the runtime for the kernels' LDS limit): the row thresholds of csrc/mlp_chain.hip - lean 16-row kernels
    below 8,192 rows, the 64-row split kernels from 8,192 (training) / 16,384 (inference)."""

    def rlg_mlp_chain_groups(self, rows, requested, direction):
        if requested:
            return requested
        return 1 if rows < (16384 if direction == 0 else 8192) else 4

    def rlg_mlp_chain_bx_supported(self, n, ins, outs, rows, groups, direction):
        return int(rows >= (16384 if direction == 0 else 8192))


def _chain(monkeypatch, products):
    from rl_games_amd import _lib, ops
    monkeypatch.setattr(_lib, 'load', lambda: _Lib())
    c = ops.MlpChain._from_shape(3, max_groups={0: 4, 1: 4}, frag_bytes=[1024, 1024], weights_version=lambda: 0,
                                 products=products)
    return c


@pytest.mark.parametrize('rows', [16, 4096, 8192, 16384])
def test_exact_products_take_neither_the_lean_nor_the_split_kernels(monkeypatch, rows):
    auto, exact = _chain(monkeypatch, 'auto'), _chain(monkeypatch, 'exact')
    kinds = (0, 1, 2)
    # the 'auto' chain runs every one of these launches on fp16 planes, one way or the other ...
    assert all(auto.lean_used(rows, k) or auto.split_products(rows, k) for k in kinds)
    # ... the 'exact' chain none, and it asks for no derived form of the weights
    assert not any(exact.lean_used(rows, k) or exact.split_products(rows, k) for k in kinds)
    launches = tuple((rows, k) for k in kinds)
    assert exact.forms_read(launches) == (False, False) and auto.forms_read(launches) != (False, False)
    assert exact.adam_pack_target() is None

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f'products=exact asked for {name}')
    from rl_games_amd import _lib
    monkeypatch.setattr(_lib, 'load', lambda: _NoLaunch())
    from rl_games_amd.weight_forms import ChainFormSet, _ChainForms
    ChainFormSet([_ChainForms(exact, launches, None)]).before_replay(rollout=True)          # no pack launch
    state = exact.cache_state()                             # no buffer allocated for planes / fragments
    assert exact.frags.buffer is None and exact.planes.buffer is None and state.products == 'exact'


def test_the_products_mode_travels_with_the_cache_state_and_is_validated(monkeypatch):
    c = _chain(monkeypatch, 'auto')
    c.frags.buffer = c.planes.buffer = object()             # (allocated: cache_state has nothing to do)
    before = c.cache_state()
    assert c.forms_read(((4096, 1),)) == (True, False)
    c.products = 'exact'
    assert c.products == 'exact' and c.forms_read(((4096, 1),)) == (False, False)      # (no stale cached answer)
    c.restore_cache_state(before)
    assert c.products == 'auto' and c.forms_read(((4096, 1),)) == (True, False)
    with pytest.raises(ValueError):
        c.products = 'fp16'
    from rl_games_amd import ops
    assert ops.MlpChain.PRODUCTS == ('auto', 'exact')


def test_weight_gradient_form_names():
    from rl_games_amd import ops
    from rl_games_amd.chain_net import WeightGrads
    assert ops.MlpDwPlan.FORMS == {None: -1, 'auto': -1, 'exact': 0, 'bf16': 1, 'fp16': 2}
    assert WeightGrads().form is None


if __name__ == '__main__':
    print(json.dumps(run_table()))
