"""CPU: what rlg_adam_step and rlg_adam_step_pack answer to malformed calls.

Both take the step as an rlg_adam_desc, validate it and their own arguments on the host and return hipErrorInvalidValue
(1) before they ask the HIP runtime for anything, so the answers do not depend on a device being there.  Every row below
differs from a well-formed call in one argument or descriptor field, or passes no descriptor at all.  The pointers are
small fake aligned addresses - the host code dereferences none of them (the pack form reads the `weights`, `in_features`
and `out_features` tables, which are real host arrays).

As in tests/test_chain_entry_errors_cpu.py the table runs in a child process that sees no GPU: should a row ever get
past validation, its launch fails there instead of handing fake addresses to a device.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = 1
MAX_LAYERS = 8                    # kChainMaxLayers
ARENA = 0x10000000                # params; grads, exp_avg, exp_avg_sq follow at 1 MiB steps
IN, OUT = (12, 100, 52), (100, 52, 22)
N = sum(i * o + o for i, o in zip(IN, OUT))


def _base():
    return dict(params=ARENA, grads=ARENA + 0x100000, exp_avg=ARENA + 0x200000, exp_avg_sq=ARENA + 0x300000, n=N,
                norm_partials=ARENA + 0x400000, norm_blocks=4, grad_scale=1.0, max_norm=1.0, lr_slots=ARENA + 0x500000,
                step_counter=ARENA + 0x500100, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, schedule_kind=1,
                kl=ARENA + 0x500200, kl_scale=1.0, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5,
                stats_out=ARENA + 0x500300, skip_flag=None)


def adam_desc(kw):
    """_lib.AdamDesc from a dict keyed like _base() (the `_or_null` of a field name left off)"""
    from rl_games_amd import _lib
    fields = [f for f, _ in _lib.AdamDesc._fields_]
    assert {f.replace('_or_null', '') for f in fields} == set(kw), sorted(kw)
    return _lib.AdamDesc(**{f: kw[f.replace('_or_null', '')] for f in fields})


def _offsets(ins=IN, outs=OUT):
    """element offsets of the matrices in _net's layout: every weight matrix followed by its bias"""
    offs, off = [], 0
    for i, o in zip(ins, outs):
        offs.append(off)
        off += i * o + o
    return offs


def _pack_side(ins=IN, outs=OUT, offsets=None, num_layers=None, planes=ARENA + 0x600000):
    n = len(ins)
    offsets = _offsets(ins, outs) if offsets is None else offsets
    return dict(num_layers=n if num_layers is None else num_layers,
                weights=(ctypes.c_void_p * MAX_LAYERS)(*[ARENA + 4 * o for o in offsets]),
                in_features=(ctypes.c_int * MAX_LAYERS)(*ins), out_features=(ctypes.c_int * MAX_LAYERS)(*outs),
                planes=planes)


def _rows():
    """(id, entry, overrides of the descriptor's fields - None: no descriptor -, overrides of the pack arguments)"""
    t = []
    for entry in ('adam_step', 'adam_step_pack'):
        t.append((f'{entry}: NULL descriptor', entry, None, {}))
        t.append((f'{entry}: n 0', entry, dict(n=0), {}))
        t.append((f'{entry}: n negative', entry, dict(n=-N), {}))
        t.append((f'{entry}: no step counter', entry, dict(step_counter=None), {}))
        t.append((f'{entry}: adaptive schedule without a KL', entry, dict(kl=None), {}))
        for arena in ('params', 'grads', 'exp_avg', 'exp_avg_sq'):
            t.append((f'{entry}: {arena} not 16-byte aligned', entry, {arena: _base()[arena] + 4}, {}))
    offs = _offsets()
    p = 'adam_step_pack: '
    t.append((p + 'no layers', 'adam_step_pack', {}, dict(num_layers=0)))
    t.append((p + 'more layers than kChainMaxLayers', 'adam_step_pack', {}, dict(num_layers=MAX_LAYERS + 1)))
    t.append((p + 'no planes', 'adam_step_pack', {}, dict(planes=None)))
    t.append((p + 'a weight offset not divisible by 4', 'adam_step_pack', {}, dict(offsets=[offs[0], offs[1] + 2, offs[2]])))
    t.append((p + 'in_features not divisible by 4', 'adam_step_pack', dict(n=10 * 100 + 100 + 100 * 52 + 52 + 52 * 22 + 22),
              dict(ins=(10, 100, 52), offsets=_offsets((10, 100, 52), OUT))))
    t.append((p + 'overlapping matrices', 'adam_step_pack', {}, dict(offsets=[offs[0], offs[0] + 8, offs[2]])))
    t.append((p + 'a matrix in front of the arena', 'adam_step_pack', {}, dict(offsets=[-4, offs[1], offs[2]])))
    t.append((p + 'a matrix that ends behind the arena', 'adam_step_pack', dict(n=N - 24), {}))
    return t


def run_table():
    """{row id: code} of the library that rl_games_amd._lib selects"""
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, entry, over, pack_over in _rows():
        assert name not in codes, name
        desc = None
        if over is not None:
            kw = _base()
            assert not set(over) - set(kw)
            kw.update(over)
            desc = adam_desc(kw)
        args = [None if desc is None else ctypes.addressof(desc)]
        if entry == 'adam_step_pack':
            side = _pack_side(**pack_over)
            args += [side[k] for k in ('num_layers', 'weights', 'in_features', 'out_features', 'planes')]
        codes[name] = getattr(lib, 'rlg_' + entry)(*args, None)
    return codes


def test_malformed_optimiser_calls_are_rejected_before_any_launch():
    env = dict(os.environ)
    env['HIP_VISIBLE_DEVICES'] = '-1'            # no device for the child: a row that validation let through by mistake
    env['CUDA_VISIBLE_DEVICES'] = '-1'           # must not reach one
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    names = [name for name, _, _, _ in _rows()]
    assert len(names) == 26 and set(codes) == set(names)
    wrong = {name: codes[name] for name in names if codes[name] != INVALID}
    assert not wrong, f'rows that were not answered with hipErrorInvalidValue: {wrong}'


if __name__ == '__main__':
    print(json.dumps(run_table()))
