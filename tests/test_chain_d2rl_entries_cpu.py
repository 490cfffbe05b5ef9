"""CPU: what the entries of csrc/mlp_chain_d2rl.hip answer on the host.  Malformed calls - a NULL descriptor, a shape that
breaks in[l] == out[l-1] + in[0], no rows - are hipErrorInvalidValue, a net or a descriptor field outside the envelope
hipErrorNotSupported; rlg_mlp_chain_d2rl_supported is host arithmetic.  The table runs in a child process that sees no
GPU (the pattern of tests/test_chain_entry_errors_cpu.py): a row that got past validation could not reach a device."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 801
OBS = 60
D2RL = ((OBS, 256 + OBS, 128 + OBS, 64), (256, 128, 64, 9), (1, 1, 1, 0))        # [256, 128, 64] elu over 60 observations


_addr = lambda k: 0x100000 * (k + 1)     # noqa: E731  (16-byte aligned, never dereferenced)


def _call(lib, entry, ins=D2RL[0], outs=D2RL[1], acts=D2RL[2], rows=64, null=None, cat=OBS, **fields):
    from rl_games_amd import _lib
    n = len(ins)
    ints, ptrs, lls = ctypes.c_int * n, ctypes.c_void_p * n, ctypes.c_longlong * n
    arrays = [ptrs(*[_addr(k) for k in range(n)]), ptrs(*[_addr(20 + k) for k in range(n)]), ints(*ins), ints(*outs), ints(*acts),
              ptrs(*[_addr(40 + k) for k in range(n)]), lls(*[o + cat for o in outs]), ptrs(*[_addr(60 + k) for k in range(n)]),
              lls(*outs)]
    at = [ctypes.addressof(a) for a in arrays]
    net = _lib.ChainNet(n, *at[:5])
    if entry == 'supported':
        return lib.rlg_mlp_chain_d2rl_supported(ctypes.byref(net), None, rows, fields.get('direction', 0))
    if entry == 'forward':
        half = _lib.ChainFwd(act_out=at[5], act_ld=at[6], x=_addr(80), ldx=ins[0], rms_eps=1e-5)
    else:
        half = _lib.ChainBwd(act_in=at[5], act_ld=at[6], d_out=_addr(81), ld_dout=outs[-1], dz_out=at[7], dz_ld=at[8])
    for k, v in fields.items():
        setattr(half, k, v)
    descs = dict(net=net, half=half, launch=_lib.ChainLaunch(rows, 0))
    args = [None if k == null else ctypes.byref(d) for k, d in descs.items()]
    return getattr(lib, 'rlg_mlp_chain_d2rl_' + entry)(*args, None)


def _rows():
    plain = dict(ins=(OBS, 256, 128, 64))                            # a sequential trunk: not a D2RL shape
    t = {}
    for e in ('forward', 'backward'):
        for d in ('net', 'half', 'launch'):
            t[f'{e}: NULL {d} descriptor'] = (INVALID, e, dict(null=d))
        t[f'{e}: a plain shape'] = (INVALID, e, plain)
        t[f'{e}: no rows'] = (INVALID, e, dict(rows=0))
        t[f'{e}: one hidden layer'] = (NOT_SUPPORTED, e, dict(ins=(OBS, 64), outs=(64, 9), acts=(1, 0)))
        t[f'{e}: width 516'] = (NOT_SUPPORTED, e, dict(ins=(OBS, 516 + OBS, 516), outs=(516, 516, 9), acts=(1, 1, 0)))
        t[f'{e}: a weight form'] = (NOT_SUPPORTED, e, dict(weight_form_or_null=_addr(90)))
    t['forward: a concat row stride without room for the observations'] = (INVALID, 'forward', dict(cat=0))
    t['backward: gradient maxima'] = (NOT_SUPPORTED, 'backward', dict(maxima_or_null=_addr(91), maxima_stride=8))
    # the query: the groups a launch runs (2 from 8,192 rows, 4 from 16,384, while two workgroups fit a CU's LDS), 0 outside
    t['supported: the bench shape, 16 rows'] = (1, 'supported', {})
    t['supported: 32,768 rows, 112 KiB at four groups'] = (2, 'supported', dict(rows=32768, direction=2))
    t['supported: [64, 32] at 32,768 rows'] = (4, 'supported', dict(ins=(OBS, 64 + OBS, 32), outs=(64, 32, 9), acts=(1, 1, 0), rows=32768))
    t['supported: four layers of 512'] = (1, 'supported', dict(ins=(12, 524, 524, 524, 512), outs=(512, 512, 512, 512, 3), acts=(1, 1, 1, 1, 0), rows=32768, direction=1))
    t['supported: a plain shape'] = (0, 'supported', plain)
    t['supported: width 6'] = (0, 'supported', dict(ins=(OBS, 6 + OBS, 6), outs=(6, 6, 9), acts=(1, 1, 0)))
    t['supported: 2,600 observations'] = (0, 'supported', dict(ins=(2600, 2664, 32), outs=(64, 32, 9), acts=(1, 1, 0)))
    return t


def test_d2rl_entries_answer_on_the_host():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    wrong = {name: (codes.get(name), want) for name, (want, _, _) in _rows().items() if codes.get(name) != want}
    assert not wrong, f'(got, expected) per row: {wrong}'


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib as lib_module
    print(json.dumps({name: _call(lib_module.load(), entry, **over) for name, (_, entry, over) in _rows().items()}))
