"""CPU: what the six launching entry points of the fused MLP chain answer to malformed calls.

rlg_mlp_chain_forward / _backward / _step and their _lean forms validate their arguments on the host, in a fixed order:
the order decides which code a doubly wrong call gets, and the callers in ops.MlpChain tell hipErrorNotSupported (801:
"use the other engine") from hipErrorInvalidValue (1: a bug).  Every row below is rejected before the entry asks the
HIP runtime for anything, so the answers do not depend on a device being there; the rows of the two step entries stop
in front of their device query for that reason.  The pointers are small fake aligned addresses - the host code
dereferences none of them.

The table runs in a child process that sees no GPU: should a row ever get past validation, its launch fails there
instead of handing fake addresses to a device.  `python tests/test_chain_entry_errors_cpu.py` prints the codes of the
library that RLG_HIP_LIB selects (one JSON object), which is how two builds are compared.

The expected values are the answers of the library before the entry points shared their argument setup, and before
their arguments travelled as descriptors (rlg_chain_net / _fwd / _bwd / _launch of include/rlg_hip.h): the rows name
descriptor fields.  What a backward call answers to gradient maxima depends on that call's descriptor alone.

The two stand-alone loss entries take the same kind of descriptor (rlg_ppo_loss_fused the chain's own) and are asked
beside them, in the same child: no descriptor, and what rlg_ppo_loss_fused itself rejects.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, NOT_SUPPORTED = 1, 801
MAX_LAYERS = 8                    # kChainMaxLayers
ROWS = 64
IN = (24, 64, 64)
OUT = (64, 64, 5)
ACTS = (1, 1, 0)                  # ELU, ELU, identity


def _addr(k):
    return 0x100000 * (k + 1)     # 16-byte aligned, never dereferenced


def _ptrs(base, n=MAX_LAYERS + 1, null=(), offset=None):
    v = [0 if L in null else _addr(base + L) for L in range(n)]
    for L, d in (offset or {}).items():
        v[L] += d
    return (ctypes.c_void_p * n)(*v)


def _ints(values, n=MAX_LAYERS + 1):
    v = list(values) + [values[-1]] * (n - len(values))
    return (ctypes.c_int * n)(*v)


def _lls(values, n=MAX_LAYERS + 1):
    v = list(values) + [values[-1]] * (n - len(values))
    return (ctypes.c_longlong * n)(*v)


def _desc(**over):
    from rl_games_amd._lib import PpoLossDesc
    d = PpoLossDesc()
    for k, name in enumerate(('mu', 'logstd', 'values', 'actions', 'old_neglogp', 'advantages', 'old_values', 'returns',
                              'old_mu', 'old_sigma', 'd_mu', 'd_values', 'partials')):
        setattr(d, name, _addr(200 + k))
    d.minibatch, d.actions_num = ROWS, 4
    d.ld_mu = d.ld_values = d.ld_d_mu = d.ld_d_values = 5
    d.e_clip, d.critic_coef, d.bounds_coef = 0.2, 1.0, 0.0
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _shape(n=3, ins=IN, outs=OUT):
    return dict(num_layers=n, in_features=_ints(ins), out_features=_ints(outs), acts=_ints(ACTS))


def _wide():
    """a hidden layer of 20,480 units: beyond the LDS tiles of the exact-product kernels and the lean fragment format"""
    return _shape(ins=(24, 64, 20480), outs=(64, 20480, 5))


# the fold of the normaliser state must publish into a second buffer set
_RMS = dict(rms_mean_or_null=_addr(300), rms_var=_addr(301), rms_batch_or_null=_addr(302), rms_count=_addr(303),
            rms_mean_out=_addr(304), rms_var_out=_addr(305), rms_count_out=_addr(306))

# the descriptors each entry takes, in argument order (include/rlg_hip.h), in front of the stream
_ENTRIES = {'forward': ('net', 'fwd', 'launch'), 'backward': ('net', 'bwd', 'launch'),
            'step': ('net', 'fwd', 'bwd', 'launch'), 'forward_lean': ('net', 'fwd', 'launch'),
            'backward_lean': ('net', 'bwd', 'launch'), 'step_lean': ('net', 'fwd', 'bwd', 'launch')}


def _well_formed(entry):
    """{descriptor: {field: value}} of a well-formed call of `entry` - which is never made as it stands"""
    lean, step = entry.endswith('_lean'), entry.startswith('step')
    d = dict(net=dict(_shape(), weights=None if lean else _ptrs(0), biases=None if 'backward' in entry else _ptrs(20)),
             launch=dict(rows=ROWS, groups=0))
    if 'fwd' in _ENTRIES[entry]:
        d['fwd'] = dict(act_out=_ptrs(40), act_ld=_lls(OUT), x=_addr(60), ldx=IN[0], rms_eps=1e-5,
                        weight_form_or_null=_addr(400) if lean else None)
    if 'bwd' in _ENTRIES[entry]:
        d['bwd'] = dict(act_in=None if step else _ptrs(40), act_ld=None if step else _lls(OUT), d_out=_addr(80),
                        ld_dout=OUT[-1], dz_out=_ptrs(100), dz_ld=_lls(OUT), ppo_loss_or_null=_desc() if step else None,
                        weight_form_or_null=_addr(401) if lean else None)
    return d


_LOSS_ENTRIES = ('ppo_loss_fused', 'ppo_loss_finalize')      # (descriptor, stream)


def _call(lib, entry, **over):
    """Overrides are descriptor fields (fwd_<field> / bwd_<field> where an entry has the field in both halves), or a
    descriptor's own name with None: that descriptor is passed as NULL."""
    if entry in _LOSS_ENTRIES:
        desc = over['desc']
        return getattr(lib, 'rlg_' + entry)(None if desc is None else ctypes.byref(desc), None)
    from rl_games_amd import _lib
    classes = dict(net=_lib.ChainNet, fwd=_lib.ChainFwd, bwd=_lib.ChainBwd, launch=_lib.ChainLaunch)
    fields = _well_formed(entry)
    for key, v in over.items():
        if key in fields:
            assert v is None, key
            fields[key] = None
            continue
        side, _, name = key.partition('_')
        if side in ('fwd', 'bwd') and side in fields and name in dict(classes[side]._fields_):
            hit = [(side, name)]
        else:
            hit = [(d, key) for d in _ENTRIES[entry] if key in dict(classes[d]._fields_)]
        assert len(hit) == 1, (entry, key, hit)
        fields[hit[0][0]][hit[0][1]] = v
    keep, args = [], []
    for d in _ENTRIES[entry]:
        if fields[d] is None:
            args.append(None)
            continue
        desc = classes[d]()
        for name, v in fields[d].items():
            if isinstance(v, (ctypes.Array, ctypes.Structure)):      # (arrays, the loss descriptor: by address)
                keep.append(v)
                v = ctypes.addressof(v)
            setattr(desc, name, v)
        keep.append(desc)
        args.append(ctypes.byref(desc))
    return getattr(lib, 'rlg_mlp_chain_' + entry)(*args, None)


_BIG_LOSS = dict(actions_num=2000)        # a loss tile beyond the LDS of every backward kernel
_H_ODD_LD = dict(act_ld=_lls((63, 64, 5)))      # layer 0: rows of H that are not 16-byte accesses


def _rows():
    """(id, expected code, entry, overrides); a row whose entry is a tuple runs a sequence and expects a list of codes."""
    t = []

    def row(name, expected, entry, **over):
        t.append((name, expected, entry, over))

    for e in _ENTRIES:
        row(f'{e}: rows 0', 0, e, rows=0)
    # ---- layer table (chain_fill / chain_fill_shape)
    for e in ('forward', 'backward', 'forward_lean', 'backward_lean'):
        row(f'{e}: no layers', INVALID, e, num_layers=0)
        row(f'{e}: more layers than kChainMaxLayers', INVALID, e, num_layers=MAX_LAYERS + 1)
        row(f'{e}: in of layer 1 is not out of layer 0', INVALID, e, **_shape(ins=(24, 48, 64)))
        row(f'{e}: a layer of width 0', INVALID, e, **_shape(ins=(24, 0, 64), outs=(0, 64, 5)))
    for e in ('backward', 'backward_lean'):
        row(f'{e}: one layer', INVALID, e, num_layers=1)
    for e in ('forward', 'backward'):
        row(f'{e}: a weight matrix that is not 4-byte aligned', INVALID, e, weights=_ptrs(0, offset={1: 2}))
        row(f'{e}: a hidden layer too wide for LDS', INVALID, e, **_wide())
    for e in ('forward_lean', 'backward_lean'):
        row(f'{e}: a hidden layer outside the fragment format', NOT_SUPPORTED, e, **_wide())
    # ---- forward side
    for e in ('forward', 'forward_lean'):
        row(f'{e}: no output array of the last layer', INVALID, e, act_out=_ptrs(40, null=(2,)))
        row(f'{e}: normaliser fold into the buffers it reads', INVALID, e, **dict(_RMS, rms_mean_out=_RMS['rms_mean_or_null']))
        row(f'{e}: normaliser fold into the count it reads', INVALID, e, **dict(_RMS, rms_count_out=_RMS['rms_count']))
        row(f'{e}: normaliser fold without a count', INVALID, e, **dict(_RMS, rms_count=None))
    row('forward_lean: no fragments', INVALID, 'forward_lean', weight_form_or_null=None)
    row('forward_lean: fragments that are not 4-byte aligned', INVALID, 'forward_lean', weight_form_or_null=_addr(400) + 2)
    row('forward_lean: a bias vector that is not 4-byte aligned', INVALID, 'forward_lean', biases=_ptrs(20, offset={1: 2}))
    row('forward_lean: no fragments AND outside the fragment format', INVALID, 'forward_lean', weight_form_or_null=None,
        **_wide())
    row('forward_lean: outside the fragment format AND no output array of the last layer', NOT_SUPPORTED, 'forward_lean',
        act_out=_ptrs(40, null=(2,)), **_wide())
    # ---- backward side
    for e in ('backward', 'backward_lean'):
        row(f'{e}: no dZ array of a hidden layer', INVALID, e, dz_out=_ptrs(100, null=(1,)))
        row(f'{e}: no H array of a hidden layer', INVALID, e, act_in=_ptrs(40, null=(0,)))
        row(f'{e}: descriptor of another minibatch size', INVALID, e, ppo_loss_or_null=_desc(minibatch=ROWS + 1))
        row(f'{e}: descriptor without actions', INVALID, e, ppo_loss_or_null=_desc(actions_num=0))
        row(f'{e}: descriptor with a mask and no mask sum', INVALID, e, ppo_loss_or_null=_desc(mask_or_null=_addr(250)))
        row(f'{e}: descriptor without partials', INVALID, e, ppo_loss_or_null=_desc(partials=None))
        row(f'{e}: descriptor without d_mu', INVALID, e, ppo_loss_or_null=_desc(d_mu=None))
    row('backward: a loss tile beyond LDS', INVALID, 'backward', ppo_loss_or_null=_desc(**_BIG_LOSS))
    row('backward_lean: a loss tile beyond LDS', NOT_SUPPORTED, 'backward_lean', ppo_loss_or_null=_desc(**_BIG_LOSS))
    row('backward_lean: no fragments', INVALID, 'backward_lean', weight_form_or_null=None)
    row('backward_lean: fragments that are not 4-byte aligned', INVALID, 'backward_lean', weight_form_or_null=_addr(401) + 2)
    row('backward_lean: row stride of H not a multiple of 4', NOT_SUPPORTED, 'backward_lean', **_H_ODD_LD)
    row('backward_lean: row stride of dZ not a multiple of 4', NOT_SUPPORTED, 'backward_lean', dz_ld=_lls((64, 66, 5)))
    row('backward_lean: H not 16-byte aligned', NOT_SUPPORTED, 'backward_lean', act_in=_ptrs(40, offset={1: 4}))
    row('backward_lean: dZ not 16-byte aligned', NOT_SUPPORTED, 'backward_lean', dz_out=_ptrs(100, offset={0: 8}))
    row('backward_lean: row stride of H of 2^20', NOT_SUPPORTED, 'backward_lean', act_ld=_lls((1 << 20, 64, 5)))
    row('backward_lean: hidden width not a multiple of 4', NOT_SUPPORTED, 'backward_lean',
        **_shape(ins=(24, 62, 64), outs=(62, 64, 5)))
    # the hidden layers are checked one after the other, each for missing arrays first
    row('backward_lean: layer 0 rows not 16-byte AND no dZ of layer 1', NOT_SUPPORTED, 'backward_lean',
        dz_out=_ptrs(100, null=(1,)), **_H_ODD_LD)
    row('backward_lean: no dZ of layer 0 AND layer 1 rows not 16-byte', INVALID, 'backward_lean',
        dz_out=_ptrs(100, null=(0,)), act_ld=_lls((64, 63, 5)))
    row('backward_lean: rows not 16-byte AND a bad descriptor', NOT_SUPPORTED, 'backward_lean',
        ppo_loss_or_null=_desc(actions_num=0), **_H_ODD_LD)
    row('backward_lean: outside the fragment format AND no dZ', NOT_SUPPORTED, 'backward_lean',
        dz_out=_ptrs(100, null=(0,)), **_wide())
    # ---- the one-launch steps, up to their device query
    for e in ('step', 'step_lean'):
        row(f'{e}: no layers', NOT_SUPPORTED, e, num_layers=0)
        row(f'{e}: one layer', NOT_SUPPORTED, e, num_layers=1)
        row(f'{e}: no descriptor', NOT_SUPPORTED, e, ppo_loss_or_null=None)
    row('step: a minibatch of the 64-row kernels', NOT_SUPPORTED, 'step', rows=16384, ppo_loss_or_null=_desc(minibatch=16384))
    row('step_lean: no forward fragments', NOT_SUPPORTED, 'step_lean', fwd_weight_form_or_null=None)
    row('step_lean: no backward fragments', NOT_SUPPORTED, 'step_lean', bwd_weight_form_or_null=None)
    # ---- the stand-alone loss launches
    for e in _LOSS_ENTRIES:
        row(f'{e}: NULL descriptor', INVALID, e, desc=None)
    row('ppo_loss_fused: minibatch 0', INVALID, 'ppo_loss_fused', desc=_desc(minibatch=0))
    row('ppo_loss_fused: descriptor without actions', INVALID, 'ppo_loss_fused', desc=_desc(actions_num=0))
    row('ppo_loss_fused: descriptor with a mask and no mask sum', INVALID, 'ppo_loss_fused',
        desc=_desc(mask_or_null=_addr(250)))
    row('ppo_loss_fused: a loss tile beyond LDS', INVALID, 'ppo_loss_fused', desc=_desc(**_BIG_LOSS))
    # ---- a NULL descriptor: answered first, in front of the early return for no rows
    for e, descs in _ENTRIES.items():
        for d in descs:
            row(f'{e}: NULL {d} descriptor', INVALID, e, **({d: None} if d == 'launch' else {d: None, 'rows': 0}))
    # ---- gradient maxima are asked for in the call's own backward descriptor.  The lean backward looks at them behind
    # its rows check and its loss descriptor: too few entries per tensor (stride 1 for 4 workgroups) is
    # hipErrorInvalidValue, in front of the LDS check that answers 801.
    big = dict(ppo_loss_or_null=_desc(**_BIG_LOSS))
    short = dict(maxima_or_null=_addr(500), maxima_stride=1)
    row('backward_lean: maxima with too few entries AND a loss tile beyond LDS', INVALID, 'backward_lean', **big, **short)
    row('backward_lean: the same call without maxima', NOT_SUPPORTED, 'backward_lean', **big)
    row('backward_lean: maxima with too few entries AND rows not 16-byte', NOT_SUPPORTED, 'backward_lean', **_H_ODD_LD,
        **short)
    row('backward_lean: maxima with too few entries AND a bad descriptor', INVALID, 'backward_lean',
        ppo_loss_or_null=_desc(actions_num=0), **short)
    # nothing is carried from call to call: each call of a sequence gets the code of its own descriptor
    t.append(('backward_lean: with short maxima, without, with again', [INVALID, NOT_SUPPORTED, INVALID],
              (('backward_lean', dict(big, **short)), ('backward_lean', big), ('backward_lean', dict(big, **short))), None))
    return t


def run_table():
    """{row id: code} of the library that rl_games_amd._lib selects; a row whose entry is a tuple runs a sequence of calls
    and answers the list of their codes"""
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, _, entry, over in _rows():
        assert name not in codes, name
        if isinstance(entry, str):
            codes[name] = _call(lib, entry, **over)
        else:
            codes[name] = [_call(lib, step_entry, **step_over) for step_entry, step_over in entry]
    return codes


def test_malformed_chain_calls_get_the_codes_they_always_got():
    env = dict(os.environ)
    # no device for the child: a row that validation let through by mistake must not reach one
    env['HIP_VISIBLE_DEVICES'] = '-1'
    env['CUDA_VISIBLE_DEVICES'] = '-1'
    for k in [k for k in env if k.startswith('RLG_CHAIN_')]:
        del env[k]                                           # (the engine switches change which check answers first)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    expected = {name: code for name, code, _, _ in _rows()}
    assert len(expected) >= 80
    wrong = {name: (codes.get(name), code) for name, code in expected.items() if codes.get(name) != code}
    assert not wrong, f'(got, expected) per row: {wrong}'
    assert set(codes) == set(expected)


if __name__ == '__main__':
    print(json.dumps(run_table()))
