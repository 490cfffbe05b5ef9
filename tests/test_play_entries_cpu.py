"""CPU: the players' entry points (csrc/play.hip) at the boundary, and the player's choice of path.

The five symbols are exported and bound; every malformed call listed in include/rlg_hip.h is answered on the host -
hipErrorInvalidValue, more than 16 branches hipErrorNotSupported - before the runtime is asked for anything; rows == 0
returns 0.  The table runs in a child process that sees no GPU, as tests/test_rnn_pair_cpu.py does: the pointers are
small fake addresses the host code dereferences none of, and one well-formed call per entry shows the runtime's own
code, which is not hipErrorInvalidValue.

The player's host logic runs on CPU tensors over a recording stand-in for the library (the technique of
tests/test_weight_forms_cpu.py): without `player.fused` no rlg_play_* name is called, and a network outside the engines
prints the notice and calls none either.
"""
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, NOT_SUPPORTED = 1, 801
ENTRIES = ('rlg_play_policy_head', 'rlg_play_categorical_head', 'rlg_play_post_step_num_blocks', 'rlg_play_post_step',
           'rlg_play_fold')
P = [0x100000 * (k + 1) for k in range(8)]            # fake aligned addresses


def _head(**o):
    a = dict(heads=P[0], ld_heads=4, mu_col=1, logstd=P[1], noise=P[2], low=P[3], high=P[4], out=P[5], rows=5, A=3)
    a.update(o)
    return ('rlg_play_policy_head', [a[k] for k in ('heads', 'ld_heads', 'mu_col', 'logstd', 'noise', 'low', 'high', 'out',
                                                    'rows', 'A')] + [None])


def _cat(**o):
    a = dict(logits=P[0], ld_logits=7, sizes=[3, 4], noise=P[1], masks=P[2], ld_masks=7, out=P[3], rows=5)
    a.update(o)
    sizes = a['sizes']
    arr = None if sizes is None else sizes
    return ('rlg_play_categorical_head', [a['logits'], a['ld_logits'], arr, a.get('B', 0 if sizes is None else len(sizes)),
                                          a['noise'], a['masks'], a['ld_masks'], a['out'], a['rows'], None])


def _post(**o):
    a = dict(rewards=P[0], ld=1, dones=P[1], cur_r=P[2], cur_n=P[3], slot=P[4], rows=5)
    a.update(o)
    return ('rlg_play_post_step', [a[k] for k in ('rewards', 'ld', 'dones', 'cur_r', 'cur_n', 'slot', 'rows')] + [None])


def _fold(**o):
    a = dict(partials=P[0], slots=2, blocks=3, limit=10, totals=P[1])
    a.update(o)
    return ('rlg_play_fold', [a[k] for k in ('partials', 'slots', 'blocks', 'limit', 'totals')] + [None])


def _rows():
    """(id, (entry, args), expected code; None: reaches the runtime, whose code is its own and not INVALID)"""
    t = [('head: well formed', _head(), None), ('head: deterministic, no logstd', _head(noise=None, logstd=None), None),
         ('head: no bounds', _head(low=None, high=None), None),
         ('head: rows 0', _head(rows=0), 0), ('head: rows < 0', _head(rows=-1), INVALID),
         ('head: no heads', _head(heads=None), INVALID), ('head: no output', _head(out=None), INVALID),
         ('head: noise without logstd', _head(logstd=None), INVALID),
         ('head: A = 0', _head(A=0), INVALID), ('head: A < 0', _head(A=-2), INVALID),
         ('head: ld 0', _head(ld_heads=0), INVALID), ('head: ld below the columns read', _head(ld_heads=3), INVALID),
         ('head: mu_col < 0', _head(mu_col=-1), INVALID),
         ('head: low without high', _head(high=None), INVALID), ('head: high without low', _head(low=None), INVALID),
         ('cat: well formed', _cat(), None), ('cat: arg-max, no masks', _cat(noise=None, masks=None), None),
         ('cat: 16 branches', _cat(sizes=[2] * 16, ld_logits=32, ld_masks=32), None),
         ('cat: rows 0', _cat(rows=0), 0), ('cat: rows < 0', _cat(rows=-4), INVALID),
         ('cat: no logits', _cat(logits=None), INVALID), ('cat: no output', _cat(out=None), INVALID),
         ('cat: no branch sizes', _cat(sizes=None, B=2), INVALID), ('cat: no branches', _cat(sizes=[], B=0), INVALID),
         ('cat: 17 branches', _cat(sizes=[2] * 17, ld_logits=34, ld_masks=34), NOT_SUPPORTED),
         ('cat: branch size 0', _cat(sizes=[3, 0]), INVALID), ('cat: branch size < 0', _cat(sizes=[-1, 4]), INVALID),
         ('cat: ld_logits 0', _cat(ld_logits=0), INVALID), ('cat: ld_logits below the columns', _cat(ld_logits=6), INVALID),
         ('cat: ld_masks 0', _cat(ld_masks=0), INVALID), ('cat: ld_masks below the columns', _cat(ld_masks=6), INVALID),
         ('post: well formed', _post(), None), ('post: rows 0', _post(rows=0), 0), ('post: rows < 0', _post(rows=-1), INVALID),
         ('post: ld 0', _post(ld=0), INVALID)]
    t += [(f'post: no {k}', _post(**{k: None}), INVALID) for k in ('rewards', 'dones', 'cur_r', 'cur_n', 'slot')]
    t += [('fold: well formed', _fold(), None), ('fold: slots 0', _fold(slots=0), 0), ('fold: slots < 0', _fold(slots=-1), INVALID),
          ('fold: blocks 0', _fold(blocks=0), INVALID), ('fold: no partials', _fold(partials=None), INVALID),
          ('fold: no totals', _fold(totals=None), INVALID)]
    return t


def run_table():
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, (entry, args), _ in _rows():
        assert name not in codes, name
        args = [(ctypes.c_int * max(len(a), 1))(*a) if isinstance(a, list) else a for a in args]
        codes[name] = getattr(lib, entry)(*args)
    return codes


def test_the_entries_are_exported_and_bound():
    from rl_games_amd import _lib
    lib, table = _lib.load(), _lib.exported_prototypes()
    for name in ENTRIES:
        assert name in table and hasattr(lib, name), name


def test_malformed_play_calls_are_rejected_on_the_host():
    env = dict(os.environ)
    env['HIP_VISIBLE_DEVICES'] = '-1'             # no device for the child: nothing that got past validation reaches one
    env['CUDA_VISIBLE_DEVICES'] = '-1'
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    rows = _rows()
    assert set(codes) == {r[0] for r in rows}
    wrong = {name: codes[name] for name, _, want in rows
             if (codes[name] != want if want is not None else codes[name] in (0, INVALID, NOT_SUPPORTED))}
    assert not wrong, f'codes against the table: {wrong}'


def test_post_step_blocks_are_positive_and_monotone():
    from rl_games_amd import _lib
    lib = _lib.load()
    blocks = [lib.rlg_play_post_step_num_blocks(rows) for rows in (1, 64, 65, 65536)]
    assert all(b > 0 for b in blocks) and blocks == sorted(blocks), blocks
    assert blocks[-1] > blocks[0]


# ----------------------------------------------------------------------------- the player's choice of path

class _Recorder:
    """Stands in for librlg_hip.so: every entry answers 0 and is recorded by name."""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        if not name.startswith('rlg_'):
            raise AttributeError(name)

        def entry(*args):
            self.names.append(name)
            return 0
        return entry


def _cpu_player(monkeypatch, capsys, player_config, **network):
    from rl_games_amd import _lib, configs, player
    fake = _Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: fake)
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, what: None)
    monkeypatch.setattr(_lib, 'stream_handle', lambda device=None: 0)
    monkeypatch.setattr(player, '_require_hip', lambda device: None)
    torch.manual_seed(3)
    params = configs.tiny(num_actors=8, device='cpu', normalize_input=False, normalize_value=False)
    params['network'].update({k: v for k, v in network.items() if k != 'fixed_sigma'})
    if 'fixed_sigma' in network:
        params['network']['space']['continuous']['fixed_sigma'] = network['fixed_sigma']
    params['config']['player'] = dict(player_config, games_num=4, print_stats=False)
    p = player.PpoPlayerContinuous(params)
    p.has_batch_dimension = True
    p.batch_size = 8
    p.init_rnn()
    for det in (True, False, True):
        act = p.get_action(torch.randn(8, 12), is_deterministic=det)
        assert tuple(act.shape) == (8, 3) and torch.isfinite(act).all()
    return p, fake, capsys.readouterr().out


def test_without_the_key_no_play_entry_is_called(monkeypatch, capsys):
    p, lib, out = _cpu_player(monkeypatch, capsys, {})
    assert p._fused is None and 'fused play path' not in out
    assert not [n for n in lib.names if n.startswith('rlg_play_')], lib.names


def test_a_declined_network_prints_the_notice_and_calls_no_play_entry(monkeypatch, capsys):
    for network, why in ((dict(fixed_sigma=False), 'a log sigma vector and one value column only'),
                         (dict(rnn={'name': 'lstm', 'units': 16, 'layers': 2}), None)):
        p, lib, out = _cpu_player(monkeypatch, capsys, {'fused': True}, **network)
        assert p._fused is None
        notice = [l for l in out.splitlines() if l.startswith('rl_games_amd: player outside the fused play path (')]
        assert len(notice) == 1 and notice[0].endswith('); using torch modules'), out
        assert why is None or f'({why})' in notice[0], notice
        assert not [n for n in lib.names if n.startswith('rlg_play_')], lib.names


if __name__ == '__main__':
    print(json.dumps(run_table()))
