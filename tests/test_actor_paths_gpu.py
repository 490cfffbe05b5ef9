"""GPU: the ordered list of library entries an agent calls over two epochs - the first eager, the second the one that
captures its graphs - for every way of running the actor (rl_games_amd/actor_paths.py: engine, pair, chains, recurrent,
autograd, general), with and without a central value critic, against the lists in tests/golden/actor_path_traces.json.

The lists are names only: every entry the agent called, in order, as indices into a table of names and with repeats
folded (_fold); the comparison leaves out the host-side size queries (_launches).  They were recorded by this file's `--record` entry on the commit BEFORE the actor paths became
objects, so they pin what that refactor had to keep: no launch added, dropped or reordered on any path, eager or captured.
The recording is the parent's, byte for byte, with ONE difference made on reading it (RETIRED): the three one-shot setters
that announced gradient maxima and timing events to the NEXT launch are gone - those arguments travel in the launches' own
descriptors - so their names are taken out of the recorded lists, and nothing else is.  And ONE renaming (RENAMED): a
paired sequence launch is a call of the single entry's name with two problems, so rlg_lstm_seq_forward_pair /
rlg_lstm_seq_backward_pair are read as rlg_lstm_seq_forward / rlg_lstm_seq_backward; a paired launch stays ONE call
where two single launches are two, so the order check keeps its force.  And in the file's table of names, the two
rollout heads that took a central value network's column under a name of their own stand under rlg_rollout_policy_head /
rlg_rollout_categorical_head (the table holds each of these two names twice): the value column is a field of the one
entry's descriptor, and the lists of indices are as recorded.
A change that moves a launch on purpose records them again:

    python tests/test_actor_paths_gpu.py --record tests/golden/actor_path_traces.json [--digests digests.txt]

(--digests: SHA-256 of every optimiser arena and normaliser behind the two epochs, to compare two trees on one machine.)
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TRACES = os.path.join(ROOT, 'tests', 'golden', 'actor_path_traces.json')
N, HZ, T, MB = 64, 8, 4, 256          # 64 envs x horizon 8 in sequences of 4: two minibatches of 256 rows
RNN16 = {'name': 'lstm', 'units': 16, 'layers': 1}
# entries of the recording that the library no longer has
RETIRED = {'rlg_mlp_chain_gradient_maxima', 'rlg_mlp_dw_gradient_maxima', 'rlg_mlp_chain_time_next'}
# entries of the recording that the library has under another name
RENAMED = {'rlg_lstm_seq_forward_pair': 'rlg_lstm_seq_forward', 'rlg_lstm_seq_backward_pair': 'rlg_lstm_seq_backward'}


class _Recorder:
    """Stands in for the loaded library (rl_games_amd._lib._lib): every entry that is called goes through, its name
    into `names` first."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('rlg_'):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


class _HalfObsEnv:
    """The synthetic env with fp16 observations (and an fp16 observation space, so the buffer keeps them as they come):
    not fp32 after preprocessing - the rollout step and the update leave the chains for the torch modules at call time."""

    def __init__(self, inner):
        self.inner = inner

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def get_env_info(self):
        from rl_games_amd.spaces import Box
        info = self.inner.get_env_info()
        info['observation_space'] = Box(-np.inf, np.inf, (self.inner.obs_dim,), np.float16)
        return info

    def reset(self):
        return self.inner.reset().half()

    def step(self, actions):
        obs, rewards, dones, infos = self.inner.step(actions)
        return obs.half(), rewards, dones, infos


def _continuous(num_actors=N, horizon=HZ, minibatch=MB, rnn=None, separate=False, env=None, **over):
    from rl_games_amd import configs
    params = configs.tiny(num_actors=num_actors, horizon=horizon, obs_dim=12, act_dim=4, minibatch_size=minibatch,
                          seq_length=T, **over)
    if rnn is not None:
        params['network']['rnn'] = dict(rnn)
    params['network']['separate'] = separate
    params['config']['env_config'].update(env or {})
    return params


def _discrete(separate=False, actions=4, masks=False, rnn=None, obs_dim=12, agents=1, env=None, **over):
    from rl_games_amd import configs
    params = configs.cartpole_discrete(num_actors=N, normalize_input=True, normalize_value=True, horizon_length=HZ,
                                       minibatch_size=MB * agents, seq_length=T, **over)
    net = params['network']
    net['separate'] = separate
    net['mlp']['units'] = [32, 16]
    params['config']['env_config'].update(obs_dim=obs_dim, discrete_actions=actions, autoreset_mode='same_step',
                                          agents=agents)
    if isinstance(actions, list):
        net['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
    if masks:
        params['config']['use_action_masks'] = True
        params['config']['env_config'].update(action_masks=True)
    if rnn is not None:
        net['rnn'] = dict(rnn)
    params['config']['env_config'].update(env or {})
    return params


def _with_critic(params, agents=1, rnn=None):
    """A central value critic over 13 privileged state features: a [32, 16] trunk, optionally an RNN behind it."""
    net = {'name': 'actor_critic', 'central_value': True,
           'mlp': {'units': [32, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}
    if rnn is not None:
        net['rnn'] = dict(rnn)
    cfg = params['config']
    cfg['env_config'].update(state_dim=13, agents=agents)
    cfg['minibatch_size'] = MB * agents
    cfg['central_value_config'] = {'minibatch_size': MB, 'mini_epochs': 2, 'learning_rate': 5e-4, 'clip_value': True,
                                   'normalize_input': True, 'truncate_grads': True, 'grad_norm': 1.0, 'network': net}
    return params


def _sigma_head():
    params = _continuous()
    params['network']['space']['continuous']['fixed_sigma'] = False
    return params


def _half_observations():
    from rl_games_amd.synthetic_env import SyntheticTensorEnv
    params = _discrete()
    env = SyntheticTensorEnv(N, device=DEV, **params['config']['env_config'])
    params['config']['vec_env'] = _HalfObsEnv(env)
    return params


CASES = {
    'continuous_mlp': _continuous,
    'continuous_mlp_split_kernels': lambda: _continuous(num_actors=512, horizon=16, minibatch=8192),
    'continuous_fused_mlp_off': lambda: _continuous(fused_mlp=False),
    'continuous_manual_mlp_off': lambda: _continuous(manual_mlp=False),
    'continuous_lstm': lambda: _continuous(rnn=RNN16),
    'continuous_gru': lambda: _continuous(rnn=dict(RNN16, name='gru')),
    'continuous_manual_lstm_off': lambda: _continuous(rnn=RNN16, manual_lstm=False),
    'continuous_separate_lstm_pair': lambda: _continuous(rnn=RNN16, separate=True),
    'general_value_size_2': lambda: _continuous(env={'value_size': 2}),
    'general_sigma_head': _sigma_head,
    'discrete_shared': _discrete,
    'discrete_separate': lambda: _discrete(separate=True),
    'discrete_multi_masked': lambda: _discrete(actions=[3, 4], masks=True),
    # (obs 3: the narrow left-over product of the recurrent engine's trunk; next_step autoreset: filler rows, rnn_masks)
    'discrete_lstm': lambda: _discrete(rnn=RNN16, obs_dim=3, env={'autoreset_mode': 'next_step', 'p_done': 0.2}),
    'discrete_fused_mlp_off': lambda: _discrete(fused_mlp=False),
    'mlp_actor_chain_critic': lambda: _with_critic(_continuous()),
    'lstm_actor_lstm_critic': lambda: _with_critic(_continuous(rnn=RNN16), rnn=RNN16),
    'discrete_lstm_actor_lstm_critic': lambda: _with_critic(_discrete(rnn=RNN16), rnn=RNN16),
    'two_agents_chain_critic': lambda: _with_critic(_discrete(agents=2), agents=2),
    'discrete_fp16_observations': _half_observations,
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def _run(case, recorder):
    """The case's agent from seed 4, two train_epoch() calls; returns (names, digests)."""
    from rl_games_amd.agent import A2CAgent
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    params = CASES[case]()
    torch.manual_seed(4)
    cls = DiscreteA2CAgent if params['algo']['name'] == 'a2c_discrete' else A2CAgent
    del recorder.names[:]
    agent = cls(case, params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    for _ in range(2):
        agent.update_epoch()
        agent.train_epoch()
    torch.cuda.synchronize()
    names = list(recorder.names)
    digests = {'flat_params': _sha(agent.optimizer.flat_params)}
    if agent.central_value_net is not None:
        digests['critic_flat_params'] = _sha(agent.central_value_net.optimizer.flat_params)
    for k, mod in enumerate(agent._stats_sync_modules()):
        digests[f'normaliser{k}'] = _sha(torch.cat([v.double().reshape(-1) for v in mod.state_dict().values()]))
    return names, digests


def _install(setattr_):
    from rl_games_amd import _lib
    recorder = _Recorder(_lib.load())
    setattr_(_lib, '_lib', recorder)
    return recorder


def _launches(names):
    """The recorded names without the host-side size queries (rlg_*_num_blocks, *_supported, *_bytes, ...): an entry
    whose prototype takes no pointer at all has no stream to launch on and no memory to touch.  Where such a question
    is asked is the host code's own business - the parent asked for the loss's block count in front of the loss launch
    on two paths and behind it on a third - and everything else is compared in order."""
    import ctypes
    from rl_games_amd import _lib
    scalars = (ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double)
    return [n for n in names if not all(t in scalars for t in _lib._PROTOTYPES[n])]


def _fold(seq, max_period=200):
    """A list with its repeats folded, so that the fixture stays small enough to read: [count, [block]] stands for the
    block `count` times over (the steps of a rollout, the minibatches of a mini-epoch); blocks are folded in turn."""
    out, i = [], 0
    while i < len(seq):
        best = (0, 1)
        for p in range(1, min(max_period, (len(seq) - i) // 2) + 1):
            r = 1
            while seq[i + r * p:i + (r + 1) * p] == seq[i:i + p]:
                r += 1
            if r >= 2 and p * r > best[0] * best[1]:
                best = (p, r)
        p, r = best
        out.append([r, _fold(seq[i:i + p], max_period)] if p else seq[i])
        i += p * r if p else 1
    return out


def _unfold(items):
    out = []
    for it in items:
        out += _unfold(it[1]) * it[0] if isinstance(it, list) else [it]
    return out


def _write_traces(path, traces):
    """{"names": [...], "traces": {case: folded list of indices into names}}, a line per case."""
    import textwrap
    names = sorted({n for t in traces.values() for n in t})
    index = {n: i for i, n in enumerate(names)}
    rows = [f'"{case}": ' + json.dumps(_fold([index[n] for n in t]), separators=(',', ':')) for case, t in sorted(traces.items())]
    table = textwrap.fill(json.dumps(names), 120, break_long_words=False, break_on_hyphens=False)
    with open(path, 'w') as f:
        f.write('{"names": ' + table + ',\n"traces": {\n' + ',\n'.join(rows) + '\n}}\n')


@pytest.fixture(scope='module')
def traces():
    with open(TRACES) as f:
        data = json.load(f)
    return {case: [RENAMED.get(n, n) for n in (data['names'][i] for i in _unfold(t)) if n not in RETIRED]
            for case, t in data['traces'].items()}


def test_every_case_has_a_recorded_trace(traces):
    assert sorted(traces) == sorted(CASES)


@pytest.mark.parametrize('case', sorted(CASES))
def test_two_epochs_call_the_recorded_entries_in_the_recorded_order(case, traces, monkeypatch):
    recorder = _install(monkeypatch.setattr)
    names, _ = _run(case, recorder)
    names, want = _launches(names), _launches(traces[case])
    assert len(want) > 0
    first = next((i for i, (a, b) in enumerate(zip(names, want)) if a != b), min(len(names), len(want)))
    assert names == want, (f'{case}: {len(names)} calls, {len(want)} recorded; first difference at {first}: '
                           f'{names[first - 3:first + 3]} != {want[first - 3:first + 3]}')


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', required=True, help='write the traces of every case to this JSON file')
    ap.add_argument('--digests', help='write SHA-256 digests of arenas and normalisers to this text file')
    args = ap.parse_args()
    rec = _install(setattr)
    out, lines = {}, []
    for name in sorted(CASES):
        try:
            out[name], dig = _run(name, rec)
        except (TypeError, ValueError, KeyError, AttributeError, NotImplementedError) as e:     # (a device error ends the run)
            import traceback
            traceback.print_exc()
            sys.exit(f'{name}: {e!r}')
        lines += [f'{name:34s} {k:20s} {v}' for k, v in dig.items()]
        print(name, len(out[name]), 'calls', flush=True)
    _write_traces(args.record, out)
    if args.digests:
        with open(args.digests, 'w') as f:
            f.write('\n'.join(lines) + '\n')
