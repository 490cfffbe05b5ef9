"""Discrete policies over dense-to-dense trunks (configs.discrete_d2rl at Ant's shape: obs 60, [256, 128, 64], 8 actions):
the D2RL chain kernels (`d2rl_kernels: True`: actor_paths.ChainsPath over ops.MlpChainD2rl, csrc/mlp_chain_d2rl.hip) against
the key off (actor_paths.AutogradPath: torch modules, one library GEMM and one torch.cat per layer under autograd, the torch
rollout), in one process and one build.

Per --envs value one agent per setting from the same seed; one train_epoch and one play_steps() each warm up, then the
two settings alternate for --repeats timed windows, each between device synchronisations: one rollout (ms per step) and
--steps optimiser steps (ms per step).  Prints one JSON line per size: both settings' medians and spreads, their ratios,
the device launches of one optimiser step (torch.profiler).

    python tools/bench_d2rl.py [--envs 4096,65536] [--units 256,128,64] [--repeats 7] [--steps 4] [--separate]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_twin import _launches, _rollout, _update  # noqa: E402
from rl_games_amd import configs  # noqa: E402
from rl_games_amd.discrete_agent import DiscreteA2CAgent  # noqa: E402


def _agent(envs, units, separate, key):
    torch.manual_seed(0)
    horizon = 16 if envs <= 8192 else 8                  # (65,536 envs: 524,288 rows, 16 minibatches of 32,768)
    params = configs.discrete_d2rl(num_actors=envs, units=units, obs_dim=60, actions=8, separate=separate, d2rl_kernels=key,
                                   horizon_length=horizon, minibatch_size=min(32768, envs * horizon), mini_epochs=1)
    agent = DiscreteA2CAgent(f'bench_d2rl_{envs}', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert agent._path.kind == ('chains' if key else 'autograd') and agent._fast_rollout_ok() == key
    agent.epoch_num += 1
    agent.train_epoch()
    _rollout(agent)
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--units', default='256,128,64')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--separate', action='store_true')
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit('--repeats: at least 5 timed windows')
    units = [int(u) for u in args.units.split(',')]
    for envs in (int(e) for e in args.envs.split(',')):
        agents = {k: _agent(envs, units, args.separate, k) for k in (True, False)}
        times = {(k, w): [] for k in agents for w in ('rollout', 'update')}
        for _ in range(args.repeats):
            for k, a in agents.items():
                times[k, 'rollout'].append(_rollout(a))
                times[k, 'update'].append(_update(a, args.steps))
        on = agents[True]
        res = {'envs': envs, 'horizon': on.horizon_length, 'minibatch': on.minibatch_size, 'units': units, 'obs_dim': 60,
               'actions': 8, 'separate': args.separate, 'dw_path': on._chains[0].last_dw_path,
               'groups_fwd_bwd': [on._chains[0].chain.groups(on.minibatch_size, d) for d in (2, 1)], 'repeats': args.repeats}
        for k, key in ((True, 'kernels'), (False, 'autograd')):
            a = agents[k]
            for w, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
                t = times[k, w]
                res[f'{key}_{w}_{unit}'] = round(statistics.median(t), 4)
                res[f'{key}_{w}_min_max'] = [round(min(t), 4), round(max(t), 4)]
            a.set_train()
            res[f'{key}_launches_per_optimiser_step'] = _launches(lambda: a.train_actor_critic(a.dataset[0]))
        for w, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
            res[f'autograd_over_kernels_{w}'] = round(res[f'autograd_{w}_{unit}'] / res[f'kernels_{w}_{unit}'], 3)
        print(json.dumps(res), flush=True)
        del agents, on
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
