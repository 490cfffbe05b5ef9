"""Rollout time of the discrete agent, `fused_rollout` on (chain forward + categorical head launch, replayed as step
graphs) against off (the torch modules, Categorical sampling, one update_data per field), in one process.

Every shape builds one agent per setting from the same seed; one train_epoch and one play_steps() each warm up
(allocations, library algorithm choice, the step graphs' capture), then the two settings' play_steps() alternate for
--epochs timed epochs, each between device synchronisations.  Prints one JSON line per shape: the per-step rollout
time (ms, median and spread over the epochs) of both settings and their ratio.  The head kernel's own time comes from
a separate run under `rocprofv3 --kernel-trace --stats` (--only-fused keeps that trace to the fused path).

    python tools/bench_discrete_rollout.py [--shapes discrete6,multi_masked,cartpole] [--epochs 7] [--only-fused]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rl_games_amd import configs  # noqa: E402
from rl_games_amd.discrete_agent import DiscreteA2CAgent  # noqa: E402


def _params(shape, fused):
    if shape == 'cartpole':                    # BASELINE.json config #1: 16 envs, separate [32, 32] relu trunks
        return configs.cartpole_discrete(num_actors=16, fused_rollout=fused)
    # 65,536 envs x 32 steps, obs 64, shared [256, 128, 64] elu trunk
    params = configs.cartpole_discrete(num_actors=65536, horizon_length=32, minibatch_size=32768, mini_epochs=1,
                                       normalize_input=True, normalize_value=True, fused_rollout=fused)
    params['network'].update(separate=False)
    params['network']['mlp'].update(units=[256, 128, 64], activation='elu')
    env = params['config']['env_config']
    env.update(obs_dim=64, autoreset_mode='same_step')
    if shape == 'discrete6':
        env.update(discrete_actions=6)
    elif shape == 'multi_masked':
        params['network']['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
        params['config']['use_action_masks'] = True
        env.update(discrete_actions=[3, 5, 2], action_masks=True)
    else:
        raise ValueError(shape)
    return params


def _agent(shape, fused):
    torch.manual_seed(0)
    agent = DiscreteA2CAgent(f'bench_{shape}', _params(shape, fused))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert agent._fast_rollout_ok() == fused
    agent.epoch_num += 1
    agent.train_epoch()
    agent.set_eval()
    with torch.no_grad():
        agent.play_steps()
    torch.cuda.synchronize()
    return agent


def _timed_rollout(agent):
    agent.set_eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        agent.play_steps()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / agent.horizon_length * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='discrete6,multi_masked,cartpole')
    ap.add_argument('--epochs', type=int, default=7)
    ap.add_argument('--only-fused', action='store_true')
    args = ap.parse_args()
    if args.epochs < 5:
        raise SystemExit('--epochs: at least 5 timed epochs')
    settings = (True,) if args.only_fused else (True, False)
    for shape in args.shapes.split(','):
        agents = {f: _agent(shape, f) for f in settings}
        times = {f: [] for f in settings}
        for _ in range(args.epochs):
            for f in settings:
                times[f].append(_timed_rollout(agents[f]))
        a = agents[True]
        res = {'shape': shape, 'envs': a.num_actors, 'horizon': a.horizon_length, 'branches': a.branch_sizes,
               'graphs': len(a._rollout_graphs), 'epochs': args.epochs}
        for f in settings:
            key = 'fused' if f else 'torch'
            res[f'{key}_ms_per_step'] = round(statistics.median(times[f]), 4)
            res[f'{key}_ms_per_step_min_max'] = [round(min(times[f]), 4), round(max(times[f]), 4)]
        if not args.only_fused:
            res['torch_over_fused'] = round(res['torch_ms_per_step'] / res['fused_ms_per_step'], 3)
        print(json.dumps(res), flush=True)
        del agents
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
