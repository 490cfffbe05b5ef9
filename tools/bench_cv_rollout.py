"""Rollout time of agents with a central value network, `fused_rollout` on (actor chain forward + critic chain forward
+ one head launch, replayed as step graphs) against off (the torch actor and critic modules, one update_data per
field), in one process.

Every shape builds one agent per setting from the same seed; one train_epoch and one play_steps() each warm up
(allocations, library algorithm choice, the step graphs' capture), then the two settings' play_steps() alternate for
--epochs timed epochs, each between device synchronisations.  Prints one JSON line per shape: the synthetic observation
and state widths, the per-step rollout time (ms, median and spread over the epochs) of both settings and their ratio.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--only-fused keeps that trace to the
fused path).

    python tools/bench_cv_rollout.py [--shapes go1,humanoid,smac] [--epochs 7] [--only-fused]
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
from rl_games_amd.agent import A2CAgent  # noqa: E402
from rl_games_amd.discrete_agent import DiscreteA2CAgent  # noqa: E402

# shape -> (envs, horizon, agents, obs width, state width, hidden units, activation)
SHAPES = {
    # the go1 velocity config's shape: 4,096 x 24, actor and critic [512, 256, 128] elu, 12 actions
    'go1': (4096, 24, 1, 48, 96, [512, 256, 128], 'elu'),
    # BASELINE.json config #3 with a critic: 65,536 x 32, obs 108, 21 actions, both nets [400, 200, 100]
    'humanoid': (65536, 32, 1, 108, 128, [400, 200, 100], 'elu'),
    # SMAC-like: 5 agents per env, Discrete(12) with action masks, both nets [256, 128] relu
    'smac': (8192, 16, 5, 56, 120, [256, 128], 'relu'),
}


def _critic(units, act, minibatch):
    return {'minibatch_size': minibatch, 'mini_epochs': 1, 'learning_rate': 5e-4, 'clip_value': True,
            'normalize_input': True, 'truncate_grads': True, 'grad_norm': 1.0,
            'network': {'name': 'actor_critic', 'central_value': True,
                        'mlp': {'units': list(units), 'activation': act, 'initializer': {'name': 'default'}}}}


def _params(shape, fused):
    envs, horizon, agents, obs, states, units, act = SHAPES[shape]
    batch = envs * horizon
    mb = min(batch // 4, 32768)                 # (the update only warms up here: BASELINE's minibatch size at most)
    if shape == 'smac':
        params = configs.cartpole_discrete(num_actors=envs, horizon_length=horizon, minibatch_size=mb * agents,
                                           mini_epochs=1, normalize_input=True, normalize_value=True,
                                           fused_rollout=fused)
        params['network'].update(separate=True)
        params['network']['mlp'].update(units=units, activation=act)
        params['config']['use_action_masks'] = True
        params['config']['env_config'].update(obs_dim=obs, discrete_actions=12, action_masks=True,
                                              autoreset_mode='same_step')
    else:
        act_dim = 12 if shape == 'go1' else 21
        params = configs.tiny(num_actors=envs, horizon=horizon, obs_dim=obs, act_dim=act_dim, minibatch_size=mb,
                              fused_rollout=fused)
        params['config']['mini_epochs'] = 1
        params['network']['mlp'].update(units=units, activation=act)
    params['config']['env_config'].update(state_dim=states, agents=agents)
    params['config']['central_value_config'] = _critic(units, act, mb)
    return params


def _agent(shape, fused):
    torch.manual_seed(0)
    params = _params(shape, fused)
    cls = DiscreteA2CAgent if params['algo']['name'] == 'a2c_discrete' else A2CAgent
    agent = cls(f'bench_cv_{shape}', params)
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
    ap.add_argument('--shapes', default='go1,humanoid,smac')
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
        envs, horizon, n_agents, obs, states, units, act = SHAPES[shape]
        chain = a._critic_chain().chain
        res = {'shape': shape, 'envs': envs, 'horizon': horizon, 'agents': n_agents, 'obs_dim': obs, 'state_dim': states,
               'units': units, 'activation': act, 'actions': getattr(a, 'branch_sizes', a.actions_num),
               'critic_split_planes': chain.split_products(envs, 0), 'critic_lean': chain.lean_used(envs, 0),
               'graphs': len(a._rollout_graphs), 'epochs': args.epochs}
        for f in settings:
            key = 'fused' if f else 'torch'
            res[f'{key}_ms_per_step'] = round(statistics.median(times[f]), 4)
            res[f'{key}_ms_per_step_min_max'] = [round(min(times[f]), 4), round(max(times[f]), 4)]
        if not args.only_fused:
            res['torch_over_fused'] = round(res['torch_ms_per_step'] / res['fused_ms_per_step'], 3)
        print(json.dumps(res), flush=True)
        del agents, a
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
