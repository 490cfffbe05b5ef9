"""Rollout time of agents with a central value network, `fused_rollout` on (actor chain forward + critic chain forward
+ one head launch, replayed as step graphs) against off (the torch actor and critic modules, one update_data per
field), in one process.

Every shape builds one agent per setting from the same seed; one train_epoch and one play_steps() each warm up
(allocations, library algorithm choice, the step graphs' capture), then the two settings' play_steps() alternate for
--epochs timed epochs, each between device synchronisations.  Prints one JSON line per shape: the synthetic observation
and state widths, the per-step rollout time (ms, median and spread over the epochs) of both settings and their ratio.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--only-fused keeps that trace to the
fused path).

--critic-update (recurrent-critic shapes): times CentralValueTrain.train_net() instead - the critic on its engine
(chain_net.RecurrentChainNet with the value tail of csrc/rnn_value_tail.hip) against `fused_mlp: False` in the critic's
config (torch modules + autograd) - the same way, and counts the device launches of one critic optimiser step of either
setting with torch.profiler.

    python tools/bench_cv_rollout.py [--shapes go1,humanoid,smac,smac_rnn_24,smac_rnn] [--epochs 7] [--only-fused]
                                     [--critic-update]
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
    # configs.smac_rnn_cv_discrete (5m_vs_6m_rnn_cv.yaml): 5 agents, masked Discrete(14), actor and critic [512, 256]
    # relu + LSTM 128, sequences of 8 - at the config's 24 envs and at 4,096
    'smac_rnn_24': (24, 16, 5, 80, 98, [512, 256], 'relu'),
    'smac_rnn': (4096, 16, 5, 80, 98, [512, 256], 'relu'),
}


def _critic(units, act, minibatch):
    return {'minibatch_size': minibatch, 'mini_epochs': 1, 'learning_rate': 5e-4, 'clip_value': True,
            'normalize_input': True, 'truncate_grads': True, 'grad_norm': 1.0,
            'network': {'name': 'actor_critic', 'central_value': True,
                        'mlp': {'units': list(units), 'activation': act, 'initializer': {'name': 'default'}}}}


def _params(shape, fused, critic_engine=True):
    envs, horizon, agents, obs, states, units, act = SHAPES[shape]
    if shape.startswith('smac_rnn'):
        params = configs.smac_rnn_cv_discrete(num_actors=envs, agents=agents, state_dim=states, horizon_length=horizon,
                                              fused_rollout=fused, mini_epochs=1)
        params['network']['mlp'].update(units=units)
        params['config']['central_value_config'].update(mini_epochs=1)
        if not critic_engine:
            params['config']['central_value_config']['fused_mlp'] = False
        return params
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


def _play(agent):
    return agent.play_steps_rnn() if agent.is_rnn else agent.play_steps()


def _agent(shape, fused, critic_engine=True):
    torch.manual_seed(0)
    params = _params(shape, fused, critic_engine)
    cls = DiscreteA2CAgent if params['algo']['name'] == 'a2c_discrete' else A2CAgent
    agent = cls(f'bench_cv_{shape}', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert agent._fast_rollout_ok() == (fused and critic_engine)
    agent.epoch_num += 1
    agent.train_epoch()
    agent.set_eval()
    with torch.no_grad():
        _play(agent)
    torch.cuda.synchronize()
    return agent


def _timed_rollout(agent):
    agent.set_eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        _play(agent)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / agent.horizon_length * 1e3


def _timed_critic_update(agent):
    cv = agent.central_value_net
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cv.train_net()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _launches_per_critic_step(agent):
    """Device launches (kernels and memory operations) of one CentralValueTrain.train_critic call."""
    from torch.profiler import ProfilerActivity, profile
    cv = agent.central_value_net
    cv.train()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        cv.train_critic(cv.dataset[0])
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def _critic_update(shape, epochs):
    agents = {e: _agent(shape, True, critic_engine=e) for e in (True, False)}
    assert agents[True].central_value_net._rnn_engine is not None
    assert agents[False].central_value_net._rnn_engine is None
    for a in agents.values():
        _timed_critic_update(a)
    times = {e: [] for e in agents}
    for _ in range(epochs):
        for e, a in agents.items():
            times[e].append(_timed_critic_update(a))
    cv = agents[True].central_value_net
    steps = cv.mini_epoch * cv.num_minibatches
    envs, horizon, n_agents, obs, states, units, act = SHAPES[shape]
    res = {'shape': shape, 'mode': 'critic-update', 'envs': envs, 'horizon': horizon, 'state_dim': states, 'units': units,
           'critic_minibatch': cv.minibatch_size, 'optimiser_steps_per_train_net': steps, 'epochs': epochs,
           'dw_path': cv._rnn_engine.last_dw_path}
    for e, key in ((True, 'engine'), (False, 'autograd')):
        res[f'{key}_train_net_ms'] = round(statistics.median(times[e]), 4)
        res[f'{key}_train_net_ms_min_max'] = [round(min(times[e]), 4), round(max(times[e]), 4)]
        res[f'{key}_launches_per_step'] = _launches_per_critic_step(agents[e])
    # the tail launch stands for five: padded row-GEMM head, rlg_value_loss, narrow_dx, the bias sum, the 1 x H dW job
    res['engine_launches_per_step_with_five_launch_tail'] = res['engine_launches_per_step'] + 4
    res['autograd_over_engine'] = round(res['autograd_train_net_ms'] / res['engine_train_net_ms'], 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='go1,humanoid,smac')
    ap.add_argument('--epochs', type=int, default=7)
    ap.add_argument('--only-fused', action='store_true')
    ap.add_argument('--critic-update', action='store_true')
    args = ap.parse_args()
    if args.epochs < 5:
        raise SystemExit('--epochs: at least 5 timed epochs')
    if args.critic_update:
        for shape in args.shapes.split(','):
            if not shape.startswith('smac_rnn'):
                raise SystemExit('--critic-update: recurrent-critic shapes (smac_rnn_24, smac_rnn) only')
            _critic_update(shape, args.epochs)
            torch.cuda.empty_cache()
        return
    settings = (True,) if args.only_fused else (True, False)
    for shape in args.shapes.split(','):
        agents = {f: _agent(shape, f) for f in settings}
        times = {f: [] for f in settings}
        for _ in range(args.epochs):
            for f in settings:
                times[f].append(_timed_rollout(agents[f]))
        a = agents[True]
        envs, horizon, n_agents, obs, states, units, act = SHAPES[shape]
        chain = a.central_value_net.engines()[0].chain
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
