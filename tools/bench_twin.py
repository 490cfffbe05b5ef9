"""Continuous policies with separate actor / critic MLPs (configs.mujoco_separate_mlp): the twin-trunk chain path
(actor_paths.TwinPath, csrc/mlp_chain_twin.hip) against `fused_mlp: False`, in one process.  `fused_mlp: False` is the
route every such policy took before the twin path existed: actor_paths.AutogradPath in the update (torch.nn.Linear
forwards, library GEMMs, autograd) and the torch rollout.

Per --envs value one agent per setting from the same seed; one train_epoch and one play_steps() each warm up
(allocations, library algorithm choice, the step graphs' capture), then the two settings alternate for --repeats timed
windows, each between device synchronisations: one rollout (ms per step) and --steps optimiser steps
(train_actor_critic on successive minibatches, ms per step).  Prints one JSON line per size: both settings' medians and
spreads, their ratios, the device launches of one optimiser step (torch.profiler), the 16-row groups the chain launches
run with.

    python tools/bench_twin.py [--envs 4096,65536] [--units 256,128,64] [--repeats 7] [--steps 4]
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


def _agent(envs, units, fused):
    torch.manual_seed(0)
    horizon = 16 if envs <= 8192 else 8                  # (65,536 envs: 524,288 rows, 16 minibatches of 32,768)
    params = configs.mujoco_separate_mlp(num_actors=envs, units=units, horizon_length=horizon, mini_epochs=1, fused_mlp=fused)
    agent = A2CAgent(f'bench_twin_{envs}', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert agent._path.kind == ('twin' if fused else 'autograd') and agent._fast_rollout_ok() == fused
    agent.epoch_num += 1
    agent.train_epoch()
    _rollout(agent)
    return agent


def _rollout(agent):
    agent.set_eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        batch = agent.play_steps()
    torch.cuda.synchronize()
    agent._bench_batch = batch
    return (time.perf_counter() - t0) / agent.horizon_length * 1e3


def _update(agent, steps):
    agent.set_train()
    agent.prepare_dataset(agent._bench_batch)
    n = len(agent.dataset)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        agent.train_actor_critic(agent.dataset[i % n])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _launches(fn):
    """Device launches (kernels and memory operations) of fn()."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--units', default='256,128,64')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=4)
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit('--repeats: at least 5 timed windows')
    units = [int(u) for u in args.units.split(',')]
    for envs in (int(e) for e in args.envs.split(',')):
        agents = {f: _agent(envs, units, f) for f in (True, False)}
        times = {(f, k): [] for f in agents for k in ('rollout', 'update')}
        for _ in range(args.repeats):
            for f, a in agents.items():
                times[f, 'rollout'].append(_rollout(a))
                times[f, 'update'].append(_update(a, args.steps))
        twin = agents[True]
        chain, mb = twin._path.twin.chain, twin.minibatch_size
        res = {'envs': envs, 'horizon': twin.horizon_length, 'minibatch': mb, 'units': units, 'obs_dim': 17, 'actions': 6,
               'groups_fwd_train': chain.groups(mb, 2), 'groups_bwd': chain.groups(mb, 1), 'groups_rollout': chain.groups(envs, 0),
               'rollout_graphs': len(twin._rollout_graphs), 'dw_path': twin._path.twin.last_dw_path,
               'dw_library_products': twin._path.twin.weight_grads.last_dw_library_jobs, 'repeats': args.repeats}
        for f, key in ((True, 'twin'), (False, 'autograd')):
            a = agents[f]
            for k, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
                t = times[f, k]
                res[f'{key}_{k}_{unit}'] = round(statistics.median(t), 4)
                res[f'{key}_{k}_min_max'] = [round(min(t), 4), round(max(t), 4)]
            a.set_train()
            res[f'{key}_launches_per_optimiser_step'] = _launches(lambda: a.train_actor_critic(a.dataset[0]))
        for k, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
            res[f'autograd_over_twin_{k}'] = round(res[f'autograd_{k}_{unit}'] / res[f'twin_{k}_{unit}'], 3)
        print(json.dumps(res), flush=True)
        del agents, twin, chain
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
