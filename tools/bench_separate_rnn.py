"""Rollout step and optimiser step of a continuous policy with separate actor / critic trunks, each with its own RNN, on one
MI355X: chain_net.RecurrentChainPair (the default) against the torch-module path it replaces (`manual_lstm: False`:
torch.nn modules with autograd between this library's rollout, loss and optimiser kernels).

    python tools/bench_separate_rnn.py [--envs 24,4096] [--epochs 7]

Shapes: the lunar shape (configs.lunar_separate_rnn: trunks [64], LSTM 64) and trunks [512, 256] + LSTM 128, horizon 16
in sequences of 4, two minibatches x 4 mini-epochs, at 24 and 4,096 envs.  Both agents live in one process and take
turns epoch by epoch: two warm-up epochs each (the second captures the step graphs), then `--epochs` timed ones.  A
host clock around each phase, which ends in a device synchronise: the rollout (play_steps_rnn, synthetic env included)
per step, the update (every train_actor_critic of the epoch) per optimiser step.  Printed: the medians, each version's
spread (max - min over its epochs as a share of the median), and the device kernels of one optimiser step as the
profiler counts them (`launches`; `n/a` where the profiler gives no device events)."""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_games_amd import configs  # noqa: E402
from rl_games_amd.agent import A2CAgent  # noqa: E402

SHAPES = {'lunar [64] + LSTM 64': dict(units=64, mlp=[64]), '[512, 256] + LSTM 128': dict(units=128, mlp=[512, 256])}


def make(shape, envs, engine):
    params = configs.lunar_separate_rnn(num_actors=envs, units=shape['units'], horizon_length=16)
    params['network']['mlp']['units'] = list(shape['mlp'])
    params['config']['env_config'].update(p_done=0.05)
    if not engine:
        params['config']['manual_lstm'] = False
    torch.manual_seed(0)
    agent = A2CAgent('bench', copy.deepcopy(params))
    assert (agent._rnn_pair is not None) == engine and agent._engine is None
    agent.init_tensors()
    agent.obs = agent.env_reset()
    return agent


def epoch(agent):
    """(seconds per rollout step, seconds per optimiser step) of one epoch"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.set_eval()
    with torch.no_grad():
        batch = agent.play_steps_rnn()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    agent.set_train()
    agent.curr_frames = batch.pop('played_frames')
    agent.prepare_dataset(batch)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    steps = 0
    for _ in range(agent.mini_epochs_num):
        for i in range(len(agent.dataset)):
            agent.train_actor_critic(agent.dataset[i])
            steps += 1
        if agent.normalize_input:
            agent.model.running_mean_std.eval()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    agent._eager_epochs += 1                                 # (what train_epoch counts: step graphs from the second epoch on)
    return (t1 - t0) / agent.horizon_length, (t3 - t2) / steps


def launches_per_step(agent):
    try:
        from torch.profiler import ProfilerActivity, profile
        agent.set_train()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            agent.train_actor_critic(agent.dataset[0])
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return str(n) if n else 'n/a'
    except Exception as e:                                   # the count is an extra: never the reason a timing is lost
        return f'n/a ({type(e).__name__})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='24,4096')
    ap.add_argument('--epochs', type=int, default=7)
    args = ap.parse_args()
    print('shape                    envs  version   rollout step us   optimiser step us   spread roll / opt   launches', flush=True)
    for name, shape in SHAPES.items():
        for envs in (int(x) for x in args.envs.split(',')):
            agents = {'pair': make(shape, envs, True), 'torch': make(shape, envs, False)}
            times = {k: [] for k in agents}
            for e in range(2 + args.epochs):
                for k, agent in agents.items():
                    t = epoch(agent)
                    if e >= 2:
                        times[k].append(t)
            for k, agent in agents.items():
                roll, opt = ([t[c] for t in times[k]] for c in (0, 1))
                mr, mo = statistics.median(roll), statistics.median(opt)
                print(f'{name:24s} {envs:5d}  {k:6s}  {mr * 1e6:15.1f}   {mo * 1e6:17.1f}   '
                      f'{100 * (max(roll) - min(roll)) / mr:5.1f} % / {100 * (max(opt) - min(opt)) / mo:5.1f} %   '
                      f'{launches_per_step(agent)}', flush=True)
            del agents


if __name__ == '__main__':
    main()
