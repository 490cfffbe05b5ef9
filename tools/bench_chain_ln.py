"""Time of a `normalization: layer_norm` discrete agent on the fused chain kernels of csrc/mlp_chain_ln.hip against the
same agent on torch modules + autograd (`fused_mlp: False`: the path such networks took before), in one process.

Network: the SMAC shape - obs 98, shared trunk [512, 256] relu with a layer norm behind every layer, 15 actions.
  chain  : the network alone at 2,560 and 20,480 rows - one training forward + backward + weight gradients of the
           agent's chain_net.ChainNet (3 launches + the first layer's library GEMM) against normaliser + modules +
           torch.autograd.grad over the same parameters, from the same d heads
  update : one whole train_actor_critic() of such a minibatch (chain forward + loss + chain backward + weight
           gradients + Adam on one side; module forward + loss + autograd + Adam on the other)
  rollout: one play_steps() of 40 envs, per step (fused rollout step graphs against the torch rollout)
Both settings are built from the same seed and warmed up (allocations, library algorithm choice, graph capture); then
they alternate for --rounds timed rounds of --calls calls each, every round between device synchronisations.  Prints
one JSON line per measurement: median and spread (min .. max) over the rounds per setting, in ms per call, and the
ratio of the medians.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--only-fused).

    python tools/bench_chain_ln.py [--what chain2560,chain20480,update2560,update20480,rollout40] [--rounds 7] [--calls 100] [--only-fused]
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


def _agent(num_actors, horizon, minibatch, fused):
    params = configs.cartpole_discrete(num_actors=num_actors, horizon_length=horizon, minibatch_size=minibatch,
                                       mini_epochs=1, normalize_input=True, normalize_value=True, fused_mlp=fused)
    params['network'].update(separate=False, normalization='layer_norm')
    params['network']['mlp'].update(units=[512, 256], activation='relu')
    params['config']['env_config'].update(obs_dim=98, discrete_actions=15, autoreset_mode='same_step')
    torch.manual_seed(0)
    agent = DiscreteA2CAgent('bench_chain_ln', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert (agent._path.kind == 'chains') == fused
    agent.epoch_num += 1
    agent.train_epoch()
    torch.cuda.synchronize()
    return agent


def _minibatch(agent):
    agent.set_eval()
    with torch.no_grad():
        batch = agent.play_steps()
    agent.set_train()
    agent.prepare_dataset(batch)
    return agent.dataset[0]


def _chain_only(agent, obs, fused):
    """The network's forward + backward + weight gradients over `obs`, from fixed d heads [value | logits]."""
    net = agent.model.a2c_network
    torch.manual_seed(1)
    d_heads = torch.randn(obs.shape[0], 1 + net.logits.out_features, device=obs.device)
    if fused:
        chain = agent._chains[0]
        chain.d_heads[:obs.shape[0]].copy_(d_heads)
        rms, eps = agent._obs_rms(), agent._obs_eps()

        def run():
            chain.forward(obs, rms, eps)
            chain.backward()
        return run
    agent.model.eval()                         # (the normaliser's state as it is, as in the chain launch)
    params = list(net.parameters())

    def run():
        feat = net.actor_mlp(agent.model.norm_obs(obs))
        torch.autograd.grad(torch.cat([net.value(feat), net.logits(feat)], 1), params, d_heads)
    return run


def _timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def _measure(name, fns, rounds, calls, scale=1.0):
    for fn in fns.values():                    # warm-up of exactly the timed call
        _timed(fn, 3)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():              # the settings alternate
            times[k].append(_timed(fn, calls) / scale)
    out = {'what': name, 'unit': 'ms per call', 'rounds': rounds, 'calls': calls}
    for k, ts in times.items():
        out[k] = {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
    if len(times) == 2:
        out['torch_over_fused'] = round(out['torch']['median'] / out['fused']['median'], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='chain2560,chain20480,update2560,update20480,rollout40')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--only-fused', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_chain_ln.py measures on the GPU; none found')
    settings = {'fused': True} if args.only_fused else {'fused': True, 'torch': False}
    for what in args.what.split(','):
        if what.startswith('chain'):
            mb = int(what[len('chain'):])
            agents = {k: _agent(mb // 8, 8, mb, f) for k, f in settings.items()}
            _measure(what, {k: _chain_only(ag, _minibatch(ag)['obs'], settings[k]) for k, ag in agents.items()},
                     args.rounds, args.calls)
        elif what.startswith('update'):
            mb = int(what[len('update'):])
            agents = {k: _agent(mb // 8, 8, mb, f) for k, f in settings.items()}
            fns = {}
            for k, ag in agents.items():
                _minibatch(ag)
                fns[k] = (lambda a: lambda: a.train_actor_critic(a.dataset[0]))(ag)
            _measure(what, fns, args.rounds, args.calls)
        elif what.startswith('rollout'):
            envs, horizon = int(what[len('rollout'):]), 16
            agents = {k: _agent(envs, horizon, envs * horizon, f) for k, f in settings.items()}
            if 'fused' in agents:
                assert agents['fused']._fast_rollout_ok()

            def play(a):
                def run():
                    a.set_eval()
                    with torch.no_grad():
                        a.play_steps()
                return run
            _measure(what + ' (per step)', {k: play(a) for k, a in agents.items()}, args.rounds, max(args.calls // 4, 1),
                     scale=horizon)
        else:
            raise SystemExit(f'unknown measurement {what}')


if __name__ == '__main__':
    main()
