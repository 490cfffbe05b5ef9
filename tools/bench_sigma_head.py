"""Continuous policies with a sigma head (configs.pendulum_sigma_head at Ant's shape: obs 60, A = 8): the sigma-head
kernels (`sigma_head_kernels: True`: actor_paths.SigmaPath, csrc/ppo_loss_sigma.hip) against the key off
(actor_paths.GeneralPath: torch modules, torch_fallback.ppo_loss under autograd, the torch rollout), in one process.

Per --envs value one agent per setting from the same seed; one train_epoch and one play_steps() each warm up, then the
two settings alternate for --repeats timed windows, each between device synchronisations: one rollout (ms per step) and
--steps optimiser steps (ms per step).  Prints one JSON line per size: both settings' medians and spreads, their ratios,
the device launches of one optimiser step (torch.profiler).  --errors: instead, per sigma form, the largest error of the
loss kernel's gradients and of the fp32 torch-op path (torch_fallback.ppo_loss on the GPU) against fp64 on the CPU, each
relative to the tensor's largest magnitude, and their ratio; and the errors of both paths' five scalars, KL and loss next
to the tests' bound for them.

    python tools/bench_sigma_head.py [--envs 4096,65536] [--units 256,128,64] [--repeats 7] [--steps 4] [--errors]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_twin import _launches, _rollout, _update  # noqa: E402
from rl_games_amd import configs, ops  # noqa: E402
from rl_games_amd import torch_fallback as tf  # noqa: E402
from rl_games_amd.agent import A2CAgent  # noqa: E402

FORMS = {'exp': {}, 'exp_bounds': {'logstd_bounds': (-1.0, 0.5)}, 'exp_floor': {'min_sigma': 0.05},
         'softplus_floor': {'sigma_parametrization': 'softplus', 'min_sigma': 0.05},
         'linear_floor': {'sigma_parametrization': 'linear', 'min_sigma': 0.2}}


def _agent(envs, units, key):
    torch.manual_seed(0)
    horizon = 16 if envs <= 8192 else 8                  # (65,536 envs: 524,288 rows, 16 minibatches of 32,768)
    params = configs.pendulum_sigma_head(num_actors=envs, units=units, obs_dim=60, act_dim=8, horizon_length=horizon,
                                         mini_epochs=1, sigma_head_kernels=key)
    agent = A2CAgent(f'bench_sigma_{envs}', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    assert agent._path.kind == ('sigma' if key else 'general') and agent._fast_rollout_ok() == key
    agent.epoch_num += 1
    agent.train_epoch()
    _rollout(agent)
    return agent


def _sigma_fn(form):
    """ActorCriticNetwork.sigma_and_logstd for the form fields, in the dtype of its argument."""
    def fn(raw):
        if form['sigma_kind'] == 1:
            sigma = F.softplus(raw) + form['min_sigma']
        elif form['sigma_kind'] == 2:
            floor = max(form['min_sigma'], 1e-3)
            sigma = floor + F.softplus(raw - floor)
        else:
            if form['has_bounds']:
                raw = raw.clamp(form['sigma_lo'], form['sigma_hi'])
            sigma = raw.exp()
            if form['min_sigma'] <= 0:
                return sigma, raw
            sigma = sigma + form['min_sigma']
        return sigma, sigma.log()
    return fn


def errors(rows=4096, A=8):
    kw = dict(e_clip=0.2, critic_coef=2.0, entropy_coef=0.01, bounds_coef=0.05, bound_kind=1, clip_value=True, smooth=0)
    for name, net in FORMS.items():
        form, gen = ops.sigma_form(net), torch.Generator().manual_seed(1)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        mu, raw, v, adv, ret = rnd(rows, A), rnd(rows, A) * 0.8 - 0.3, rnd(rows), rnd(rows), rnd(rows)
        sigma, logstd = _sigma_fn(form)(raw.double())
        x = (mu.double() + sigma * rnd(rows, A).double()).float()
        nlp = 0.5 * (((x.double() - mu.double()) / sigma) ** 2).sum(-1) + 0.9189385332046727 * A + logstd.sum(-1)
        step = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (rows,), generator=gen)]
        onlp, vo = (nlp + step([-0.5, -0.1, 0.05, 0.3]).double()).float(), v + step([-0.5, -0.1, 0.1, 0.4])

        def torch_path(dtype, dev):
            t = [z.to(dev, dtype).requires_grad_() for z in (mu, raw, v)]
            c = [z.to(dev, dtype) for z in (x, onlp, adv, vo, ret)]
            loss, sc, sg = tf.ppo_loss(t[0], t[1], t[2].view(-1, 1), c[0], c[1], c[2], c[3].view(-1, 1), c[4].view(-1, 1),
                                       sigma_fn=_sigma_fn(form), **kw)
            loss.backward()
            kl = tf.policy_kl(t[0].detach(), sg.detach(), torch.zeros_like(t[0]), torch.ones_like(t[0]))
            scalars = [sc[k] for k in ('a_loss', 'c_loss', 'entropy', 'b_loss')] + [kl, loss.detach()]
            return [z.grad.double().cpu() for z in t] + [torch.stack([z.double().cpu() for z in scalars])]
        ref, op32 = torch_path(torch.float64, 'cpu'), torch_path(torch.float32, 'cuda')
        g = [z.cuda() for z in (mu, raw, v, x, onlp, adv, vo, ret)]
        d = [torch.empty_like(g[0]), torch.empty_like(g[1]), torch.empty_like(g[2])]
        partials = torch.empty(ops.ppo_loss_sigma_blocks(rows), 7, dtype=torch.float64, device='cuda')
        ops.ppo_loss_sigma(g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], torch.zeros_like(g[0]), torch.ones_like(g[0]),
                           d[0], d[1], d[2], partials, form, 0.2, 2.0, 0.01, 0.05, True, 0, 1, False)
        s8 = torch.empty(8, device='cuda')
        ops.ppo_loss_finalize(partials, partials.shape[0], 0, rows, False, 2.0, 0.01, 0.05, s8, torch.zeros(1, device='cuda'))
        res = {'form': name, 'rows': rows, 'actions': A}
        for k, r, o, h in zip(('d_mu', 'd_raw_sigma', 'd_values'), ref, op32, d):
            scale = r.abs().max().item()
            e_k, e_o = (h.double().cpu() - r).abs().max().item() / scale, (o - r).abs().max().item() / scale
            res[k] = {'kernel': float(f'{e_k:.3g}'), 'torch_fp32': float(f'{e_o:.3g}'), 'ratio': round(e_k / e_o, 2)}
        # the scalars: |error|, and the tests' bound rtol 1e-5 |fp64| + 2e-7 next to it
        for j, k in enumerate(('a_loss', 'c_loss', 'entropy', 'b_loss', 'kl', 'loss')):
            r = ref[3][j].item()
            res[k] = {'fp64': float(f'{r:.6g}'), 'kernel': float(f'{abs(s8[j].item() - r):.3g}'),
                      'torch_fp32': float(f'{abs(op32[3][j].item() - r):.3g}'), 'bound': float(f'{1e-5 * abs(r) + 2e-7:.3g}')}
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--units', default='256,128,64')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--errors', action='store_true')
    args = ap.parse_args()
    if args.errors:
        return errors()
    if args.repeats < 5:
        raise SystemExit('--repeats: at least 5 timed windows')
    units = [int(u) for u in args.units.split(',')]
    for envs in (int(e) for e in args.envs.split(',')):
        agents = {k: _agent(envs, units, k) for k in (True, False)}
        times = {(k, w): [] for k in agents for w in ('rollout', 'update')}
        for _ in range(args.repeats):
            for k, a in agents.items():
                times[k, 'rollout'].append(_rollout(a))
                times[k, 'update'].append(_update(a, args.steps))
        on = agents[True]
        res = {'envs': envs, 'horizon': on.horizon_length, 'minibatch': on.minibatch_size, 'units': units, 'obs_dim': 60,
               'actions': 8, 'rollout_graphs': len(on._rollout_graphs), 'dw_path': on._path.chain.last_dw_path,
               'repeats': args.repeats}
        for k, key in ((True, 'sigma'), (False, 'general')):
            a = agents[k]
            for w, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
                t = times[k, w]
                res[f'{key}_{w}_{unit}'] = round(statistics.median(t), 4)
                res[f'{key}_{w}_min_max'] = [round(min(t), 4), round(max(t), 4)]
            a.set_train()
            res[f'{key}_launches_per_optimiser_step'] = _launches(lambda: a.train_actor_critic(a.dataset[0]))
        for w, unit in (('rollout', 'ms_per_step'), ('update', 'ms_per_optimiser_step')):
            res[f'general_over_sigma_{w}'] = round(res[f'general_{w}_{unit}'] / res[f'sigma_{w}_{unit}'], 3)
        print(json.dumps(res), flush=True)
        del agents, on
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
