"""GPU: the sigma-head kernels of csrc/ppo_loss_sigma.hip - rlg_ppo_loss_sigma (+ rlg_ppo_loss_finalize, actions_num 0) and
rlg_rollout_policy_head_sigma - against fp64 on the CPU: the formulas of torch_fallback.ppo_loss / policy_kl with
ActorCriticNetwork.sigma_and_logstd, gradients by fp64 autograd.

Bound of every compared tensor: the largest difference is at most 1e-5 of the reference's largest magnitude - the figure
tests/test_chain_ln_agent_gpu.py holds fp32 paths to; of the five scalars, the loss and the KL: rtol 1e-5 of the scalar
itself plus a floor of 2e-7, the criterion of tests/test_loss_tile_gpu.py (_check_scalars) for the fixed-sigma kernel.
It follows from the formats: the kernel does the fp32 ops of the torch-op path, one rounding (6e-8) each; the longest
chain ends in exp(old_neglogp - neglogp), which multiplies the neglogp's error by |neglogp| <= 40 here: 2.4e-6 (the fp32
torch-op path's own error and the kernel's ratio to it: profiles/sigma_head.txt).  The inputs keep every branch decision
away from its threshold or exactly on it, so that fp32 and fp64 decide alike."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_CLIP, COEF_C, COEF_E, COEF_B = 0.2, 2.0, 0.01, 0.05
FORMS = {'exp': dict(sigma_parametrization='exp'), 'exp_bounds': dict(sigma_parametrization='exp', logstd_bounds=(-1.0, 0.5)),
         'exp_floor': dict(sigma_parametrization='exp', min_sigma=0.05),
         'softplus_floor': dict(sigma_parametrization='softplus', min_sigma=0.05),
         'linear_floor': dict(sigma_parametrization='scalar', min_sigma=0.2)}
OPTIONS = [(0, True, 1, False), (1, False, 2, True), (2, True, 0, False), (0, False, 0, True), (1, True, 1, False),
           (2, False, 2, True)]


def sigma64(raw, form):
    """sigma_and_logstd (policy.py) in the dtype of `raw`, from the form fields the kernels get."""
    kind, floor = form['sigma_kind'], form['min_sigma']
    if kind == 1:
        sigma = F.softplus(raw) + floor
    elif kind == 2:
        f = max(floor, float(np.float32(1e-3)))
        sigma = f + F.softplus(raw - f)
    else:
        if form['has_bounds']:
            raw = raw.clamp(form['sigma_lo'], form['sigma_hi'])
        sigma = raw.exp()
        if floor <= 0:
            return sigma, raw
        sigma = sigma + floor
    return sigma, sigma.log()


def neglogp64(x, mu, sigma, logstd):
    return 0.5 * (((x - mu) / sigma) ** 2).sum(-1) + 0.5 * math.log(2.0 * math.pi) * x.shape[-1] + logstd.sum(-1)


def raw_inputs(rows, A, name, gen):
    """Raw head outputs; first: outside both bounds and on them, a softplus input above 20, sigma at its floor."""
    raw = torch.randn(rows, A, generator=gen) * 0.8 - 0.3
    edges = {'exp_bounds': [-3.0, 2.0, -1.0, 0.5], 'softplus_floor': [25.0, -9.0], 'linear_floor': [25.0, -9.0, 0.2],
             'exp_floor': [-7.0]}.get(name, [])
    flat = raw.view(-1)
    flat[:min(len(edges), flat.numel())] = torch.tensor(edges[:flat.numel()])
    return raw


def reference(c, form, surrogate, clip_value, bound_kind):
    """fp64: the loss of torch_fallback.ppo_loss, its gradients, the five scalars, the KL and the loss."""
    mu, raw, v = (c[k].double().requires_grad_() for k in ('mu', 'raw', 'v'))
    x, adv, vo, ret, m = (c[k].double() for k in ('x', 'adv', 'vo', 'ret', 'mask'))
    sigma, logstd = sigma64(raw, form)
    nlp = neglogp64(x, mu, sigma, logstd)
    ent = (0.5 + 0.5 * math.log(2.0 * math.pi) + sigma.log()).sum(-1)
    ratio = (c['onlp'].double() - nlp).exp()
    lo, hi = 1.0 - E_CLIP, 1.0 + E_CLIP
    if surrogate == 2:
        a = nlp * adv
    elif surrogate == 1:
        a = torch.max(-adv * ratio, -adv * ((hi - lo) / (1 + ((0.5 - (ratio - lo) / (hi - lo)) * 4).exp()) + lo))
    else:
        a = torch.max(-adv * ratio, -adv * ratio.clamp(lo, hi))
    cr = (ret - v) ** 2
    if clip_value:
        cr = torch.max((v - ret) ** 2, (vo + (v - vo).clamp(-E_CLIP, E_CLIP) - ret) ** 2)
    b = torch.zeros_like(nlp)
    if bound_kind == 1:
        b = ((mu + 1.1).clamp_max(0.0) ** 2 + (mu - 1.1).clamp_min(0.0) ** 2).sum(-1)
    elif bound_kind == 2:
        b = (mu * mu).sum(-1)
    osg, omu = c['osg'].double(), c['omu'].double()
    kl = ((osg / sigma + 1e-5).log() + (sigma ** 2 + (omu - mu) ** 2) / (2.0 * (osg ** 2 + 1e-5)) - 0.5).sum(-1)
    rows = torch.stack([a, cr, ent, b, kl.detach()])
    means = (rows * m).sum(-1) / m.sum().clamp(min=1.0)
    loss = means[0] + 0.5 * means[1] * COEF_C - means[2] * COEF_E + means[3] * COEF_B
    loss.backward()
    scalars = torch.cat([means.detach(), loss.detach().reshape(1)])
    return dict(d_mu=mu.grad, d_raw=raw.grad, d_v=v.grad, nlp=nlp.detach(), sigma=sigma.detach(), scalars=scalars)


def close(name, have, want):
    diff, scale = (have.double().cpu() - want).abs().max().item(), want.abs().max().item()
    print(name, 'max |diff|', diff, 'scale', scale)
    assert math.isfinite(diff) and diff <= 1e-5 * scale, (name, diff, scale)


@pytest.mark.parametrize('A', [1, 3, 8])
@pytest.mark.parametrize('rows', [1, 255, 257])
@pytest.mark.parametrize('name', list(FORMS))
def test_sigma_loss_and_its_gradients_equal_fp64(name, rows, A):
    from rl_games_amd import ops
    case = list(FORMS).index(name) + [1, 255, 257].index(rows) + 2 * [1, 3, 8].index(A)
    surrogate, clip_value, bound_kind, masked = OPTIONS[case % len(OPTIONS)]
    form = ops.sigma_form(FORMS[name])
    gen = torch.Generator().manual_seed(100 + case)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    pick = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (rows,), generator=gen)]
    c = dict(mu=rnd(rows, A) * 1.2, raw=raw_inputs(rows, A, name, gen), v=rnd(rows), adv=rnd(rows), ret=rnd(rows),
             omu=rnd(rows, A) * 1.2, osg=rnd(rows, A).abs() * 0.5 + 0.3, mask=torch.ones(rows))
    sigma = sigma64(c['raw'].double(), form)[0]
    c['x'] = (c['mu'].double() + sigma * rnd(rows, A).double()).float()
    # log ratio and value step on a grid that stays clear of log(1 +- e_clip) = -0.223 / 0.182 and of +- e_clip
    c['onlp'] = (neglogp64(c['x'].double(), c['mu'].double(), *sigma64(c['raw'].double(), form))
                 + pick([-0.5, -0.1, 0.05, 0.3]).double()).float()
    c['vo'] = c['v'] + pick([-0.5, -0.1, 0.1, 0.4])
    if masked:
        c['mask'] = (torch.rand(rows, generator=gen) < 0.6).float()
        c['mask'][:4] = 1.0                                               # (the rows of the edge inputs stay valid)
    ref = reference(c, form, surrogate, clip_value, bound_kind)
    g = {k: t.to(DEV) for k, t in c.items()}
    heads = torch.empty(rows, 1 + 2 * A, device=DEV)                     # [value | mu | raw sigma]: strided views
    heads[:, 0], heads[:, 1:1 + A], heads[:, 1 + A:] = g['v'], g['mu'], g['raw']
    d_heads = torch.full_like(heads, float('nan'))
    nlp = torch.full((rows,), float('nan'), device=DEV)
    blocks = ops.ppo_loss_sigma_blocks(rows)
    partials = torch.full((blocks, 7), float('nan'), dtype=torch.float64, device=DEV)
    scalars, kl_slot = torch.full((8,), float('nan'), device=DEV), torch.full((1,), float('nan'), device=DEV)
    mask = g['mask'] if masked else None
    ops.ppo_loss_sigma(heads[:, 1:1 + A], heads[:, 1 + A:], heads[:, 0], g['x'], g['onlp'], g['adv'], g['vo'], g['ret'],
                       g['omu'], g['osg'], d_heads[:, 1:1 + A], d_heads[:, 1 + A:], d_heads[:, 0], partials, form, E_CLIP,
                       COEF_C, COEF_E, COEF_B, clip_value, surrogate, bound_kind, True, mask,
                       mask.sum().reshape(1) if masked else None, new_neglogp=nlp)
    ops.ppo_loss_finalize(partials, blocks, 0, rows, masked, COEF_C, COEF_E, COEF_B, scalars, torch.zeros(1, device=DEV), kl_slot)
    close('d_values', d_heads[:, 0], ref['d_v'])
    close('d_mu', d_heads[:, 1:1 + A], ref['d_mu'])
    close('d_raw_sigma', d_heads[:, 1 + A:], ref['d_raw'])
    close('new_neglogp', nlp, ref['nlp'])
    assert torch.equal(g['omu'], g['mu'])                                 # written back
    close('sigma written back', g['osg'], ref['sigma'])
    for k, label in enumerate(('a_loss', 'c_loss', 'entropy', 'b_loss', 'kl', 'loss')):
        got, want = scalars[k].item(), ref['scalars'][k].item()
        print(label, got, 'fp64', want, 'err', abs(got - want))
        assert abs(got - want) <= 1e-5 * abs(want) + 2e-7, (label, got, want)
    assert kl_slot.item() == scalars[4].item() and scalars[6].item() == c['mask'].sum().item()


@pytest.mark.parametrize('rows,A,stats,env,last', [(1, 1, True, False, False), (65, 8, False, True, True),
                                                   (257, 1, False, False, True), (1, 8, True, True, True),
                                                   (65, 1, True, True, False), (257, 8, True, False, False)])
def test_sigma_rollout_head_equals_fp64(rows, A, stats, env, last):
    from rl_games_amd import ops
    case = [1, 65, 257].index(rows) * 2 + (A == 8)
    name = list(FORMS)[case % len(FORMS)]                                 # each form once (and exp twice)
    form = ops.sigma_form(FORMS[name])
    gen = torch.Generator().manual_seed(7 + case)
    H, step = 3, (2 if last else 0)
    heads = torch.randn(rows, 1 + 2 * A + 2, generator=gen) * 1.5         # (two columns nobody reads: ld > 1 + 2 A)
    heads[:, 0] *= 4.0                                                    # values beyond the +- 5 clamp
    heads[:, 1 + A:1 + 2 * A] = raw_inputs(rows, A, name, gen)
    noise = torch.randn(rows, A, generator=gen)
    mean, var, eps = torch.tensor([0.3], dtype=torch.float64), torch.tensor([2.5], dtype=torch.float64), 1e-5
    low, high = torch.linspace(-2.0, -1.0, A), torch.linspace(0.5, 3.0, A)
    hd = heads.to(DEV)
    poison = lambda *s: torch.full(s, float('nan'), device=DEV)
    storage = {'actions': poison(rows, H, A), 'mus': poison(rows, H, A), 'sigmas': poison(rows, H, A),
               'neglogpacs': poison(rows, H), 'values': poison(rows, H)}
    actions, values, env_out = poison(rows, A), poison(rows), poison(rows, A)
    ops.rollout_policy_head_sigma(hd, hd[:, 1 + A:1 + 2 * A], form, noise.to(DEV), (mean.to(DEV), var.to(DEV)) if stats else None,
                                  eps, actions, values, storage, H, step,
                                  env_actions=(env_out, low.to(DEV), high.to(DEV)) if env else None)
    mu = heads[:, 1:1 + A].double()
    sigma, logstd = sigma64(heads[:, 1 + A:1 + 2 * A].double(), form)
    close('actions', actions, mu + sigma * noise.double())
    assert torch.equal(storage['actions'][:, step], actions) and torch.equal(storage['mus'][:, step].cpu(), heads[:, 1:1 + A])
    close('sigmas', storage['sigmas'][:, step], sigma)
    # the neglogp of the action that was stored (what the update's ratio is taken against)
    close('neglogp', storage['neglogpacs'][:, step], neglogp64(actions.double().cpu(), mu, sigma, logstd))
    v = heads[:, 0].double()
    close('values', values, (var + eps).sqrt() * v.clamp(-5.0, 5.0) + mean if stats else v)
    assert torch.equal(storage['values'][:, step], values)
    if env:
        close('env actions', env_out, actions.double().cpu().clamp(-1.0, 1.0) * ((high - low) / 2).double() + ((high + low) / 2).double())
    assert all(torch.isnan(t[:, [s for s in range(H) if s != step]]).all() for t in storage.values())
