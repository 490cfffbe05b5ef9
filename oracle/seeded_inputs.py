"""TEST INFRASTRUCTURE ONLY - seeded synthetic inputs shared by tests/, the golden-fixture
generator and bench.py's parity checks."""
import torch


def gae_inputs(horizon, num_envs, value_size, seed=0, p_done=0.15):
    """Seeded GAE inputs, generated exactly like the reference's own test factory
    (tests/test_triton_gae.py:45-52): one CPU generator, draw order rewards, values, dones,
    last_values, last_dones."""
    g = torch.Generator().manual_seed(seed)
    rewards = torch.randn(horizon, num_envs, value_size, generator=g)
    values = torch.randn(horizon, num_envs, value_size, generator=g)
    dones = (torch.rand(horizon, num_envs, generator=g) < p_done).float()
    last_values = torch.randn(num_envs, value_size, generator=g)
    last_dones = (torch.rand(num_envs, generator=g) < p_done).float()
    return rewards, values, dones, last_values, last_dones


# ------------------------------------------------------------------ PPO loss
def loss_inputs(mb, A, seed, mu=None, values=None):
    """SURVEY 8d kernel-level inputs of the continuous PPO loss: (mu [mb, A], logstd [A], values [mb, 1], batch) with the
    batch keys of the oracle (ppo_oracle.distribution_loss_and_grads).  Both clip sides fire (old neglogp = new neglogp +
    0.2 N(0, 1): ratios on both sides of [1 - e, 1 + e] and inside it) and the bound loss is active (|mu| > 1.1 in places).
    mu / values given (a network's outputs): the same draws in the same order, the OLD policy and the old values are then
    placed around them instead of the new ones around the old."""
    from oracle import ppo_oracle as O
    gen = torch.Generator().manual_seed(seed)
    old_nlp = torch.randn(mb, generator=gen)
    batch = {
        'old_logp_actions': old_nlp,
        'advantages': torch.randn(mb, generator=gen),
        'old_values': torch.randn(mb, 1, generator=gen),
        'returns': torch.randn(mb, 1, generator=gen),
        'actions': torch.randn(mb, A, generator=gen),
        'mu': 1.2 * torch.randn(mb, A, generator=gen),
        'sigma': torch.exp(0.1 * torch.randn(mb, A, generator=gen)),
    }
    d_mu = 0.1 * torch.randn(mb, A, generator=gen)
    logstd = 0.1 * torch.randn(A, generator=gen)
    d_values = 0.3 * torch.randn(mb, 1, generator=gen)
    if mu is None:
        mu = batch['mu'] + d_mu
    else:
        mu = mu.detach().clone().reshape(mb, A)
        batch['mu'] = mu - d_mu
    if values is None:
        values = batch['old_values'] + d_values
    else:
        values = values.detach().clone().reshape(mb, 1)
        batch['old_values'] = values - d_values
    # make neglogp land near old_neglogp so that ratios straddle the clip range
    with torch.no_grad():
        sigma = torch.exp(logstd)
        nlp = O.neglogp(batch['actions'], mu, mu * 0 + sigma, mu * 0 + logstd)
        batch['old_logp_actions'] = nlp + 0.2 * torch.randn(mb, generator=gen)
    return mu, logstd, values, batch


# ------------------------------------------------------------------ optimiser step
# (length, truncation, weight_decay, grad_scale, betas, eps, step counter before the first step): a covering set - every
# value of every option appears with at least two lengths, one of them with a tail (length % 4 != 0).
# 1024 = exactly one block of vector threads of adam_step_kernel, 1027 = three tail threads that open a second block.
_B_A, _B_B = (0.9, 0.999), (0.8, 0.99)
_THIRD = 1.0 / 3.0          # world 3 (rounded to fp32 by ops.adam_step)
ADAM_CASES = [
    (1, 'off', 0.0, 1.0, _B_A, 1e-8, 0),
    (2, 'active', 1e-2, 0.25, _B_B, 1e-5, 1),
    (3, 'inactive', 0.0, _THIRD, _B_A, 1e-5, 999),
    (4, 'active', 1e-2, 1.0, _B_B, 1e-8, 99999),
    (5, 'inactive', 1e-2, _THIRD, _B_A, 1e-8, 0),
    (7, 'off', 1e-2, 0.25, _B_B, 1e-5, 999),
    (8, 'active', 0.0, _THIRD, _B_B, 1e-8, 1),
    (1023, 'inactive', 1e-2, 1.0, _B_A, 1e-5, 99999),
    (1024, 'off', 0.0, 0.25, _B_A, 1e-8, 1),
    (1025, 'active', 1e-2, _THIRD, _B_B, 1e-5, 0),
    (1027, 'inactive', 0.0, 0.25, _B_B, 1e-8, 99999),
    (123921, 'active', 1e-2, _THIRD, _B_A, 1e-8, 999),
    (123921, 'off', 0.0, 1.0, _B_B, 1e-5, 0),
]
ADAM_STEPS = 3
ADAM_LR = 3e-4
ADAM_KLS = (0.02, 0.001, 0.008)     # the minibatch KL of each step: the adaptive rule divides, multiplies, keeps the lr
# the non-finite-gradient test (one element of the first gradient replaced) and the FlatAdam round trip (4 steps from
# zero moments over a small model of 115 parameters)
ADAM_NONFINITE_CASE = (1027, 'active', 1e-2, 1.0, _B_A, 1e-8, 1)
ADAM_NONFINITE_INDEX = 5
ADAM_FLAT_CASE = (115, 'active', 1e-2, 1.0, _B_B, 1e-8, 0)
ADAM_FLAT_SHAPES = [(7, 12), (7,), (3, 7), (3,)]
ADAM_FLAT_STEPS = 4
ADAM_FLAT_KL = 0.001      # below half the threshold of 0.008: the adaptive rule multiplies the lr by 1.5 at every step


def adam_case_id(case):
    n, trunc, wd, gs, betas, eps, start = case
    return f'n{n}-{trunc}-wd{wd:g}-gs{gs:.3g}-b{betas[0]:g}-eps{eps:g}-t{start}'


def adam_inputs(case, steps=ADAM_STEPS, zero_moments=False):
    """Seeded optimiser state and gradients of one ADAM_CASES row, as numpy fp32: dict(p, m, v, grads [steps], max_norm).
    The first gradient is large (3.0) and the later ones small (0.01), like a first and a late minibatch.  max_norm is
    None ('off'), a power of two below half the smallest norm of the scaled gradients ('active': every step is clipped)
    or one above twice the largest ('inactive': the coefficient is 1 at every step) - exact in fp32."""
    import math
    import numpy as np
    n, trunc, _, gs, _, _, _ = case
    gen = torch.Generator().manual_seed(1000 + n)
    p = (torch.randn(n, generator=gen) * 0.1).numpy()
    m = (torch.randn(n, generator=gen) * 0.01).numpy()
    v = (torch.rand(n, generator=gen) * 1e-3).numpy()
    if zero_moments:
        m, v = m * 0, v * 0
    grads = [(torch.randn(n, generator=gen) * (3.0 if k == 0 else 0.01)).numpy() for k in range(steps)]
    norms = [math.sqrt(float(np.sum((g.astype(np.float64) * float(np.float32(gs))) ** 2))) for g in grads]
    max_norm = None
    if trunc == 'active':
        max_norm = 2.0 ** (math.floor(math.log2(min(norms))) - 1)
    elif trunc == 'inactive':
        max_norm = 2.0 ** (math.ceil(math.log2(max(norms))) + 1)
    return dict(p=p, m=m, v=v, grads=grads, max_norm=max_norm)
