"""The discrete agent's fused rollout: the categorical head kernel (ops.rollout_categorical_head, csrc/
rollout_categorical.hip) against the torch path it replaces (DiscreteA2CModel's eval branch: CategoricalMasked,
Categorical.sample(), log_prob, denorm_value), and the agent's rollout with `fused_rollout` on against off, with the
step graphs on against off, and after restore() / set_weights between epochs."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, STEP = 4, 2


def _torch_head(logits, value, sizes, masks, vstats):
    """The eval branch of DiscreteA2CModel.forward on given heads: (actions [N, B], neglogp [N], values [N], p / q of
    every branch).  Consumes the default generator as the model does."""
    from rl_games_amd.policy import DiscreteA2CModel
    heads = torch.split(logits, sizes, dim=1)
    ms = [None] * len(sizes) if masks is None else torch.split(masks, sizes, dim=1)
    dists = [DiscreteA2CModel._dist(h, m)[0] for h, m in zip(heads, ms)]
    acts = [d.sample().long() for d in dists]
    nlp = sum(-d.log_prob(a) for d, a in zip(dists, acts))
    v = value if vstats is None else vstats(value, denorm=True)
    return torch.stack(acts, dim=1), nlp, v.reshape(-1), [d.probs for d in dists]


def _value_stats(on):
    if not on:
        return None
    from rl_games_amd.normalizers import RunningMeanStd
    vm = RunningMeanStd((1,)).to(DEV)
    vm.running_mean.fill_(0.75)
    vm.running_var.fill_(2.5)
    vm.eval()
    return vm


def _buffers(N, B, multi):
    return {'actions': torch.full((N, H, B) if multi else (N, H), -7, dtype=torch.int64, device=DEV),
            'neglogpacs': torch.full((N, H), 1234.5, device=DEV), 'values': torch.full((N, H, 1), -99.0, device=DEV)}


def _run_kernel(logits, value, sizes, masks, vstats, seed, noise=None):
    from rl_games_amd import ops
    N, B = value.shape[0], len(sizes)
    storage = _buffers(N, B, B > 1)
    own = noise is None
    if own:
        torch.manual_seed(seed)
        noise = torch.empty(N * sum(sizes) + 5, device=DEV)
        at = 0
        for n in sizes:
            noise[at:at + N * n].view(N, n).exponential_()
            at += N * n
    acts = torch.empty((N, B) if B > 1 else (N,), dtype=torch.int64, device=DEV)
    vals = torch.empty(N, device=DEV)
    vs = None if vstats is None else (vstats.running_mean, vstats.running_var)
    ops.rollout_categorical_head(logits, value, sizes, noise, masks, vs, 1e-5 if vstats is None else vstats.epsilon,
                                 acts, vals, storage, H, STEP)
    after = torch.rand(3, device=DEV) if own else None
    return acts.view(N, B), vals, storage, after


def _heads(N, sizes, shared, gen):
    """(logits view, value view) with row strides: the chain's [value | logits] tensor, or two separate tensors."""
    S = sum(sizes)
    if shared:
        t = (torch.rand(N, 1 + S + 3, generator=gen, device=DEV) * 2 - 1) * 30
        return t[:, 1:1 + S], t[:, :1]
    lg = (torch.rand(N, S + 2, generator=gen, device=DEV) * 2 - 1) * 30
    v = torch.randn(N, 3, generator=gen, device=DEV) * 4
    return lg[:, :S], v[:, 1:2]


def _masks(N, sizes, gen):
    """Random masks with, in every branch, some rows with one allowed action and some with none."""
    S = sum(sizes)
    m = torch.rand(N, S, generator=gen, device=DEV) > 0.4
    at = 0
    for n in sizes:
        one = torch.arange(N, device=DEV) % 7 == 3
        m[one, at:at + n] = False
        m[one, at + (torch.arange(N, device=DEV)[one] % n)] = True
        m[torch.arange(N, device=DEV) % 11 == 5, at:at + n] = False
        at += n
    return m


@pytest.mark.parametrize('N', [1, 63, 300, 4096, 65536])
@pytest.mark.parametrize('sizes', [[2], [6], [17], [3, 5, 2], [1, 4], [3, 70]])
def test_categorical_head_matches_torch(N, sizes):
    """Same seed, same heads: the kernel's actions are the torch path's except at near-ties of p / q (none expected at
    these counts); neglogp / values to 1e-6; masked actions never chosen; only slot STEP written; the generator left
    where the torch path leaves it.  [3, 70]: a row too wide for the LDS tile form (the one-wave-per-row form)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(N * 31 + len(sizes))
    for shared in (True, False):
        for masked in (False, True):
            for norm in (False, True):
                logits, value = _heads(N, sizes, shared, gen)
                masks = _masks(N, sizes, gen) if masked else None
                vstats = _value_stats(norm)
                seed = 17 + N
                torch.manual_seed(seed)
                ref_a, ref_nlp, ref_v, probs = _torch_head(logits, value, sizes, masks, vstats)
                ref_after = torch.rand(3, device=DEV)
                acts, vals, storage, after = _run_kernel(logits, value, sizes, masks, vstats, seed)
                assert torch.equal(after, ref_after), 'generator use differs from Categorical.sample()'
                # near-ties of the torch path's p / q (the draws regenerated in the same order)
                torch.manual_seed(seed)
                ratios = [p / torch.empty_like(p).exponential_() for p in probs]
                tie = torch.zeros(N, dtype=torch.bool, device=DEV)
                for r in ratios:
                    if r.shape[1] > 1:
                        top = r.topk(2, dim=1).values
                        tie |= (top[:, 0] - top[:, 1]) <= 1e-6 * top[:, 0]
                diff = (acts != ref_a).any(dim=1)
                assert not (diff & ~tie).any(), 'actions differ away from a near-tie'
                assert int(diff.sum()) <= max(1, 1e-5 * N)
                same = ~diff
                assert torch.allclose(storage['neglogpacs'][:, STEP][same], ref_nlp.reshape(-1)[same], rtol=1e-6, atol=1e-6)
                assert torch.allclose(vals, ref_v, rtol=1e-6, atol=1e-6)
                assert torch.equal(storage['values'][:, STEP, 0], vals)
                buf_a = storage['actions'][:, STEP].reshape(N, -1)
                assert torch.equal(buf_a, acts)
                at = 0
                for b, n in enumerate(sizes):
                    assert ((acts[:, b] >= 0) & (acts[:, b] < n)).all()
                    if masks is not None:
                        mb = masks[:, at:at + n]
                        some = mb.any(dim=1)
                        chosen = mb.gather(1, acts[:, b:b + 1]).squeeze(1)
                        assert chosen[some].all(), 'a masked action was chosen'
                    at += n
                others = [t for t in range(H) if t != STEP]
                assert (storage['actions'][:, others] == -7).all()
                assert (storage['neglogpacs'][:, others] == 1234.5).all()
                assert (storage['values'][:, others] == -99.0).all()


@pytest.mark.parametrize('sizes', [[4], [3, 100]])
def test_categorical_head_crafted_draws(sizes):
    """Crafted q: exact ties of p / q go to the lowest index (within a lane and across lanes of the wave form), and a
    row with every action masked stays uniform (the smallest q wins)."""
    N, S, n = 5, sum(sizes), sizes[-1]
    c0 = S - n
    logits = torch.zeros(N, S, device=DEV)
    noise = torch.full((N * S,), 2.0, device=DEV)
    last = noise[N * c0:].view(N, n)
    # row 0: everything equal -> column 0
    last[1, [n - 3, n - 1]] = 1.0                 # row 1: two equal maxima -> the lower column
    logits[2, c0 + 1:] = 3.0                      # row 2: equal maxima at columns 1.. -> column 1
    last[3, n - 2] = 0.5                          # row 3: every action masked -> the smallest q
    last[4, [(n - 1) % 64, n - 1]] = 1.0          # row 4: equal maxima 64 columns apart (one lane of the wave form)
    masks = torch.ones(N, S, dtype=torch.bool, device=DEV)
    masks[3] = False
    acts, vals, storage, _ = _run_kernel(logits, torch.zeros(N, 1, device=DEV), sizes, masks, None, 0, noise=noise)
    got = acts[:, -1].tolist()
    assert got == [0, n - 3, 1, n - 2, (n - 1) % 64], got
    if len(sizes) > 1:
        assert acts[:, 0].tolist() == [0] * N
    # the all-masked row's neglogp is torch's: -(-1e8 - (log(n) + -1e8)) per branch, in fp32
    floor = torch.tensor(-1e8)
    want = sum(-(floor - (torch.log(torch.tensor(float(k))) + floor)) for k in sizes)
    assert storage['neglogpacs'][3, STEP].item() == float(want)


def test_categorical_head_rejects_more_than_16_branches():
    from rl_games_amd import _lib, ops
    sizes = [2] * 17
    N = 8
    with pytest.raises(_lib.HipLibraryError, match='hipError_t 801'):
        _run_kernel(torch.zeros(N, 34, device=DEV), torch.zeros(N, 1, device=DEV), sizes, None, None, 0,
                    noise=torch.ones(N * 34, device=DEV))
    assert ops.CATEGORICAL_MAX_BRANCHES == 16


# ----------------------------------------------------------------------------- the agent

def _params(layout, norm, num_actors=64, horizon=16, **over):
    from rl_games_amd import configs
    params = configs.cartpole_discrete(num_actors=num_actors, device=DEV, normalize_input=norm, normalize_value=norm,
                                       horizon_length=horizon, minibatch_size=num_actors * horizon // 2, **over)
    net = params['network']
    net['separate'] = layout in ('separate', 'separate_tanh_wide')
    if layout == 'multi_discrete_masked':
        net['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
        params['config']['use_action_masks'] = True
        params['config']['env_config'].update(discrete_actions=[3, 5, 2], obs_dim=12, action_masks=True)
    if layout == 'shared':
        params['config']['env_config'].update(obs_dim=8, discrete_actions=4)
    if layout == 'separate_tanh_wide':
        net['mlp'].update(units=[128, 64, 32], activation='tanh')
        params['config']['env_config'].update(obs_dim=20, discrete_actions=6)
    return params


_FIELDS = ('obses', 'dones', 'actions', 'neglogpacs', 'values', 'action_masks')


def _agent(params, seed=4):
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    torch.manual_seed(seed)
    agent = DiscreteA2CAgent('droll', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    batches = []
    play = agent.play_steps

    def recording_play_steps():
        batch = play()
        batches.append({k: batch[k].clone() for k in _FIELDS if k in batch})
        return batch
    agent.play_steps = recording_play_steps
    return agent, batches


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('layout', ['separate', 'shared', 'multi_discrete_masked', 'separate_tanh_wide'])
def test_fused_rollout_matches_torch_rollout(layout, norm):
    """Two epochs (the second replays the step graphs) with `fused_rollout` on and off at the same seed: identical
    observations, dones and actions; neglogpacs / values to 1e-5 (the chain forward's rounding)."""
    out = {}
    for fused in (True, False):
        agent, batches = _agent(_params(layout, norm, fused_rollout=fused))
        assert agent._fast_rollout_ok() == fused
        for _ in range(2):
            agent.epoch_num += 1
            agent.train_epoch()
        if fused:
            assert len(agent._rollout_graphs) > 0
        out[fused] = batches
    for a, b in zip(out[True], out[False]):
        assert a.keys() == b.keys()
        for k in ('obses', 'dones', 'actions', 'action_masks'):
            if k in a:
                assert torch.equal(a[k], b[k]), k
        for k in ('neglogpacs', 'values'):
            assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-6), (k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize('layout,num_actors', [('multi_discrete_masked', 64), ('separate', 64), ('shared', 16384)])
def test_rollout_graphs_replay_the_eager_rollout(layout, num_actors):
    """Three epochs with the step graphs on and off: every rollout tensor bit-identical, and graphs were captured
    (a captured step holds no host read).  16,384 envs: the chain's inference forward on split planes."""
    horizon = 4 if num_actors > 1024 else 16
    out = {}
    for graphs in (True, False):
        agent, batches = _agent(_params(layout, True, num_actors=num_actors, horizon=horizon, rollout_graphs=graphs))
        for _ in range(3):
            agent.epoch_num += 1
            agent.train_epoch()
        assert (len(agent._rollout_graphs) > 0) == graphs
        out[graphs] = batches
    for a, b in zip(out[True], out[False]):
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('how', ['restore', 'set_weights'])
@pytest.mark.parametrize('num_actors', [64, 16384])
def test_replayed_rollout_sees_new_weights(how, num_actors, tmp_path):
    """restore() / set_weights between epochs: the next rollout, replayed from graphs captured for the old weights,
    equals a fresh agent's eager rollout from the same weights, observations and seed."""
    horizon = 4 if num_actors > 1024 else 16
    params = _params('separate_tanh_wide', True, num_actors=num_actors, horizon=horizon)
    donor, _ = _agent(params, seed=11)
    donor.epoch_num += 1
    donor.train_epoch()
    path = donor.save(str(tmp_path / 'donor'))
    weights = donor.get_weights()
    trained, got = _agent(params, seed=4)
    for _ in range(2):
        trained.epoch_num += 1
        trained.train_epoch()
    assert len(trained._rollout_graphs) > 0
    fresh, ref = _agent(params, seed=5)
    for agent in (trained, fresh):
        if how == 'restore':
            agent.restore(path)
        else:
            agent.set_weights(weights)
        agent.vec_env.seed(321)
        agent.obs = agent.env_reset()
        agent.dones = torch.ones_like(agent.dones)
        agent.set_eval()
        torch.manual_seed(99)
        with torch.no_grad():
            agent.play_steps()
    assert len(fresh._rollout_graphs) == 0 and fresh._fast_rollout_ok()
    for k in got[-1]:
        assert torch.equal(got[-1][k], ref[-1][k]), k
