"""CPU: the oracle and the host-side mirrors checked against the real reference's own functions,
modules and builders on seeded inputs.

Pins the rows SURVEY 8c lists as 'parity unpinned' (clipped surrogate, value loss, bound loss,
policy_kl, advantage normalisation) to outputs of the reference functions themselves on seeded
inputs, plus RunningMeanStd / GeneralizedMovingStats / apply_masks / schedulers / PPODataset /
ExperienceBuffer semantics.

The reference's side of every comparison is a recording: tests/golden/vs_reference/<test>.pt holds what
the reference computed on exactly these inputs (one file per test function, keyed by the case's id), so the
suite runs without a reference checkout.  Each test hands its reference side to the `reference` fixture as a
function; with RLG_RECORD_REFERENCE=1 (and the checkout that tests/golden/ref_import.py finds) that function
runs the real reference, the test applies its assertions to the live result, and the results are written
back to the golden files:

    RLG_RECORD_REFERENCE=1 python -m pytest tests/test_vs_reference_cpu.py
"""
import copy
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ref_import  # noqa: E402

RECORD = os.environ.get('RLG_RECORD_REFERENCE') == '1'
if RECORD:
    ref_import.enable()                                 # (recording needs the checkout: ReferenceUnavailable otherwise)
REF_DIR = os.path.join(HERE, 'golden', 'vs_reference')
_recorded = {}                                          # test function -> {case id: recording}

from oracle import ppo_oracle as O  # noqa: E402


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _frozen(x):
    """Detached copies of the tensors inside nested dicts / lists / tuples (what a recording holds)."""
    if isinstance(x, torch.Tensor):
        return x.detach().clone()
    if isinstance(x, dict):
        return type(x)((k, _frozen(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return type(x)(_frozen(v) for v in x)
    return x


def _ref_file(function):
    return os.path.join(REF_DIR, function + '.pt')


@functools.lru_cache(maxsize=None)
def _stored(function):
    return torch.load(_ref_file(function), map_location='cpu', weights_only=False)


@pytest.fixture(autouse=True)
def _one_thread():
    """Every test, recorded or replayed, runs its CPU ops on one intra-op thread: the reductions inside them (batch-norm
    statistics, for one) round differently with the thread count, and the comparisons are bit for bit.  (Per test: the
    reference's Runner sets the process's thread count itself.)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope='module', autouse=True)
def _write_recording():
    yield
    if RECORD and _recorded:
        os.makedirs(REF_DIR, exist_ok=True)
        for function, cases in _recorded.items():
            path = _ref_file(function)
            merged = torch.load(path, map_location='cpu', weights_only=False) if os.path.exists(path) else {}
            merged.update(cases)
            torch.save(dict(sorted(merged.items())), path)


@pytest.fixture
def reference(request):
    """reference(fn): the reference's side of this test - fn() run against the real reference (RLG_RECORD_REFERENCE=1,
    recorded under the test's id) or the recorded result."""
    def get(fn):
        function, key = request.node.originalname, request.node.name
        if RECORD:
            _recorded.setdefault(function, {})[key] = _frozen(fn())
            return copy.deepcopy(_recorded[function][key])
        stored = _stored(function)
        assert key in stored, f'{key}: no recording in {_ref_file(function)} (RLG_RECORD_REFERENCE=1 writes it)'
        return copy.deepcopy(stored[key])
    return get


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_losses_and_kl_equal_reference_functions(seed, reference):
    g = gen(seed)
    mb, A = 4096, 21
    old_nlp = torch.randn(mb, generator=g)
    nlp = old_nlp + 0.2 * torch.randn(mb, generator=g)
    adv = torch.randn(mb, generator=g)
    v_old = torch.randn(mb, 1, generator=g)
    v = v_old + 0.3 * torch.randn(mb, 1, generator=g)
    R = torch.randn(mb, 1, generator=g)
    mu = 1.2 * torch.randn(mb, A, generator=g)
    s0 = torch.exp(0.1 * torch.randn(mb, A, generator=g))
    s1 = torch.exp(0.1 * torch.randn(mb, A, generator=g))
    mu1 = mu + 0.1 * torch.randn(mb, A, generator=g)
    mask = (torch.rand(mb, generator=g) < 0.7).float()
    losses = [adv.unsqueeze(1), v, R]

    def ref_side():
        from rl_games.common import common_losses
        from rl_games.algos_torch import torch_ext
        return {'ppo': common_losses.actor_loss(old_nlp, nlp, adv, True, 0.2),
                'smoothed': common_losses.smoothed_actor_loss(old_nlp, nlp, adv, True, 0.2),
                'a2c': common_losses.actor_loss(old_nlp, nlp, adv, False, 0.2),
                'critic': {clip: common_losses.default_critic_loss(v_old, v, 0.2, R, clip) for clip in (True, False)},
                'kl': torch_ext.policy_kl(mu, s0, mu1, s1, True),
                'kl_rows': torch_ext.policy_kl(mu, s0, mu1, s1, False),
                'masked_means': [torch_ext.apply_masks(losses, m)[0] for m in (None, mask)],
                'normalized_masked': torch_ext.normalization_with_masks(adv, mask)}
    ref = reference(ref_side)
    assert torch.equal(O.actor_loss(old_nlp, nlp, adv, 0.2), ref['ppo'])
    assert torch.equal(O.actor_loss(old_nlp, nlp, adv, 0.2, smooth=True), ref['smoothed'])
    assert torch.equal(O.actor_loss(old_nlp, nlp, adv, 0.2, ppo=False), ref['a2c'])
    for clip in (True, False):
        assert torch.equal(O.critic_loss(v_old, v, 0.2, R, clip), ref['critic'][clip])
    assert torch.equal(O.policy_kl(mu, s0, mu1, s1), ref['kl'])
    assert torch.equal(O.policy_kl(mu, s0, mu1, s1, mask), (ref['kl_rows'] * mask).sum() / mask.sum().clamp(min=1.0))
    # apply_masks
    for m, theirs in zip((None, mask), ref['masked_means']):
        mine, _ = O.masked_means(losses, m)
        assert all(torch.equal(a, b) for a, b in zip(mine, theirs))
    # advantage normalisation (a2c_common.py:1634) and its masked variant
    assert torch.equal(O.normalize_advantages(adv), (adv - adv.mean()) / (adv.std() + 1e-8))
    assert torch.equal(O.normalize_advantages(adv, mask), ref['normalized_masked'])


def test_bound_losses_equal_reference_methods(reference):
    mu = 1.5 * torch.randn(1000, 8, generator=gen(3))

    def ref_side():
        from rl_games.algos_torch.a2c_continuous import A2CAgent as RefAgent

        class Stub:
            bounds_loss_coef = 1e-4
        return {'bound': RefAgent.bound_loss(Stub(), mu), 'regularisation': RefAgent.reg_loss(Stub(), mu)}
    ref = reference(ref_side)
    assert torch.equal(O.bound_loss(mu, 'bound'), ref['bound'])
    assert torch.equal(O.bound_loss(mu, 'regularisation'), ref['regularisation'])


def test_neglogp_and_entropy_equal_reference_model(reference):
    g = gen(4)
    x, mu = torch.randn(512, 21, generator=g), torch.randn(512, 21, generator=g)
    logstd = (0.2 * torch.randn(21, generator=g)).expand(512, 21)
    sigma = torch.exp(logstd)

    def ref_side():
        from rl_games.algos_torch.models import ModelA2CContinuousLogStd
        return ModelA2CContinuousLogStd.Network.neglogp(None, x, mu, sigma, logstd)
    ref = reference(ref_side)
    assert torch.equal(O.neglogp(x, mu, sigma, logstd), ref)
    assert torch.equal(O.normal_entropy(mu, sigma), torch.distributions.Normal(mu, sigma).entropy().sum(-1))


@pytest.mark.parametrize('shape', [(1,), (12,)])
def test_running_mean_std_equals_reference_module(shape, reference):
    g = gen(5)
    feed = []
    for it in range(4):
        x = torch.randn(300, shape[0], generator=g) * (it + 1) + it
        mask = (torch.rand(300, generator=g) < 0.8).float().unsqueeze(1) if (it == 2 and shape[0] == 1) else None
        feed.append((x, mask))
    x_eval = torch.randn(50, shape[0], generator=g) * 9

    def ref_side():
        from rl_games.algos_torch.running_mean_std import RunningMeanStd
        ref = RunningMeanStd(shape)
        steps = []
        for x, mask in feed:
            ref.train()
            y = ref(x, mask=mask)
            steps.append(_frozen({'y': y, 'running_mean': ref.running_mean, 'running_var': ref.running_var,
                                  'count': ref.count.item()}))
        ref.eval()
        return {'steps': steps, 'eval': ref(x_eval), 'denorm': ref(x_eval, denorm=True)}
    ref = reference(ref_side)
    state = O.new_running_stats(shape[0])
    for (x, mask), want in zip(feed, ref['steps']):
        y, state = O.running_stats_forward(state, x, True, mask=mask)
        assert torch.equal(y, want['y'])
        assert torch.equal(state['running_mean'], want['running_mean'])
        assert torch.equal(state['running_var'], want['running_var'])
        assert state['count'].item() == want['count']
    assert torch.equal(O.running_stats_forward(state, x_eval, False)[0], ref['eval'])
    assert torch.equal(O.running_stats_forward(state, x_eval, False, denorm=True)[0], ref['denorm'])


def test_moving_stats_equal_reference_module(reference):
    g = gen(6)
    feed = []
    for it in range(3):
        x = torch.randn(2000, generator=g) * (it + 1)
        mask = (torch.rand(2000, generator=g) < 0.6).float() if it == 1 else None
        feed.append((x, mask))

    def ref_side():
        from rl_games.algos_torch.moving_mean_std import GeneralizedMovingStats
        ref = GeneralizedMovingStats((1,), decay=0.5)
        ref.train()
        steps = []
        for x, mask in feed:
            y = ref(x, mask=mask)
            steps.append(_frozen({'y': y, **{k: getattr(ref, k) for k in ('mean', 'sqrs', 'step')}}))
        return steps
    ref = reference(ref_side)
    state = O.new_moving_stats(1)
    for (x, mask), want in zip(feed, ref):
        y, state = O.moving_stats_forward(state, x, True, 0.5, mask=mask)
        assert torch.equal(y, want['y'])
        for k in ('mean', 'sqrs', 'step'):
            assert torch.equal(state[k], want[k])


def test_schedulers_equal_reference(reference):
    from rl_games_amd import lr_control as mine
    kls = (0.02, 0.001, 0.008, 0.5, 1e-5, 0.016, 0.004)
    eps = (0, 1, 50, 99, 100, 150)

    def ref_side():
        from rl_games.common import schedulers as ref
        a = ref.AdaptiveScheduler(0.008)
        lr, adaptive = 3e-4, []
        for kl in kls:
            adaptive.append(a.update(lr, 0.0, 0, 0, kl))
            lr = a.update(lr, 0.0, 0, 0, kl)[0]
        la = ref.LinearScheduler(3e-4, max_steps=100, apply_to_entropy=True, start_entropy_coef=0.01)
        return {'adaptive': adaptive, 'linear': [la.update(0, 0.01, ep, 0, 0) for ep in eps]}
    ref = reference(ref_side)
    b = mine.AdaptiveScheduler(0.008)
    lr = 3e-4
    for kl, want in zip(kls, ref['adaptive']):
        assert want == b.update(lr, 0.0, 0, 0, kl)
        assert b.update(lr, 0.0, 0, 0, kl)[0] == O.adaptive_lr(lr, kl)
        lr = want[0]
    lb = mine.LinearScheduler(3e-4, max_steps=100, apply_to_entropy=True, start_entropy_coef=0.01)
    for ep, want in zip(eps, ref['linear']):
        assert want == lb.update(0, 0.01, ep, 0, 0)
        assert lb.update(0, 0.01, ep, 0, 0)[0] == O.linear_lr(3e-4, ep, 100)


def test_ppo_dataset_equals_reference(reference):
    from rl_games_amd.minibatch import PPODataset as Mine
    B, mb = 64, 16
    vals = {'obs': torch.arange(B * 3).reshape(B, 3).float(), 'advantages': torch.arange(B).float(),
            'mu': torch.zeros(B, 2), 'sigma': torch.zeros(B, 2), 'rnn_states': None, 'rnn_masks': None}
    rs = [torch.arange(2 * 16 * 5).reshape(2, 16, 5).float()]

    def ref_side():
        from rl_games.common.datasets import PPODataset as Ref
        r = Ref(B, mb, False, False, 'cpu', 4)
        r.update_values_dict({k: (v.clone() if v is not None else None) for k, v in vals.items()})
        items = []
        for i in range(len(r)):
            items.append(_frozen(dict(r[i])))
            r.update_mu_sigma(torch.full((mb, 2), float(i)), torch.full((mb, 2), 2.0 * i))
        r2 = Ref(B, mb, False, True, 'cpu', 4)
        r2.update_values_dict({'obs': vals['obs'].clone(), 'rnn_states': rs})
        rnn = [(r2[i]['obs'], r2[i]['rnn_states'][0]) for i in range(len(r2))]
        return {'len': len(r), 'items': items, 'mu': r.values_dict['mu'], 'len_rnn': len(r2), 'rnn': rnn}
    ref = reference(ref_side)
    m = Mine(B, mb, False, False, 'cpu', 4)
    m.update_values_dict({k: (v.clone() if v is not None else None) for k, v in vals.items()})
    assert ref['len'] == len(m)
    for i in range(len(m)):
        a, b = ref['items'][i], m[i]
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k])
        m.update_mu_sigma(torch.full((mb, 2), float(i)), torch.full((mb, 2), 2.0 * i))
    assert torch.equal(ref['mu'], m.values_dict['mu'])
    # rnn slicing
    m2 = Mine(B, mb, False, True, 'cpu', 4)
    m2.update_values_dict({'obs': vals['obs'].clone(), 'rnn_states': rs})
    assert ref['len_rnn'] == len(m2)
    for i in range(len(m2)):
        assert torch.equal(ref['rnn'][i][0], m2[i]['obs'])
        assert torch.equal(ref['rnn'][i][1], m2[i]['rnn_states'][0])
    with pytest.raises(ValueError):
        Mine(10, 3, False, False, 'cpu', 1)


def test_experience_buffer_equals_reference_layout_and_flatten(reference):
    from rl_games_amd.rollout_buffer import ExperienceBuffer as Mine
    from rl_games_amd.agent import swap_and_flatten01
    from rl_games_amd.spaces import Box
    env_info = {'observation_space': Box(-np.inf, np.inf, (7,), np.float32),
                'action_space': Box(-1, 1, (3,), np.float32), 'agents': 1, 'value_size': 1}
    algo = {'num_actors': 5, 'horizon_length': 4, 'has_central_value': False, 'use_action_masks': False}
    names = ['actions', 'neglogpacs', 'values', 'mus', 'sigmas', 'obses', 'states', 'dones']
    m = Mine(env_info, algo, 'cpu')
    g = gen(8)
    vals = [{k: (torch.rand(t.shape[1:], generator=g) * 5).to(t.dtype) for k, t in m.tensor_dict.items()} for _ in range(4)]

    def ref_side():
        from rl_games.common.experience import ExperienceBuffer as Ref
        from rl_games.common.a2c_common import swap_and_flatten01 as ref_flatten
        r = Ref(env_info, algo, 'cpu')
        layout = {k: (tuple(t.shape), t.dtype) for k, t in r.tensor_dict.items()}
        for n in range(4):
            for k in r.tensor_dict:
                r.update_data(k, n, vals[n][k])
        return {'layout': layout, 'flat': r.get_transformed_list(ref_flatten, names)}
    ref = reference(ref_side)
    assert ref['layout'].keys() == m.tensor_dict.keys()
    for k, (shape, dtype) in ref['layout'].items():
        assert shape == tuple(m.tensor_dict[k].shape) and dtype == m.tensor_dict[k].dtype
    for n in range(4):
        for k in m.tensor_dict:
            m.update_data(k, n, vals[n][k])
    a, b = ref['flat'], m.get_transformed_list(swap_and_flatten01, names)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert b[k].data_ptr() == m.storage[k].data_ptr()       # zero-copy in the env-major layout


def test_reference_restores_amd_checkpoint(tmp_path, reference):
    """Interop, reverse direction: tests/golden/amd_checkpoint.pth was written by
    rl_games_amd.A2CAgent.save() on an MI355X (tests/golden/make_amd_checkpoint.py).  The REAL
    reference agent restores it (`A2CBase.restore`, a2c_common.py:927-930) - weights, normaliser
    statistics, Adam state, counters - and trains on.  The recording names the checkpoint it was
    made from (SHA-256): a rewritten checkpoint needs a new recording."""
    src = os.path.join(HERE, 'golden', 'amd_checkpoint.pth')
    with open(src, 'rb') as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    ck = torch.load(src, map_location='cpu', weights_only=False)
    meta = ck.pop('_meta')

    def ref_side():
        from rl_games.torch_runner import Runner
        from rl_games_amd.synthetic_env import SyntheticTensorEnv
        path = str(tmp_path / 'amd_ckpt.pth')
        torch.save(ck, path)
        params = copy.deepcopy(meta['params'])
        params['config'].update(device='cpu', train_dir=str(tmp_path / 'runs'))
        env = SyntheticTensorEnv(meta['env']['num_envs'], meta['env']['obs_dim'], meta['env']['act_dim'],
                                 device='cpu', seed=meta['env']['seed'])
        runner = Runner()
        runner.load({'params': copy.deepcopy(params)})
        runner.params['config']['vec_env'] = env
        runner.params['config']['env_info'] = env.get_env_info()
        agent = runner.algo_factory.create(runner.algo_name, base_name='interop', params=runner.params)
        agent.restore(path)
        restored = _frozen({'checkpoint_sha256': sha, 'model': agent.model.state_dict(), 'epoch_num': agent.epoch_num,
                            'frame': agent.frame, 'last_mean_rewards': agent.last_mean_rewards,
                            'lr': agent.optimizer.param_groups[0]['lr'], 'optimizer_state': agent.optimizer.state_dict()['state']})
        agent.init_tensors()
        agent.obs = agent.env_reset()
        agent.epoch_num += 1
        res = agent.train_epoch()
        restored['train_epoch_finite'] = all(bool(torch.isfinite(x).all()) for x in res[4] + res[5])
        return restored
    ref = reference(ref_side)
    assert ref['checkpoint_sha256'] == sha, 'tests/golden/amd_checkpoint.pth changed since the recording'
    sd = ref['model']
    assert list(sd.keys()) == list(ck['model'].keys())
    for k, v in ck['model'].items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k
    assert ref['epoch_num'] == ck['epoch'] == 2 and ref['frame'] == ck['frame']
    assert ref['last_mean_rewards'] == ck['last_mean_rewards'] == -3.5
    # (the reference restores the optimiser's lr but keeps `last_lr` at the config value)
    assert ref['lr'] == ck['optimizer']['param_groups'][0]['lr']
    for i, st in ck['optimizer']['state'].items():
        assert torch.equal(ref['optimizer_state'][i]['exp_avg'], st['exp_avg']), i
        assert float(ref['optimizer_state'][i]['step']) == float(st['step'])
    assert ref['train_epoch_finite']


def test_schedulers_equal_reference_trajectories(reference):
    """lr_control (pure-function form) vs rl_games/common/schedulers.py: identical python-float
    trajectories for the KL-band rule and the linear ramp (incl. the entropy ramp)."""
    import random
    from rl_games_amd import lr_control as M
    rnd = random.Random(0)
    kls = [rnd.choice([0.001, 0.003, 0.004, 0.005, 0.01, 0.016, 0.02, 0.05, rnd.random() * 0.03]) for _ in range(5000)]
    epochs = range(0, 1300, 7)

    def ref_side():
        from rl_games.common import schedulers as R
        a = R.AdaptiveScheduler(0.008, 1e-6, 1e-2, 1.5)
        lr1, adaptive = 3e-4, []
        for kl in kls:
            lr1, e1 = a.update(lr1, 0.01, 0, 0, kl)
            adaptive.append((lr1, e1))
        linear = {}
        for use_epochs in (True, False):
            l1 = R.LinearScheduler(3e-4, 1e-6, 1000, use_epochs, True, start_entropy_coef=0.01)
            linear[use_epochs] = [l1.update(0, 0.01, e, e * 3, 0) for e in epochs]
        return {'adaptive': adaptive, 'linear': linear, 'identity': R.IdentityScheduler().update(1e-3, 0.5, 3, 4, 0.1)}
    ref = reference(ref_side)
    b = M.AdaptiveScheduler(0.008, 1e-6, 1e-2, 1.5)
    lr2 = 3e-4
    for kl, (lr1, e1) in zip(kls, ref['adaptive']):
        lr2, e2 = b.update(lr2, 0.01, 0, 0, kl)
        assert lr1 == lr2 and e1 == e2
    assert b.device_rule() == dict(kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5)
    for use_epochs in (True, False):
        l2 = M.LinearScheduler(3e-4, 1e-6, 1000, use_epochs, True, start_entropy_coef=0.01)
        for e, want in zip(epochs, ref['linear'][use_epochs]):
            assert want == l2.update(0, 0.01, e, e * 3, 0)
    assert M.IdentityScheduler().update(1e-3, 0.5, 3, 4, 0.1) == ref['identity']


@pytest.mark.parametrize('heads,with_masks', [([5], False), ([5], True), ([3, 4, 2], False), ([3, 4, 2], True)])
def test_discrete_models_equal_reference_models(heads, with_masks, reference):
    """policy.DiscreteA2CModel vs the reference's ModelA2C / ModelA2CMultiDiscrete (models.py:66-206)
    built by the reference's own ModelBuilder from the same params, same weights: training-mode
    outputs (neglogp, entropy, values, normalised logits) are bit-identical, with and without
    CategoricalMasked action masks."""
    from rl_games_amd import configs
    from rl_games_amd.policy import PolicyBuilder
    multi = len(heads) > 1
    params = configs.cartpole_discrete()
    if multi:
        params['network']['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
    build_cfg = {'actions_num': heads if multi else heads[0], 'input_shape': (6,), 'num_seqs': 4, 'value_size': 1,
                 'normalize_value': False, 'normalize_input': False}
    g = gen(sum(heads))
    B, n = 64, sum(heads)
    obs = torch.randn(B, 6, generator=g)
    masks = None
    if with_masks:
        masks = torch.rand(B, n, generator=g) > 0.4
        o = 0
        for s in heads:
            masks[torch.arange(B), o + torch.randint(0, s, (B,), generator=g)] = True
            o += s
    acts = []
    o = 0
    for s in heads:
        w = torch.ones(B, s) if masks is None else masks[:, o:o + s].float()
        acts.append(torch.multinomial(w, 1, generator=g))
        o += s
    prev = torch.cat(acts, 1) if multi else acts[0].squeeze(1)

    def ref_side():
        from rl_games.algos_torch import model_builder
        ref_net = model_builder.ModelBuilder().load(copy.deepcopy(params))
        ref = ref_net.build(copy.deepcopy(build_cfg))
        state_dict = _frozen(ref.state_dict())
        out = ref({'is_train': True, 'obs': obs.clone(), 'prev_actions': prev, 'action_masks': masks})
        return {'state_dict': state_dict, 'out': {k: out[k] for k in ('prev_neglogp', 'entropy', 'values', 'logits')}}
    ref = reference(ref_side)
    mine = PolicyBuilder(copy.deepcopy(params)).build(copy.deepcopy(build_cfg))
    assert list(mine.state_dict().keys()) == list(ref['state_dict'].keys())
    mine.load_state_dict(ref['state_dict'])
    a = ref['out']
    b = mine({'is_train': True, 'obs': obs.clone(), 'prev_actions': prev, 'action_masks': masks})
    assert torch.equal(a['prev_neglogp'], b['prev_neglogp'])
    assert torch.equal(a['entropy'], b['entropy'])
    assert torch.equal(a['values'], b['values'])
    la = a['logits'] if multi else [a['logits']]
    lb = b['logits'] if multi else [b['logits']]
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    # and the oracle's categorical loss consumes the same quantities
    lg, vals = mine.forward_heads({'obs': obs})
    batch = {'actions': prev, 'old_logp_actions': a['prev_neglogp'].detach() + 0.1, 'advantages': torch.randn(B, generator=g),
             'old_values': torch.randn(B, 1, generator=g), 'returns': torch.randn(B, 1, generator=g)}
    out = O.categorical_loss_and_grads(lg, vals, batch, dict(e_clip=0.2, clip_value=True, critic_coef=1.0, entropy_coef=0.01),
                                       None, heads, masks)
    assert torch.equal(out['neglogp'], a['prev_neglogp'].detach())
    assert torch.allclose(out['entropy'], a['entropy'].mean().detach(), rtol=1e-6)


@pytest.mark.parametrize('kind', ['mlp', 'lstm', 'central_value'])
def test_continuous_and_recurrent_and_central_models_equal_reference(kind, reference):
    """policy.ContinuousA2CLogStdModel (MLP and LSTM with done resets) and CentralValueModel vs the
    reference's ModelBuilder-built networks from the same params and weights (training-mode forward;
    normalisers off - they are HIP kernels on our side and are tested on the GPU)."""
    from rl_games_amd import configs
    from rl_games_amd.policy import PolicyBuilder
    g = gen(11)
    if kind == 'central_value':
        params = {'model': {'name': 'central_value'},
                  'network': {'name': 'actor_critic', 'central_value': True,
                              'mlp': {'units': [24, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}}
        cfg = {'actions_num': 3, 'input_shape': (9,), 'num_seqs': 4, 'value_size': 1, 'normalize_value': False,
               'normalize_input': False, 'num_agents': 1}
    else:
        params = configs.pendulum_lstm_4096() if kind == 'lstm' else configs.tiny()
        params = {k: params[k] for k in ('model', 'network')}
        if kind == 'lstm':
            params['network']['rnn'] = {'name': 'lstm', 'units': 16, 'layers': 1}
        cfg = {'actions_num': 3, 'input_shape': (9,), 'num_seqs': 8, 'value_size': 1, 'normalize_value': False,
               'normalize_input': False}
    T, S = 4, 8
    B = T * S
    obs = torch.randn(B, 9, generator=g)
    if kind == 'central_value':
        batch = {'is_train': True, 'obs': obs}
        keys = ('values',)
    else:
        batch = {'is_train': True, 'obs': obs, 'prev_actions': torch.randn(B, 3, generator=g)}
        keys = ('prev_neglogp', 'values', 'entropy', 'mus', 'sigmas')
    if kind == 'lstm':
        batch['rnn_states'] = [0.3 * torch.randn(1, S, 16, generator=g) for _ in range(2)]
        batch['seq_length'] = T
        batch['dones'] = (torch.rand(B, generator=g) < 0.3).to(torch.uint8)

    def ref_side():
        from rl_games.algos_torch import model_builder
        ref = model_builder.ModelBuilder().load(copy.deepcopy(params)).build(copy.deepcopy(cfg))
        state_dict = _frozen(ref.state_dict())
        out = ref({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
        return {'state_dict': state_dict, 'out': {k: out[k] for k in keys}}
    ref = reference(ref_side)
    mine = PolicyBuilder(copy.deepcopy(params)).build(copy.deepcopy(cfg))
    assert sorted(mine.state_dict().keys()) == sorted(ref['state_dict'].keys())
    mine.load_state_dict(ref['state_dict'])
    a = ref['out']
    b = mine({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
    if kind == 'central_value':
        assert torch.equal(a['values'], b['values'])
        return
    tol = dict(rtol=1e-5, atol=1e-6) if kind == 'lstm' else dict(rtol=0, atol=0)   # per-step vs segment LSTM calls
    for k in keys:
        assert torch.allclose(a[k], b[k], **tol), k


def test_reference_runner_plugin_seam_constructs_our_agents(reference):
    """the REAL reference Runner with our agents registered in its
    algo_factory (torch_runner.py:117-120) loads an unmodified params dict and calls our
    constructors with (base_name, params) (:258).  Without a GPU the constructors stop at the
    device check - after parsing the reference-format params - which is what this container can
    verify; the GPU tests cover everything behind it.  The recording holds what the Runner handed
    to the registered builder (algo name, keyword arguments, the params it loaded - objects of the
    reference's own classes by class name); the call is repeated on those arguments, with this
    package's no-op observer in place of the reference's."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent, NullObserver
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    from rl_games_amd.synthetic_env import SyntheticTensorEnv
    cases = ((configs.tiny(device='cpu'), A2CAgent, dict(obs_dim=12, act_dim=3)),
             (configs.cartpole_discrete(device='cpu'), DiscreteA2CAgent, dict(obs_dim=4, discrete_actions=2)))

    def env_for(params, env_kw):
        return SyntheticTensorEnv(params['config']['num_actors'], device='cpu', **env_kw)

    def plain(x):
        """Containers and python scalars as they are, any other object as ('<object>', its class)."""
        if isinstance(x, dict):
            return {k: plain(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(plain(v) for v in x)
        if x is None or isinstance(x, (bool, int, float, str)):
            return x
        return ('<object>', f'{type(x).__module__}.{type(x).__qualname__}')

    def ref_side():
        from rl_games.torch_runner import Runner
        seen = []
        for params, cls, env_kw in cases:
            calls = []

            def builder(agent_cls):
                def make(**kw):
                    config = {k: v for k, v in kw['params']['config'].items() if k not in ('vec_env', 'env_info')}
                    calls.append({'kwargs': sorted(kw), 'base_name': kw['base_name'],
                                  'params': plain(dict(kw['params'], config=config))})
                    return agent_cls(**kw)
                return make
            runner = Runner()
            runner.algo_factory.register_builder('a2c_continuous', builder(A2CAgent))
            runner.algo_factory.register_builder('a2c_discrete', builder(DiscreteA2CAgent))
            runner.load({'params': copy.deepcopy(params)})
            env = env_for(params, env_kw)
            runner.params['config']['vec_env'] = env
            runner.params['config']['env_info'] = env.get_env_info()
            with pytest.raises(RuntimeError, match='MI355X HIP device only'):
                runner.algo_factory.create(runner.algo_name, base_name='run', params=runner.params)
            assert len(calls) == 1
            seen.append(dict(calls[0], algo_name=runner.algo_name))
        return seen
    ref = reference(ref_side)
    builders = {'a2c_continuous': A2CAgent, 'a2c_discrete': DiscreteA2CAgent}
    for (params, cls, env_kw), call in zip(cases, ref):
        assert builders[call['algo_name']] is cls and call['kwargs'] == ['base_name', 'params']
        loaded = call['params']
        features = loaded['config'].get('features') or {}
        if 'observer' in features:
            assert features['observer'] == ('<object>', 'rl_games.common.algo_observer.DefaultAlgoObserver')
            features['observer'] = NullObserver()
        env = env_for(params, env_kw)
        loaded['config']['vec_env'] = env
        loaded['config']['env_info'] = env.get_env_info()
        with pytest.raises(RuntimeError, match='MI355X HIP device only'):
            cls(base_name=call['base_name'], params=loaded)


# ----------------------------------------------------------------------------- value_size > 1 torch forms (round 5)

@pytest.mark.parametrize('V,masked,smooth,bound', [(1, False, False, 'bound'), (2, False, False, 'bound'), (3, True, False, 'regularisation'),
                                                   (2, True, True, 'bound'), (2, False, True, None),
                                                   (1, True, 2, 'bound'), (2, False, 2, None),
                                                   (1, False, False, 'bound-rowsigma'), (2, True, True, 'regularisation-rowsigma')])
def test_torch_fallback_losses_equal_the_reference_agent_functions(V, masked, smooth, bound, reference):
    """rl_games_amd/torch_fallback.py (the value_size > 1 path of the agent) against the reference's OWN calc_losses
    (a2c_continuous.py:97-134, called unbound on a stand-in with exactly the attributes it reads), its model epilogue
    (models.py:329-364) and policy_kl - loss, the four scalars, KL, and the gradients w.r.t. mu / logstd / values."""
    from rl_games_amd import torch_fallback as tf
    g = gen(3 + V)
    mb, A = 512, 5
    # ('-rowsigma': a state-dependent sigma head, fixed_sigma False - log sigma per row [mb, A]; round 6)
    row_sigma = bound is not None and bound.endswith('-rowsigma')
    if row_sigma:
        bound = bound[:-len('-rowsigma')]
    mu0 = 1.3 * torch.randn(mb, A, generator=g)
    logstd0 = 0.2 * torch.randn(*((mb, A) if row_sigma else (A,)), generator=g)
    values0 = torch.randn(mb, V, generator=g)
    actions = mu0 + torch.randn(mb, A, generator=g)
    old_nlp = 0.5 * torch.randn(mb, generator=g) + 6.0
    adv = torch.randn(mb, generator=g)
    old_values = values0 + 0.3 * torch.randn(mb, V, generator=g)
    returns = torch.randn(mb, V, generator=g)
    old_mu = mu0 + 0.1 * torch.randn(mb, A, generator=g)
    old_sigma = torch.exp(0.2 * torch.randn(mb, A, generator=g))
    mask = (torch.rand(mb, generator=g) < 0.7).float() if masked else None
    coef_b = None if bound is None else 1e-3
    kind = {None: 0, 'bound': 1, 'regularisation': 2}[bound]

    def leaves():
        return [t.clone().requires_grad_(True) for t in (mu0, logstd0, values0)]
    # ---- ours
    mu, logstd, values = leaves()
    loss, sc, sigma = tf.ppo_loss(mu, logstd, values, actions, old_nlp, adv, old_values, returns, e_clip=0.2, critic_coef=2.0,
                                  entropy_coef=0.01, bounds_coef=coef_b if coef_b is not None else 0.0, bound_kind=kind,
                                  clip_value=True, smooth=smooth, mask=mask)
    loss.backward()
    ours = (loss.detach(), sc, [t.grad.clone() for t in (mu, logstd, values)])
    kl = tf.policy_kl(mu.detach(), sigma.detach().expand_as(mu), old_mu, old_sigma, mask)

    # ---- the reference: epilogue as ModelA2CContinuousLogStd.Network.forward computes it, then calc_losses
    def ref_side():
        import types
        from rl_games.algos_torch import a2c_continuous, torch_ext
        from rl_games.algos_torch.models import ModelA2CContinuousLogStd
        from rl_games.common import common_losses
        mu, logstd, values = leaves()
        logstd_full = mu * 0.0 + logstd                                                    # network_builder.py:506-512
        sigma_full = torch.exp(logstd_full)
        distr = torch.distributions.Normal(mu, sigma_full, validate_args=False)
        entropy = distr.entropy().sum(dim=-1)
        nlp = torch.squeeze(ModelA2CContinuousLogStd.Network.neglogp(None, actions, mu, sigma_full, logstd_full))
        # (smooth == 2: `ppo: False`, the plain A2C actor loss - round 6)
        stub = types.SimpleNamespace(ppo=(smooth != 2), has_value_loss=True, model=None, clip_value=True,
                                     bound_loss_type=bound, bounds_loss_coef=coef_b, critic_coef=2.0, entropy_coef=0.01,
                                     ppo_device='cpu')
        stub.bound_loss = types.MethodType(a2c_continuous.A2CAgent.bound_loss, stub)
        stub.reg_loss = types.MethodType(a2c_continuous.A2CAgent.reg_loss, stub)
        stub.bounds_loss_coef = coef_b
        fn = common_losses.smoothed_actor_loss if smooth == 1 else common_losses.actor_loss
        ref_loss, a, c, e, b, _ = a2c_continuous.A2CAgent.calc_losses(stub, fn, old_nlp, nlp, adv, 0.2, old_values, values,
                                                                   returns, mu, entropy, mask)
        ref_loss.backward()
        ref_kl = torch_ext.policy_kl(mu.detach(), sigma_full.detach(), old_mu, old_sigma, mask is None)
        if mask is not None:
            ref_kl = (ref_kl * mask).sum() / mask.sum()                                     # a2c_continuous.py:218-221
        return {'losses': (ref_loss, a, c, e, b), 'grads': [leaf.grad for leaf in (mu, logstd, values)], 'kl': ref_kl}
    ref = reference(ref_side)
    ref_loss, a, c, e, b = ref['losses']
    for got, want in ((ours[0], ref_loss.detach()), (ours[1]['a_loss'], a), (ours[1]['c_loss'], c), (ours[1]['entropy'], e),
                      (ours[1]['b_loss'], b.reshape(()) if bound is None else b)):
        assert torch.allclose(got, want.detach(), rtol=1e-6, atol=1e-7), (got, want)
    for got, want in zip(ours[2], ref['grads']):
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-8)
    assert torch.allclose(kl, ref['kl'], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('masked', [False, True])
def test_torch_fallback_advantage_normalisation_and_ema_equal_the_reference(masked, reference):
    from rl_games_amd import torch_fallback as tf
    from rl_games_amd.normalizers import GeneralizedMovingStats
    g = gen(11)
    adv = 3 * torch.randn(4096, generator=g) + 0.5
    mask = (torch.rand(4096, generator=g) < 0.6).float() if masked else None
    xs = [(k + 1) * torch.randn(4096, generator=g) - k for k in range(3)]

    def ref_side():
        from rl_games.algos_torch import torch_ext
        from rl_games.algos_torch.moving_mean_std import GeneralizedMovingStats as RefStats
        ref = RefStats((1,), decay=0.5)
        return {'normalized': torch_ext.normalization_with_masks(adv, mask), 'ema': [ref(x, mask=mask) for x in xs],
                **{name: getattr(ref, name) for name in ('mean', 'sqrs', 'step')}}
    ref = reference(ref_side)
    assert torch.allclose(tf.normalize_advantages(adv, mask), ref['normalized'], rtol=1e-6, atol=1e-7)
    ours = GeneralizedMovingStats((1,), decay=0.5)
    for x, want in zip(xs, ref['ema']):
        assert torch.allclose(ours(x, mask=mask), want, rtol=1e-6, atol=1e-7)
    for name in ('mean', 'sqrs', 'step'):
        assert torch.equal(getattr(ours, name), ref[name])
    # nothing valid: no update
    before = (ours.mean.clone(), ours.step.clone())
    ours(adv, mask=torch.zeros(4096))
    assert torch.equal(ours.mean, before[0]) and torch.equal(ours.step, before[1])


def test_state_dependent_sigma_network_equals_the_reference_builder(reference):
    """fixed_sigma False (network_builder.py:341-344, :508-511, init_state_dependent_sigma_head :14-25): the policy module
    builds the same parameters as the reference's A2CBuilder network - names, shapes, the constant-initialiser rule (bias =
    val, weights zero) - and, on the reference's weights, returns the same (mu, log sigma, value) and the same model outputs
    (neglogp, entropy) bit for bit."""
    from rl_games_amd.policy import ActorCriticNetwork, ContinuousA2CLogStdModel
    net_params = {'name': 'actor_critic', 'separate': False,
                  'space': {'continuous': {'mu_activation': 'None', 'sigma_activation': 'None',
                                           'mu_init': {'name': 'default'}, 'sigma_init': {'name': 'const_initializer', 'val': -0.7},
                                           'fixed_sigma': False}},
                  'mlp': {'units': [32, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}
    obs = torch.randn(8, 7, generator=gen(10))
    acts = torch.randn(8, 3, generator=gen(11))
    keys = ('prev_neglogp', 'values', 'entropy', 'mus', 'sigmas')

    def ref_side():
        from rl_games.algos_torch import network_builder
        from rl_games.algos_torch.models import ModelA2CContinuousLogStd
        builder = network_builder.A2CBuilder()
        builder.load(copy.deepcopy(net_params))
        torch.manual_seed(4)
        ref_net = builder.build('a2c', actions_num=3, input_shape=(7,), value_size=1, num_seqs=8)
        initial = copy.deepcopy(ref_net.state_dict())
        ref_sd = ref_net.state_dict()
        with torch.no_grad():
            for k, v in ref_sd.items():
                if k.startswith('sigma.'):
                    ref_sd[k] = v + 0.1 * torch.randn(v.shape, generator=gen(9))      # a sigma head that does depend on the state
        ref_net.load_state_dict(ref_sd)
        ref_sd = _frozen(ref_sd)
        want = ref_net({'obs': obs, 'rnn_states': None})
        # the model epilogue around it (models.py:329-364)
        ref_model = ModelA2CContinuousLogStd.Network(ref_net, obs_shape=(7,), normalize_value=False, normalize_input=False,
                                                     value_size=1)
        a = ref_model({'is_train': True, 'prev_actions': acts, 'obs': obs, 'rnn_states': None})
        return {'initial': initial, 'state_dict': ref_sd, 'heads': want[:3], 'model': {k: a[k] for k in keys}}
    ref = reference(ref_side)
    ours = ActorCriticNetwork(copy.deepcopy(net_params), actions_num=3, input_shape=(7,), value_size=1, num_seqs=8)
    ref_sd, our_sd = ref['initial'], ours.state_dict()
    assert {k: tuple(v.shape) for k, v in ref_sd.items()} == {k: tuple(v.shape) for k, v in our_sd.items()}
    assert torch.equal(our_sd['sigma.bias'], torch.full((3,), -0.7)) and not our_sd['sigma.weight'].any()
    assert torch.equal(ref_sd['sigma.bias'], our_sd['sigma.bias']) and torch.equal(ref_sd['sigma.weight'], our_sd['sigma.weight'])
    ours.load_state_dict(ref['state_dict'])
    got = ours({'obs': obs, 'rnn_states': None})
    for w, g_ in zip(ref['heads'], got[:3]):
        assert torch.equal(w, g_)
    assert got[1].shape == (8, 3) and (got[1][0] != got[1][1]).any()
    # the model epilogue around it (models.py:329-364)
    our_model = ContinuousA2CLogStdModel(ours, (7,), False, False, 1)
    b = our_model({'is_train': True, 'prev_actions': acts, 'obs': obs, 'rnn_states': None})
    for key in keys:
        assert torch.equal(ref['model'][key], b[key]), key
    mu, logstd, value, _ = our_model.forward_heads({'obs': obs})
    assert torch.equal(logstd, got[1]) and torch.equal(mu, got[0])


@pytest.mark.parametrize('space', [{'sigma_parametrization': 'softplus', 'min_sigma': 0.05},
                                   {'sigma_parametrization': 'softplus'},
                                   {'sigma_parametrization': 'scalar'}, {'sigma_parametrization': 'linear', 'min_sigma': 0.2},
                                   {'logstd_bounds': [-1.0, 0.5]}, {'min_sigma': 0.1}, {'logstd_bounds': [-2.0, 0.0], 'min_sigma': 0.3},
                                   {}])
@pytest.mark.parametrize('fixed', [True, False])
def test_sigma_parametrisations_equal_the_reference_model(space, fixed, reference):
    """network_builder.py:311-322 + models.py:272-301 (`apply_sigma_parametrization`): the reference's model and this
    one on the same weights - sigmas, neglogp and entropy of a training call bit for bit; only the unbounded exp form is
    `plain_sigma` (what the fused kernels compute)."""
    from rl_games_amd.policy import ActorCriticNetwork, ContinuousA2CLogStdModel
    sp = copy.deepcopy(_SPACE)
    sp['continuous'].update(space, fixed_sigma=fixed, sigma_init={'name': 'const_initializer', 'val': 0.4})
    net_params = {'name': 'actor_critic', 'separate': False, 'space': sp,
                  'mlp': {'units': [32, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}
    kw = dict(actions_num=3, input_shape=(7,), value_size=1, num_seqs=4)
    obs = torch.randn(16, 7, generator=gen(4))
    acts = torch.randn(16, 3, generator=gen(5))
    keys = ('sigmas', 'mus', 'prev_neglogp', 'entropy', 'values')

    def ref_side():
        from rl_games.algos_torch import network_builder, models
        builder = network_builder.A2CBuilder()
        builder.load(copy.deepcopy(net_params))
        torch.manual_seed(5)
        ref = models.ModelA2CContinuousLogStd(builder).build(dict(kw, normalize_value=False, normalize_input=False))
        sd = ref.state_dict()
        with torch.no_grad():                                       # raw values on both sides of every bound / floor
            for k, v in sd.items():
                if 'sigma' in k:
                    sd[k] = v + 1.5 * torch.randn(v.shape, generator=gen(3))
        ref.load_state_dict(sd)
        sd = _frozen(sd)
        want = ref({'is_train': True, 'obs': obs.clone(), 'prev_actions': acts})
        return {'state_dict': sd, 'out': {k: want[k] for k in keys}}
    ref = reference(ref_side)
    ours_net = ActorCriticNetwork(copy.deepcopy(net_params), **kw)
    assert ours_net.plain_sigma == (space == {})
    ours = ContinuousA2CLogStdModel(ours_net, (7,), False, False, 1)
    ours.load_state_dict(ref['state_dict'])
    want = ref['out']
    got = ours({'is_train': True, 'obs': obs.clone(), 'prev_actions': acts})
    for k in keys:
        assert torch.equal(want[k].expand_as(got[k]), got[k]), k


_SPACE = {'continuous': {'mu_activation': 'None', 'sigma_activation': 'None', 'mu_init': {'name': 'default'},
                         'sigma_init': {'name': 'const_initializer', 'val': 0}, 'fixed_sigma': True}}


@pytest.mark.parametrize('name,over', [
    ('layer_norm', {'normalization': 'layer_norm'}),
    ('layer_norm_first_only', {'normalization': 'layer_norm', 'mlp': {'units': [24, 24], 'norm_only_first_layer': True}}),
    ('batch_norm', {'normalization': 'batch_norm'}),
    ('d2rl_batch_norm_first_only', {'mlp': {'d2rl': True, 'norm_only_first_layer': True}, 'normalization': 'batch_norm'}),
    ('d2rl', {'mlp': {'d2rl': True}}),
    ('d2rl_layer_norm', {'mlp': {'d2rl': True}, 'normalization': 'layer_norm'}),
    ('gru_two_layers', {'rnn': {'name': 'gru', 'units': 12, 'layers': 2}}),
    ('lstm_layer_norm_concat', {'rnn': {'name': 'lstm', 'units': 12, 'layers': 1, 'layer_norm': True, 'concat_input': True,
                                        'concat_output': True}}),
    ('lstm_before_mlp', {'rnn': {'name': 'lstm', 'units': 12, 'layers': 1, 'before_mlp': True, 'concat_output': True}}),
    ('discrete_d2rl_layer_norm', {'mlp': {'d2rl': True}, 'normalization': 'layer_norm', 'space': {'discrete': {}}}),
    ('separate_lstm_layer_norm', {'separate': True, 'rnn': {'name': 'lstm', 'units': 12, 'layers': 1, 'layer_norm': True}}),
    ('separate_gru_before_mlp', {'separate': True, 'rnn': {'name': 'gru', 'units': 12, 'layers': 2, 'before_mlp': True}}),
    ('discrete_separate_lstm_concat', {'separate': True, 'space': {'discrete': {}},
                                       'rnn': {'name': 'lstm', 'units': 12, 'layers': 1, 'concat_input': True}}),
    ('discrete_lstm', {'rnn': {'name': 'lstm', 'units': 12, 'layers': 1}, 'space': {'discrete': {}}}),
    ('discrete_gru_before_mlp_concat', {'rnn': {'name': 'gru', 'units': 12, 'layers': 1, 'before_mlp': True,
                                                'concat_output': True}, 'space': {'discrete': {}}}),
])
def test_network_zoo_layouts_equal_the_reference_builder(name, over, reference):
    """The network layouts that left the NotImplementedError list in round 6 - layer normalisation (network_builder.py:105-132),
    D2RL trunks (d2rl.py), GRU / multi-layer RNNs, an RNN in front of the MLP, concatenated RNN inputs / outputs, layer norm
    behind the RNN (:250-276, :447-487) - against the reference's own A2CBuilder network: the same parameter names and shapes,
    and on the reference's weights the same outputs (and next RNN states) bit for bit, with done resets inside a sequence."""
    from rl_games_amd.policy import ActorCriticNetwork
    net_params = {'name': 'actor_critic', 'separate': False, 'space': copy.deepcopy(_SPACE),
                  'mlp': {'units': [32, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}
    for k, v in over.items():
        if k == 'mlp':
            net_params['mlp'].update(v)
        else:
            net_params[k] = v
    discrete = 'discrete' in net_params['space']
    kw = dict(actions_num=3, input_shape=(7,), value_size=1, num_seqs=4)
    n_out = 2 if discrete else 3
    T, S = 3, 4                                                 # seq_length 3, 4 sequences
    obs = torch.randn(S * T, 7, generator=gen(4))
    d = {'obs': obs, 'rnn_states': None}
    n_states = 0
    if 'rnn' in net_params:
        layers, units = net_params['rnn']['layers'], net_params['rnn']['units']
        n_states = (2 if net_params['rnn']['name'] == 'lstm' else 1) * (2 if net_params['separate'] else 1)
        states = tuple(torch.randn(layers, S, units, generator=gen(6 + i)) for i in range(n_states))
        dones = (torch.rand(S * T, generator=gen(8)) < 0.3).float()
        d = {'obs': obs, 'rnn_states': states, 'seq_length': T, 'dones': dones}

    def ref_side():
        from rl_games.algos_torch import network_builder
        builder = network_builder.A2CBuilder()
        builder.load(copy.deepcopy(net_params))
        torch.manual_seed(5)
        ref_net = builder.build('a2c', **kw)
        ref_sd = ref_net.state_dict()
        shapes = {k: tuple(v.shape) for k, v in ref_sd.items()}
        with torch.no_grad():                                   # LayerNorm weights away from their (1, 0) initialisation
            for k, v in ref_sd.items():
                if 'norm' in k and v.is_floating_point():
                    ref_sd[k] = v + 0.2 * torch.randn(v.shape, generator=gen(3))
        ref_net.load_state_dict(ref_sd)
        rec = {'shapes': shapes, 'state_dict': _frozen(ref_sd)}
        rec['out'] = _frozen(ref_net(dict(d)))
        if 'rnn' in net_params:
            rec['n_default_states'] = len(ref_net.get_default_rnn_state())
        if 'batch_norm' in name:
            ref_net.eval()
            rec['eval_state_dict'] = _frozen(ref_net.state_dict())
            rec['eval_out'] = ref_net(dict(d))[:n_out]
        return rec
    ref = reference(ref_side)
    ours = ActorCriticNetwork(copy.deepcopy(net_params), **kw)
    assert ref['shapes'] == {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    assert not getattr(ours, 'plain_trunk', True) or name in ('gru_two_layers', 'discrete_lstm')
    ours.load_state_dict(ref['state_dict'])
    if 'rnn' in net_params:
        assert len(ours.get_default_rnn_state()) == ref['n_default_states'] == n_states
    want = ref['out']
    got = ours(dict(d))
    for w, g_ in zip(want[:n_out], got[:n_out]):
        assert torch.allclose(w, g_, rtol=0, atol=0) or torch.allclose(w, g_, rtol=1e-6, atol=1e-7), name
    if 'rnn' in net_params:
        assert len(want[n_out]) == len(got[n_out]) == n_states
        for w, g_ in zip(want[n_out], got[n_out]):
            assert torch.allclose(w, g_, rtol=1e-6, atol=1e-7)
    else:
        for w, g_ in zip(want[:n_out], got[:n_out]):
            assert torch.equal(w, g_), name
    if 'batch_norm' in name:                                    # that call was in training mode: batch statistics, running
        ours.eval()                                             # statistics updated; now the rollout's mode
        for (k, w), g_ in zip(ref['eval_state_dict'].items(), ours.state_dict().values()):
            assert torch.equal(w, g_), k
        for w, g_ in zip(ref['eval_out'], ours(dict(d))[:n_out]):
            assert torch.equal(w, g_), name
