"""GPU parity at the BENCHMARKED shapes (BASELINE.json configs[1] and configs[2]), through the same
code path bench.py times: 32,768-row minibatches on the fused MLP kernels, one HIP graph per
mini-epoch, dataset preparation at 65,536 x 32, and the rollout head fed with the reference's own
recorded rollout.

Oracle = oracle/ppo_epoch_oracle.OracleAgent (CPU restatement of a2c_common.py:1586-1660 /
a2c_continuous.py:136-234, pinned to the reference by tests/test_oracle_epoch.py and
tests/test_vs_reference_cpu.py) on the SAME rollout tensors.  Tolerances: rtol 1e-5 (north_star)
plus an absolute floor for scalars that are means of +-O(1) terms - a_loss of the first pass is
-mean(normalised advantages) ~ 5e-3 over 32,768 rows, where one fp32 ulp of the O(1) summands is
6e-8 and the summation order (GPU block tree vs ATen's) alone moves the mean by ~1e-7.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (the exact-products worker runs this file as a script)
from oracle import ppo_oracle as O
from oracle.ppo_epoch_oracle import OracleAgent
from rl_games_amd.synthetic_env import SyntheticTensorEnv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

RTOL = 1e-5
ATOL = {'a_loss': 2e-7, 'c_loss': 2e-7, 'entropy': 2e-6, 'b_loss': 1e-7, 'kl': 2e-7}


def _make_agent(cap, **over):
    from rl_games_amd.agent import A2CAgent
    params = copy.deepcopy(cap['params'])
    params['config'].update(device=DEV, **over)
    env = SyntheticTensorEnv(cap['env']['num_envs'], cap['env']['obs_dim'], cap['env']['act_dim'],
                             device=DEV, seed=cap['env']['seed'])
    params['config']['vec_env'] = env
    params['config']['env_info'] = env.get_env_info()
    agent = A2CAgent('test', params)
    agent.init_tensors()
    return agent


def _capture_rollout(agent):
    """Wraps play_steps: keeps a CPU copy of every rollout batch and the model state it was played with."""
    caps = []
    orig = agent.play_steps

    def play():
        b = orig()
        caps.append({'batch': {k: v.detach().cpu().clone() for k, v in b.items() if isinstance(v, torch.Tensor)},
                     'state': {k: v.detach().cpu().clone() for k, v in agent.model.state_dict().items()}})
        return b
    agent.play_steps = play
    return caps


def _check_epoch(res, ref, nmb, mini_epochs, bounds=True):
    a_losses, c_losses, b_losses, entropies, kls = res[4], res[5], res[6], res[7], res[8]
    assert len(a_losses) == len(ref) == nmb * mini_epochs
    got = {'a_loss': torch.stack(a_losses).cpu(), 'c_loss': torch.stack(c_losses).cpu(),
           'entropy': torch.stack(entropies).cpu()}
    if bounds:
        got['b_loss'] = torch.stack(b_losses).cpu()
    for key, g in got.items():
        want = torch.stack([r[key].reshape(()) for r in ref])
        assert torch.allclose(g, want, rtol=RTOL, atol=ATOL[key]), (key, (g - want).abs().max().item(), g[:4], want[:4])
    want_kl = torch.stack([r['kl'].reshape(()) for r in ref]).reshape(mini_epochs, nmb).mean(1)
    got_kl = torch.stack(kls).cpu()
    assert torch.allclose(got_kl, want_kl, rtol=1e-4, atol=ATOL['kl']), (got_kl, want_kl)


def _check_final_params(agent, oracle, steps, lr_max, truth=None):
    """Parameters after `steps` Adam steps.  Adam's first updates are +-lr * g/|g|-like, so an element
    whose gradient is at rounding-noise level (|g| ~ 1e-9: dead units, bound-loss-only paths) can move
    by lr in the opposite direction when its fp32 gradient differs in the last bits between the GPU's
    and the CPU's summation order.  Hence: (i) the bulk agrees to rtol 1e-4 / atol 2e-6, at most 0.2 % of
    a tensor's elements may deviate, and (ii) no element deviates by more than the total step budget.
    truth: a callable returning the fp64 trajectory's final parameters (the oracle evaluated in double precision on the same
    inputs, _truth_for).  An element outside (i) is then judged like the loss scalars are: it passes when the agent is no
    farther from the fp64 value than 1.5 x the fp32 oracle is - log sigma's gradient is a sum that nearly cancels at the
    start of training, the loss tile forms it in fp64 and the oracle in fp32 (config #2: |agent - fp64| 3e-10,
    |oracle - fp64| 1.1e-5 in one element, tools/exp/ant_sigma_probe.py)."""
    final, want = agent.model.state_dict(), oracle.model.full_state_dict()
    tru = None
    for name, v in want.items():
        got = final[name].cpu().to(v.dtype)
        if not v.is_floating_point():
            assert torch.equal(got, v), name
            continue
        bad = ~torch.isclose(got, v, rtol=1e-4, atol=2e-6)
        if bad.float().mean().item() > 2e-3 and truth is not None:
            if tru is None:
                tru = truth()
            t = tru[name].double()
            closer = (got.double() - t).abs() <= 1.5 * (v.double() - t).abs() + 1e-9
            bad = bad & ~closer
        assert bad.float().mean().item() <= 2e-3, (name, bad.float().mean().item())
        assert (got - v).abs().max().item() <= 2.1 * steps * lr_max, (name, (got - v).abs().max().item())


def _oracle_for(params, cap, N, obs_dim, act_dim):
    cpu_params = copy.deepcopy(params)
    cpu_params['config']['device'] = 'cpu'
    oracle = OracleAgent(cpu_params, SyntheticTensorEnv(N, obs_dim, act_dim, device='cpu', seed=1))
    oracle.model.load_full_state_dict(cap['state'])
    return oracle


def _truth_for(params, cap, N, obs_dim, act_dim):
    """The oracle evaluated in fp64: same operation sequence, same fp32 inputs (rollout tensors, initial parameters, the
    normalisers' fp32 constants), every intermediate, gradient and Adam moment in double precision - the exact-arithmetic
    trajectory of the algorithm, as far as an fp64 run can tell, that every fp32 implementation is an approximation of."""
    truth = _oracle_for(params, cap, N, obs_dim, act_dim)
    truth.model.a2c_network.double()
    truth.optimizer = torch.optim.Adam(truth.model.a2c_network.parameters(), truth.lr, eps=1e-08)
    return truth


def _batch64(batch):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in batch.items()}


@pytest.mark.parametrize('graphs', [True, False])
def test_full_size_minibatches_on_the_benchmarked_path_match_oracle(graphs):
    """BASELINE config #3 network and minibatch: 32,768 x 108 -> [400,200,100] -> (1 | 21), two
    minibatches x two mini-epochs.  graphs=True runs the update as the replayed mini-epoch HIP
    graph bench.py times (forced from the first epoch, so the fresh optimiser state matches a
    fresh oracle); graphs=False the eager launches."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    N, H = 2048, 32
    params = configs.humanoid_65536(num_actors=N, minibatch_size=32768, hip_graphs=graphs)
    params['config']['mini_epochs'] = 2
    torch.manual_seed(5)
    agent = A2CAgent('headline', copy.deepcopy(params))
    assert agent._engine is not None and agent._engine.chain is not None
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    if graphs:
        agent._eager_epochs = 1           # capture + replay already in the first epoch
    agent.update_epoch()
    res = agent.train_epoch()
    if graphs:
        assert agent._update_graphs.epoch is not None and not agent._graph_failed
    assert agent._engine.last_dw_path == 'mfma' and agent._engine.last_dw_library_jobs == 0
    oracle = _oracle_for(params, caps[0], N, 108, 21)
    ref = oracle.update(caps[0]['batch'])
    # dataset preparation at this batch (65,536 rows): normalised values / returns / advantages
    vd = agent.dataset.values_dict
    for key in ('old_values', 'returns', 'advantages'):
        assert torch.allclose(vd[key].cpu().reshape(-1), oracle.dataset[key].reshape(-1), rtol=RTOL, atol=2e-6), key
    _check_epoch(res, ref, nmb=2, mini_epochs=2)
    # device-side adaptive learning rate == the oracle's python-float schedule, bit for bit
    assert agent.optimizer.last_and_next_lr()[1] == oracle.lr
    _check_final_params(agent, oracle, steps=4, lr_max=max(oracle.lr, 3e-4))


@pytest.mark.parametrize('graphs', [True, False])
def test_config2_ant_epoch_matches_oracle(graphs):
    """BASELINE config #2 end to end: 4,096 envs x horizon 16, obs 60, act 8, MLP [256,128,64],
    minibatch 32,768 x 4 mini-epochs (8 optimiser steps) - rollout on the device, update vs the oracle."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    N, H = 4096, 16
    params = configs.ant_4096(hip_graphs=graphs)
    torch.manual_seed(9)
    agent = A2CAgent('ant', copy.deepcopy(params))
    assert agent._engine is not None and agent._engine.chain is not None
    assert (agent.horizon_length, agent.num_actors, agent.minibatch_size, agent.mini_epochs_num) == (16, 4096, 32768, 4)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    if graphs:
        agent._eager_epochs = 1
    agent.update_epoch()
    res = agent.train_epoch()
    oracle = _oracle_for(params, caps[0], N, 60, 8)
    batch = caps[0]['batch']
    # the rollout itself: the GAE of the recorded buffers reproduces the recorded returns bit for bit
    tb = agent.experience_buffer.tensor_dict
    ref = oracle.update(batch)
    vd = agent.dataset.values_dict
    for key in ('old_values', 'returns', 'advantages'):
        assert torch.allclose(vd[key].cpu().reshape(-1), oracle.dataset[key].reshape(-1), rtol=RTOL, atol=2e-6), key
    assert tb['rewards'].shape[:2] == (H, N)
    _check_epoch(res, ref, nmb=2, mini_epochs=4)
    assert agent.optimizer.last_and_next_lr()[1] == oracle.lr
    def fp64_final():
        truth = _truth_for(params, caps[0], N, 60, 8)
        truth.update(_batch64(batch))
        return truth.model.full_state_dict()
    _check_final_params(agent, oracle, steps=8, lr_max=max(oracle.lr, 3e-4), truth=fp64_final)


def test_dataset_preparation_and_obs_statistics_at_65536x32():
    """prepare_dataset (value RunningMeanStd update + normalisation, advantage normalisation) on the
    full 2,097,152-row batch and the observation RunningMeanStd update on a 32,768 x 108 minibatch,
    against the oracle's op-for-op restatement (running_mean_std.py:19-114, a2c_common.py:1586-1660)."""
    from rl_games_amd import ops
    from rl_games_amd.gae import gae_returns_advantages
    N, H = 65536, 32
    g = torch.Generator().manual_seed(3)
    r = torch.randn(N, H, generator=g)
    v = torch.randn(N, H, generator=g) * 2 + 0.5
    d = (torch.rand(N, H, generator=g) < 0.05).to(torch.uint8)
    lv = torch.randn(N, generator=g)
    ld = (torch.rand(N, generator=g) < 0.05).to(torch.uint8)
    ret, adv, partials = gae_returns_advantages(r.to(DEV), v.to(DEV), d.to(DEV), lv.to(DEV), ld.to(DEV), 0.99, 0.95)
    # oracle: time-major scan, then flatten env-major
    advs = O.gae_scan(r.t().unsqueeze(-1).contiguous(), v.t().unsqueeze(-1).contiguous(), d.t().float().contiguous(),
                      lv.unsqueeze(-1), ld.float(), 0.99, 0.95)
    ret_ref = O.flatten_env_major(advs + v.t().unsqueeze(-1))
    assert torch.equal(ret.reshape(-1, 1).cpu(), ret_ref)
    values_flat = v.reshape(-1, 1)
    state = O.new_running_stats(1)
    state['running_mean'].fill_(0.3)
    state['running_var'].fill_(1.7)
    state['count'] = torch.tensor(12345, dtype=torch.int64)
    dmean = state['running_mean'].clone().to(DEV)
    dvar = state['running_var'].clone().to(DEV)
    dcount = state['count'].clone().reshape(1).to(DEV)
    stats = ops.prepare_stats_buffer(DEV)
    B = N * H
    flags = ops.PREP_NORM_VALUE | ops.PREP_NORM_ADV
    ops.prepare_finalize(partials, B, flags, (dmean, dvar, dcount), 1e-5, None, stats)
    nv, nr, na = (torch.empty(B, device=DEV) for _ in range(3))
    ops.prepare_apply(v.reshape(-1).to(DEV), ret.reshape(-1), adv.reshape(-1), flags, stats, out=(nv, nr, na))
    # oracle op chain (a2c_common.py:1598-1634): values first, then returns through the UPDATED statistics
    want = O.prepare_dataset(ret_ref, values_flat, {k: t.clone() for k, t in state.items()})
    st = want['value_stats']
    assert dcount.item() == st['count'].item()
    assert torch.allclose(dmean.cpu(), st['running_mean'], rtol=1e-6, atol=1e-9)
    assert torch.allclose(dvar.cpu(), st['running_var'], rtol=2e-6, atol=1e-9)
    assert torch.allclose(nv.cpu(), want['old_values'].reshape(-1), rtol=RTOL, atol=2e-6)
    assert torch.allclose(nr.cpu(), want['returns'].reshape(-1), rtol=RTOL, atol=2e-6)
    assert torch.allclose(na.cpu(), want['advantages'].reshape(-1), rtol=RTOL, atol=2e-6)
    # observation statistics at the minibatch shape of the benchmark
    x = (torch.randn(32768, 108, generator=g) * 3 + 1)
    ost = O.new_running_stats(108)
    y_ref, ost2 = O.running_stats_forward(ost, x, training=True)
    om, ov, oc = ost['running_mean'].clone().to(DEV), ost['running_var'].clone().to(DEV), ost['count'].clone().reshape(1).to(DEV)
    part, nb = ops.column_moments(x.to(DEV))
    ops.rms_update(part, nb, 108, 32768, 0, om, ov, oc)
    assert torch.allclose(om.cpu(), ost2['running_mean'], rtol=1e-6, atol=1e-8)
    assert torch.allclose(ov.cpu(), ost2['running_var'], rtol=2e-6, atol=1e-9)
    y = ops.rms_apply(x.to(DEV), om, ov, 1e-5, 0)
    assert torch.allclose(y.cpu(), y_ref, rtol=RTOL, atol=2e-6)


def test_reference_rollout_through_the_fused_policy_head(golden):
    """The REAL reference's recorded rollout (tests/golden/epoch.pt: observations, sampled actions,
    mus, sigmas, neglogpacs, values of ModelA2CContinuousLogStd in eval mode, models.py:346-364) fed
    through the fused chain forward + rollout_policy_head kernel: same mus / values, and - with the
    reference's own noise (a - mu)/sigma - the same actions and neglogpacs."""
    from rl_games_amd import ops
    cap = golden('epoch.pt')['default']
    agent = _make_agent(cap)
    agent.model.load_state_dict(cap['init_state'])            # the state the reference played with
    agent.set_eval()
    N, H = cap['env']['num_envs'], cap['params']['config']['horizon_length']
    b = cap['batch']
    A = b['actions'].shape[1]
    obs = b['obses'].reshape(N, H, -1)
    eng = agent._engine
    assert eng is not None and eng.chain is not None
    vm = agent.model.value_mean_std
    buf = agent.experience_buffer
    for t in range(H):
        o = obs[:, t].contiguous().to(DEV)
        heads = eng.forward_obs(o, agent._obs_rms(), agent._obs_eps(), keep=False)
        mu_ref = b['mus'].reshape(N, H, A)[:, t]
        sg_ref = b['sigmas'].reshape(N, H, A)[:, t]
        act_ref = b['actions'].reshape(N, H, A)[:, t]
        noise = ((act_ref.double() - mu_ref.double()) / sg_ref.double()).float().to(DEV)
        actions, values = torch.empty(N, A, device=DEV), torch.empty(N, device=DEV)
        ops.rollout_policy_head(heads, agent.model.a2c_network.sigma.data, noise, (vm.running_mean, vm.running_var),
                                vm.epsilon, actions, values, buf.storage, H, t)
    tb = buf.tensor_dict
    flat = lambda x: x.transpose(0, 1).reshape((N * H,) + tuple(x.shape[2:]))
    assert torch.allclose(flat(tb['mus']).cpu(), b['mus'], rtol=1e-5, atol=1e-6)
    assert torch.allclose(flat(tb['sigmas']).cpu(), b['sigmas'], rtol=1e-6, atol=0)
    assert torch.allclose(flat(tb['actions']).cpu(), b['actions'], rtol=1e-5, atol=2e-6)
    assert torch.allclose(flat(tb['neglogpacs']).cpu().reshape(-1), b['neglogpacs'].reshape(-1), rtol=1e-5, atol=1e-5)
    assert torch.allclose(flat(tb['values']).cpu().reshape(-1, 1), b['values'].reshape(-1, 1), rtol=1e-5, atol=2e-6)


# ----------------------------------------------------------------------------- round 3: the benchmarked job itself

def _oracle_threads():
    """The oracle's CPU GEMMs at a sane thread count: with all 256 threads of a GPU-box host the same
    epoch is orders of magnitude slower (bench.py's cpu_baseline notes)."""
    import os
    return max(1, min(16, os.cpu_count() or 1))


def _kl_fp64(mu, sigma, old_mu, old_sigma):
    """policy_kl (rl_games/algos_torch/torch_ext.py:27-36) evaluated in fp64 from fp32 inputs."""
    p0_mu, p0_s, p1_mu, p1_s = (t.double() for t in (mu, sigma, old_mu, old_sigma))
    c1 = torch.log(p1_s / p0_s + 1e-5)
    c2 = (p0_s ** 2 + (p1_mu - p0_mu) ** 2) / (2.0 * (p1_s ** 2 + 1e-5))
    return (c1 + c2 - 0.5).sum(dim=-1).mean()


def _epoch_deviation_rows(N, MB):
    """One epoch of the 320-step job: the agent's per-step scalars, the oracle's on the same rollout, the captured rollout."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    params = configs.humanoid_65536(num_actors=N, minibatch_size=MB, hip_graphs=True)
    torch.manual_seed(5)
    agent = A2CAgent('epoch', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    agent._eager_epochs = 1
    agent.update_epoch()
    res = agent.train_epoch()
    return params, agent, caps, res


def _deviation_per_mini_epoch(rows, ref, NMB, ME):
    cols = {'a_loss': 0, 'c_loss': 1, 'entropy': 2, 'b_loss': 3, 'kl': 4}
    out = {}
    for key, col in cols.items():
        want = torch.stack([r[key].reshape(()).float() for r in ref])
        d = (rows[:ME * NMB, col] - want).abs().reshape(ME, NMB).max(1).values
        out[key] = [float(x) for x in d]
    return out


TRUTH_FACTOR = 1.5      # the agent may be this much farther from the fp64 trajectory than the reference's own fp32 arithmetic
CEILING = 1e-3           # ... and never farther than this fraction of a scalar's scale, whatever the yardstick says


def _scalar_rows(results, dtype=torch.float64):
    return torch.stack([torch.stack([r[k].reshape(()).to(dtype) for k in COLS]) for r in results])


COLS = {'a_loss': 0, 'c_loss': 1, 'entropy': 2, 'b_loss': 3, 'kl': 4}


def _check_against_truth(rows, ref, tru, groups, what):
    """The criterion of the kernel-level tests (tests/test_ops_gpu.py: fp64 truth, the kernel as accurate as the fp32
    reference) at agent level.  rows / ref / tru: [steps, 5] scalars of the agent, of the oracle (the reference's fp32
    arithmetic) and of the oracle evaluated in fp64 on the same rollout; `groups`: consecutive step ranges (mini-epochs,
    epochs).  Within every group and for every scalar the agent must EITHER agree with the oracle at rtol 1e-5 (+ the
    stated floor) OR be no farther from the fp64 trajectory than TRUTH_FACTOR x the oracle itself is (running maxima
    over the groups so far) - and in no case farther than CEILING of the scalar's scale.  Nothing in the bound comes
    from the product, from noise models or from seeds."""
    report, env_a, env_o = [], {k: 0.0 for k in COLS}, {k: 0.0 for k in COLS}
    for g, sl in enumerate(groups):
        for key, c in COLS.items():
            a, o, t = rows[sl, c].double(), ref[sl, c].double(), tru[sl, c].double()
            scale = float(ref[:, c].abs().max())
            strict = bool(((a - o).abs() <= (1e-4 if key == 'kl' else RTOL) * o.abs() + ATOL[key]).all())
            env_a[key] = max(env_a[key], float((a - t).abs().max()))
            env_o[key] = max(env_o[key], float((o - t).abs().max()))
            report.append((g + 1, key, float((a - o).abs().max()), env_a[key], env_o[key], strict))
            assert strict or env_a[key] <= TRUTH_FACTOR * env_o[key] + ATOL[key], (what, report[-1])
            assert env_a[key] <= CEILING * scale + ATOL[key], (what, 'ceiling', report[-1])
    return report


@pytest.mark.parametrize('N,MB', [(8192, 4096), (65536, 32768)], ids=['rank_8192x32_mb4096', 'benchmarked_65536x32_mb32768'])
def test_whole_epoch_of_320_steps_matches_oracle(N, MB):
    """ALL 320 optimiser steps of one epoch against the oracle (OracleAgent = CPU restatement of
    a2c_continuous.py:136-234 / a2c_common.py:1517-1584, pinned to the real reference), every step a node of the
    replayed mini-epoch HIP graph:
      * 65,536 envs x 32, minibatch 32,768 - BASELINE.json configs[2] EXACTLY as bench.py times it (split-bf16 chain
        kernels, weight planes written by the Adam launch);
      * 8,192 envs x 32, minibatch 4,096 - what ONE of 8 data-parallel ranks runs for configs[3] (the lean 16-row
        exact-product chain kernels).
    First mini-epoch: the 64 per-minibatch (a_loss, c_loss, entropy, b_loss) at rtol 1e-5 (+ the stated floors), KL at
    1e-4 (test_kl_conditioning_fp64_demonstration), the learning-rate trajectory step for step.
    Mini-epochs 2 - 5 (round 6): against the FP64 TRAJECTORY.  The clipped objective has kinks; among 4,096 .. 32,768
    rows there is nearly always one within ~1e-6 of a clip boundary, two fp32 evaluations of a row's ratio differ by
    ~1e-6, so now and then one implementation clips a row the other does not and every later step inherits that step's
    difference (test_three_epochs_...).  Which of the two then left the algorithm's trajectory?  The oracle is run a
    second time in double precision on the same rollout (_truth_for) and both fp32 runs are measured against it
    (profiles/r6_truth_probe.txt): at the rank's shape the agent ends the fifth mini-epoch 1.0e-6 from the fp64 a_loss
    and the ORACLE 9.5e-6 - the 9.8e-6 between agent and oracle that rounds 4 - 5 built tolerance schedules and noise
    twins for is the reference's own fp32 arithmetic leaving the trajectory, not the kernels; at the benchmarked shape
    both are ~2e-5 away, the agent the closer of the two.  _check_against_truth: per mini-epoch and scalar the agent
    agrees with the oracle at rtol 1e-5, or is at most 1.5 x as far from the fp64 run as the oracle is, and never
    farther than 1e-3 of the scalar's scale.  No twins, no product-derived yardstick, no seed search.
    The learning rates of all 320 steps must agree with the oracle's unless a KL of the oracle lies within 1e-3 of a
    threshold of the rule.  End of epoch: every parameter tensor, on average, within max(1e-4 of its scale, 1.5 x the
    oracle's own distance from the fp64 parameters, 2e-5 absolute = lr / 15) of the fp64 parameters."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    H, NMB, ME = 32, 64, 5
    params = configs.humanoid_65536(num_actors=N, minibatch_size=MB, hip_graphs=True)
    torch.manual_seed(5)
    agent = A2CAgent('epoch', copy.deepcopy(params))
    assert (agent.num_actors, agent.horizon_length, agent.minibatch_size, agent.mini_epochs_num) == (N, H, MB, ME)
    assert agent._engine is not None and agent._engine.chain is not None
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    agent._eager_epochs = 1               # capture + replay already in the first epoch, like bench.py's timed epochs
    agent.update_epoch()
    res = agent.train_epoch()
    assert agent._update_graphs.epoch is not None and not agent._graph_failed
    assert agent._engine.last_dw_path == 'mfma' and agent._engine.last_dw_library_jobs == 0
    rows = agent._mb_scalars[:ME * NMB, :5].cpu()      # [a_loss, c_loss, entropy, b_loss, kl] per optimiser step
    assert len(res[4]) == ME * NMB

    prev = torch.get_num_threads()
    torch.set_num_threads(_oracle_threads())
    try:
        oracle = _oracle_for(params, caps[0], N, 108, 21)
        batch = caps[0]['batch']
        ref = oracle.update(batch)
        vd = agent.dataset.values_dict
        for key in ('old_values', 'returns', 'advantages'):
            assert torch.allclose(vd[key].cpu().reshape(-1), oracle.dataset[key].reshape(-1), rtol=RTOL, atol=2e-6), key
        truth = _truth_for(params, caps[0], N, 108, 21)
        tru = truth.update(_batch64(batch))
    finally:
        torch.set_num_threads(prev)
    stack = lambda rs, key, sl: torch.stack([r[key].reshape(()).float() for r in rs[sl]])
    # ---- first mini-epoch: the strict bounds
    first = slice(0, NMB)
    for key in ('a_loss', 'c_loss', 'entropy', 'b_loss'):
        want, got = stack(ref, key, first), rows[first, COLS[key]]
        assert torch.allclose(got, want, rtol=RTOL, atol=ATOL[key]), (key, (got - want).abs().max().item(), got[:3], want[:3])
    want_kl = stack(ref, 'kl', first)
    assert torch.allclose(rows[first, 4], want_kl, rtol=1e-4, atol=ATOL['kl']), (rows[:4, 4], want_kl[:4])
    # ---- learning rates: the device-side rule over the agent's own 320 KL values == python-float AdaptiveScheduler ...
    cfg = params['config']
    lr, traj = float(cfg['learning_rate']), []
    for k in range(ME * NMB):
        traj.append(lr)
        lr = O.adaptive_lr(lr, float(rows[k, 4]), cfg['kl_threshold'], cfg.get('min_lr', 1e-6), cfg.get('max_lr', 1e-2),
                           cfg.get('lr_multiplier', 1.5))
    assert agent.optimizer.last_and_next_lr() == (traj[-1], lr)
    assert res[9] == traj[-1]                        # train_epoch's last_lr (a2c_common.py:1584)
    # ... and the oracle's trajectory, step for step, as far as its decisions are well-posed
    margin_ok = NMB * ME
    thr = cfg['kl_threshold']
    for k, r in enumerate(ref):
        kl = float(r['kl'])
        if min(abs(kl / (2.0 * thr) - 1.0), abs(kl / (0.5 * thr) - 1.0)) < 1e-3:
            margin_ok = k + 1            # the decision after step k is inside fp32 noise of its threshold
            break
    assert margin_ok >= NMB, 'a learning-rate decision of the FIRST mini-epoch lies within 1e-3 of its threshold: pick another seed'
    assert traj[:margin_ok] == [r['lr'] for r in ref[:margin_ok]]
    # ---- all five mini-epochs against the fp64 trajectory (as far as the three runs share their learning rates)
    lr_shared = next((k for k in range(ME * NMB) if not (traj[k] == ref[k]['lr'] == tru[k]['lr'])), ME * NMB)
    groups = [slice(m * NMB, (m + 1) * NMB) for m in range(ME) if (m + 1) * NMB <= max(lr_shared, NMB)]
    report = _check_against_truth(rows, _scalar_rows(ref), _scalar_rows(tru), groups, f'{N} x 32, minibatch {MB}')
    print('mini-epoch, scalar, max |agent - oracle|, envelope |agent - fp64|, envelope |oracle - fp64|, strict vs the oracle:')
    for r in report:
        print('   ', r)
    assert len(groups) == ME or lr_shared < ME * NMB
    # ---- end of the epoch: parameters against the fp64 run's
    if lr_shared == NMB * ME:
        final, ref_sd, tru_sd = agent.model.state_dict(), oracle.model.full_state_dict(), truth.model.full_state_dict()
        for name, v in tru_sd.items():
            if not v.is_floating_point() or v.numel() < 16:
                continue
            v = v.double()
            scale = v.abs().mean().clamp_min(1e-12)
            rel = ((final[name].cpu().double() - v).abs().mean() / scale).item()
            ref_rel = ((ref_sd[name].double() - v).abs().mean() / scale).item()
            assert rel <= max(1e-4, TRUTH_FACTOR * ref_rel, 2e-5 / scale.item()), (name, rel, ref_rel)


def test_kl_conditioning_fp64_demonstration():
    """Why KL is compared at rtol 1e-4, demonstrated: on one 32,768-row minibatch the fused loss kernel's KL and
    the oracle's fp32 KL are each within a few 1e-6 relative of the fp64 value FOR THEIR OWN mu, while the two fp64
    values differ by up to ~1e-4 relative - the difference is inherited from the ~1e-6 relative fp32 rounding
    of mu (different GEMM summation orders), amplified by the cancellation (sigma^2 + dmu^2)/(2 sigma^2) - 1/2."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    N = 2048
    params = configs.humanoid_65536(num_actors=N, minibatch_size=32768, hip_graphs=False)
    params['config']['mini_epochs'] = 1
    torch.manual_seed(5)
    agent = A2CAgent('kl', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    agent.update_epoch()
    agent.train_epoch()
    kl_gpu = agent._mb_scalars[:2, 4].cpu()
    oracle = _oracle_for(params, caps[0], N, 108, 21)
    batch = caps[0]['batch']
    old_mu, old_sigma = batch['mus'].clone(), batch['sigmas'].clone()
    ref = oracle.update(batch)
    vd = agent.dataset.values_dict
    for i in range(2):
        sl = slice(i * 32768, (i + 1) * 32768)
        mu_g, sg_g = vd['mu'][sl].cpu(), vd['sigma'][sl].cpu()
        mu_o, sg_o = oracle.dataset['mu'][sl], oracle.dataset['sigma'][sl]
        true_g = _kl_fp64(mu_g, sg_g, old_mu[sl], old_sigma[sl]).item()
        true_o = _kl_fp64(mu_o, sg_o, old_mu[sl], old_sigma[sl]).item()
        err_g = abs(kl_gpu[i].item() - true_g) / true_g
        err_o = abs(ref[i]['kl'].item() - true_o) / true_o
        # each implementation against the fp64 value of ITS OWN inputs: the kernel (fp64 row sums) is at least as
        # accurate as the fp32 reference formula
        assert err_g <= max(2.0 * err_o, 2e-5), (i, err_g, err_o)
        # and the two fp64 values - same formula, exact arithmetic - already differ at the level the comparison allows
        assert abs(true_g - true_o) / true_o <= 1e-4, (true_g, true_o)
        assert abs(kl_gpu[i].item() - ref[i]['kl'].item()) <= 1e-4 * abs(ref[i]['kl'].item()) + ATOL['kl']


def test_gradients_after_first_step_match_oracle_autograd():
    """The flat gradient arena right after the first optimiser step of a 32,768-row minibatch - i.e. the clipped
    gradients clip_grad_norm_ leaves in p.grad (a2c_common.py:509-512) - against the oracle's autograd, tensor by
    tensor, to 1e-5 of the tensor's scale; the Adam step that follows against torch.optim.Adam on those gradients."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    N = 2048
    params = configs.humanoid_65536(num_actors=N, minibatch_size=32768, hip_graphs=False)
    torch.manual_seed(5)
    agent = A2CAgent('grads', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    agent.set_eval()
    with torch.no_grad():
        batch = agent.play_steps()
    state = {k: v.detach().cpu().clone() for k, v in agent.model.state_dict().items()}
    cpu_batch = {k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
    agent.set_train()
    agent.prepare_dataset(batch)
    agent._prepare_obs_fold()
    before = {n: p.detach().cpu().clone() for n, p in agent.model.named_parameters()}
    agent._with_fold(0, agent.train_actor_critic, agent.dataset[0])
    oracle = _oracle_for(params, {'state': state}, N, 108, 21)
    oracle.prepare_dataset(cpu_batch)
    oracle.minibatch_step(0)
    want = dict(oracle.model.a2c_network.named_parameters())
    for name, p in agent.model.named_parameters():
        key = name.replace('a2c_network.', '')
        g_ref = want[key].grad
        g = p.grad.cpu()
        scale = g_ref.abs().max().item()
        assert (g - g_ref).abs().max().item() <= 1e-5 * scale + 1e-9, (name, (g - g_ref).abs().max().item(), scale)
        # the step: |delta p| <= lr everywhere (Adam, first step), and it agrees with the oracle's step wherever the
        # gradient is not at rounding-noise level (there the sign of g/|g| is not determined in fp32)
        step_gpu = p.detach().cpu() - before[name]
        step_ref = want[key].detach() - before[name]
        solid = g_ref.abs() > 1e-4 * scale
        assert torch.allclose(step_gpu[solid], step_ref[solid], rtol=1e-4, atol=1e-9), name
        assert step_gpu.abs().max().item() <= 3e-4 * (1 + 1e-5)


def test_three_epochs_on_config2_stay_on_the_oracle_trajectory():
    """Drift: BASELINE configs[1] (4,096 x 16, obs 60, act 8, [256,128,64], minibatch 32,768, 4 mini-epochs) for
    THREE consecutive epochs on the same env stream.  The agent plays; the oracle is fed each epoch's rollout and
    continues from ITS OWN parameters, normaliser statistics, Adam moments and learning rate, so every difference
    accumulates - and so does a third run, the oracle in double precision (_truth_for), the yardstick of
    _check_against_truth: per epoch and scalar the agent agrees with the oracle at rtol 1e-5, or is at most 1.5 x as far
    from the fp64 trajectory as the oracle's fp32 arithmetic is (running maxima), never farther than 1e-3 of the scalar's
    scale.  The first epoch must hold the strict bounds against the oracle outright.  One seed, no search (rounds 4 - 5
    tried seeds until the oracle saw no row within 1e-6 of a clip kink and fell back to 2e-3 behind such a row: when a row
    lands on the other side of a kink the question is which run left the trajectory, and the fp64 run answers it).
    Learning rates: identical to the oracle's after every epoch unless the oracle itself disagrees with the fp64 run
    (a KL within rounding of a threshold of the rule).  Parameters after the third epoch: on average within max(1e-4 of
    the tensor's scale, 1.5 x the oracle's own distance) of the fp64 parameters."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    N, seed = 4096, 9
    params = configs.ant_4096(hip_graphs=True)
    torch.manual_seed(seed)
    agent = A2CAgent('drift', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    caps = _capture_rollout(agent)
    oracle = truth = None
    rows, ref, tru, groups = [], [], [], []
    for epoch in range(3):
        agent.update_epoch()
        res = agent.train_epoch()
        got = torch.stack([torch.stack(res[4]), torch.stack(res[5]), torch.stack(res[7]), torch.stack(res[6])], 1).cpu()
        if oracle is None:
            oracle = _oracle_for(params, caps[0], N, 60, 8)
            truth = _truth_for(params, caps[0], N, 60, 8)
        r32 = oracle.update(caps[epoch]['batch'])
        r64 = truth.update(_batch64(caps[epoch]['batch']))
        n = got.shape[0]
        assert n == len(r32)
        # (per-minibatch KL is not part of train_epoch's result: the three loss scalars + b_loss; KL column = the oracle's)
        kl32 = torch.stack([r['kl'].reshape(()).double() for r in r32])
        rows.append(torch.cat([got.double(), kl32[:, None]], 1))
        ref.append(_scalar_rows(r32))
        tru.append(_scalar_rows(r64))
        groups.append(slice(epoch * n, (epoch + 1) * n))
        if epoch == 0:
            for key in ('a_loss', 'c_loss', 'entropy', 'b_loss'):
                g, want = rows[0][:, COLS[key]].float(), ref[0][:, COLS[key]].float()
                assert torch.allclose(g, want, rtol=RTOL, atol=ATOL[key]), (key, (g - want).abs().max().item())
        lr = agent.optimizer.last_and_next_lr()[1]
        assert lr == oracle.lr or oracle.lr != truth.lr, (epoch, lr, oracle.lr, truth.lr)
        if oracle.lr != truth.lr or lr != oracle.lr:
            break                                   # (the runs are on different learning rates from here on)
    report = _check_against_truth(torch.cat(rows), torch.cat(ref), torch.cat(tru), groups, 'config #2, three epochs')
    print('epoch, scalar, max |agent - oracle|, envelope |agent - fp64|, envelope |oracle - fp64|, strict vs the oracle:')
    for r in report:
        print('   ', r)
    if len(groups) == 3:
        final, ref_sd, tru_sd = agent.model.state_dict(), oracle.model.full_state_dict(), truth.model.full_state_dict()
        for name, v in tru_sd.items():
            if v.is_floating_point() and v.numel() >= 16:
                v = v.double()
                scale = v.abs().mean().clamp_min(1e-12)
                rel = ((final[name].cpu().double() - v).abs().mean() / scale).item()
                ref_rel = ((ref_sd[name].double() - v).abs().mean() / scale).item()
                assert rel <= max(1e-4, TRUTH_FACTOR * ref_rel), (name, rel, ref_rel)
