"""GPU: the chunked env-major GAE kernel of horizons above 64 (csrc/gae.hip, gae_long_kernel) through
gae_returns_advantages / compute_gae and, with `long_horizon_gae: True`, through the agent.  fp32 results are
required to be BIT-EXACT against the oracle's scalar scan; the fp64 partial sums against numpy's."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle.seeded_inputs import gae_inputs
from rl_games_amd.synthetic_env import SyntheticTensorEnv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _guarded(n, h, dtype=torch.float32):
    """[n + 1, h] of NaN: the kernel writes rows [0, n), row n is the guard behind the output."""
    return torch.full((n + 1, h), float('nan'), dtype=dtype, device=DEV)


# one ragged chunk of 4; a ragged chunk between full chunks; exact multiples of the chunk; a single env; a ragged env
# tile; many chunks
@pytest.mark.parametrize('H,N', [(68, 64), (100, 65), (128, 130), (132, 1), (256, 63), (516, 200)])
@pytest.mark.parametrize('p_done', [0.0, 0.05, 1.0])
@pytest.mark.parametrize('gamma,tau', [(0.99, 0.95), (1.0, 1.0)])
def test_long_kernel_bit_exact_with_moments_and_guards(H, N, p_done, gamma, tau):
    from rl_games_amd.gae import compute_gae, gae_returns_advantages, num_moment_partials
    r, v, d, lv, ld = gae_inputs(H, N, 1, seed=2, p_done=p_done)
    v = v * 3 + 1
    advs = c_oracle.gae_f32_scan(r.numpy(), v.numpy(), d.numpy(), lv.numpy(), ld.numpy(), gamma, tau)
    ret_ref, adv_ref = c_oracle.returns_and_advantages(advs, v.numpy())
    rp = r[..., 0].t().contiguous().to(DEV)
    vp = v[..., 0].t().contiguous().to(DEV)
    dp = d.t().contiguous().to(torch.uint8).to(DEV)
    lvp, ldp = lv[:, 0].contiguous().to(DEV), ld.to(torch.uint8).to(DEV)
    tiles = num_moment_partials(N)
    assert tiles == -(-N // 64)
    ret, adv, part = _guarded(N, H), _guarded(N, H), _guarded(tiles, 6, torch.float64)
    gae_returns_advantages(rp, vp, dp, lvp, ldp, gamma, tau, out_returns=ret[:N], out_advantages=adv[:N],
                           moment_partials=part[:tiles])
    # physical layout is [N,H]: compare against the time-major oracle transposed
    assert np.array_equal(ret[:N].cpu().numpy(), ret_ref[..., 0].T)
    assert np.array_equal(adv[:N].cpu().numpy(), adv_ref[..., 0].T)
    assert not torch.isnan(part[:tiles]).any()                       # ceil(N/64) rows written ...
    for guard in (ret[N], adv[N], part[tiles]):                      # ... and nothing behind any output
        assert torch.isnan(guard).all()
    m = part[:tiles].sum(0).cpu().numpy()
    for k, x in enumerate((adv_ref, v.numpy(), ret_ref)):
        x = x.astype(np.float64)
        assert np.isclose(m[2 * k], x.sum(), rtol=1e-12, atol=1e-9)
        assert np.isclose(m[2 * k + 1], (x * x).sum(), rtol=1e-12, atol=1e-9)
    # the raw form on rollout-buffer views of the same storage
    out = compute_gae(rp.t().unsqueeze(2), vp.t().unsqueeze(2), dp.t(), lv.to(DEV), ldp, gamma, tau)
    assert out.shape == r.shape and out.stride(0) == 1               # came from the env-major kernel
    assert np.array_equal(out.cpu().numpy(), advs)


def test_long_envelope_and_argument_errors():
    from rl_games_amd import _lib
    lib = _lib.load()
    assert [lib.rlg_gae_long_supported(h) for h in (68, 128, 4096)] == [1, 1, 1]
    assert [lib.rlg_gae_long_supported(h) for h in (64, 32, 130, 0)] == [0, 0, 0, 0]
    x = torch.zeros(64 * 128 + 4, device=DEV)
    b = torch.zeros(64 * 128, dtype=torch.uint8, device=DEV)
    good = dict(rewards=x.data_ptr(), values=x.data_ptr(), dones=b.data_ptr(), last_values=x.data_ptr(),
                last_dones=b.data_ptr(), out=x.data_ptr(), advantages_or_null=x.data_ptr(), num_envs=64, horizon=128,
                gamma=0.99, gamma_tau=0.94, raw=0)
    assert lib.rlg_gae_long(None, None) == 1                         # hipErrorInvalidValue, nothing launched
    for bad in (dict(values=None), dict(advantages_or_null=None), dict(horizon=64), dict(horizon=130),
                dict(out=x.data_ptr() + 4), dict(ev_start_or_null=1)):
        desc = _lib.GaeLongDesc(**{**good, **bad})
        assert lib.rlg_gae_long(ctypes.addressof(desc), None) == 1, bad


def _rollout(cap, key):
    from rl_games_amd.agent import A2CAgent
    params = copy.deepcopy(cap['params'])
    params['config'].update(device=DEV, horizon_length=128, minibatch_size=2048, long_horizon_gae=key)
    env = SyntheticTensorEnv(cap['env']['num_envs'], cap['env']['obs_dim'], cap['env']['act_dim'],
                             device=DEV, seed=cap['env']['seed'])
    params['config']['vec_env'] = env
    params['config']['env_info'] = env.get_env_info()
    torch.manual_seed(5)
    agent = A2CAgent('test', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    agent.set_eval()
    with torch.no_grad():
        batch = agent.play_steps()
    agent.set_train()
    agent.prepare_dataset(batch)
    return batch, agent.dataset.values_dict


def test_agent_takes_the_fused_branch_with_the_key(golden):
    """64 envs x 128 steps, the same seeds with `long_horizon_gae` on and off: the returns of the chunked kernel and of
    the strided scan + torch add are the same bits, and the datasets (normalised with moments summed in two different
    partitions, fp64) agree far inside the suite's 1e-5 dataset bound."""
    cap = golden('epoch.pt')['default']
    (b_on, ds_on), (b_off, ds_off) = _rollout(cap, True), _rollout(cap, False)
    assert '_fused' in b_on and '_fused' not in b_off
    assert torch.equal(b_on['returns'], b_off['returns'])
    for k in ('old_values', 'returns', 'advantages'):
        assert torch.allclose(ds_on[k], ds_off[k], rtol=1e-6, atol=1e-7), k
