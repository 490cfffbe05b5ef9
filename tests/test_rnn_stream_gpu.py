"""GPU: 256-unit LSTM / GRU policies on the streamed sequence kernels (csrc/rnn_stream.hip, `wide_rnn_kernels: True`).

Kernel level: the launches against a CPU evaluation in fp64 of the same steps (`_steps`: the cells of torch.nn.LSTM /
torch.nn.GRU stepped with the reference's done resets, rl_games/common/layers/recurrent.py:26-58), gradients through
autograd on that side.  Tolerances are those of the 128-unit tests (tests/test_lstm_wide_gpu.py, tests/test_gru_gpu.py),
unwidened although K is 256 here: forward rtol 1e-5 + 2e-6, backward 2e-5 x scale + 1e-7 (profiles/rnn_stream.txt has the
measured errors next to those of a plain fp32 torch evaluation of the same steps).
Agent level: the engines against the same agent on torch modules, and the key's default."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 256
NG = {'lstm': 4, 'gru': 3}
SHAPES = [(1, 1), (17, 3), (33, 4), (64, 16)]      # a lone live slot and T = 1, ragged last tiles, a multi-tile grid


def _steps(cell, gx, w_hh, b_hh, h0, c0, dones, T, gh_extra=None):
    """gx [S*T, NG*H] rows (seq, t): the gate inputs.  Returns out, (c_t | hn), the state entering each step, hT, cT,
    each [S*T, H] / [S, H], in the dtype and on the device of its arguments.  gh_extra: zeros added to the GRU's hidden
    side, whose gradient is d_gh."""
    S = gx.shape[0] // T
    x = gx.reshape(S, T, -1)
    keep = torch.ones(S, T, 1, dtype=gx.dtype, device=gx.device)
    if dones is not None:
        keep = 1.0 - dones.reshape(S, T, 1).to(gx.dtype)
    h, c = h0, c0
    outs, kept, entering = [], [], []
    for t in range(T):
        h = h * keep[:, t]
        entering.append(h)
        a = h @ w_hh.t()
        if cell == 'lstm':
            i, f, g, o = (x[:, t] + a).chunk(4, 1)
            c = torch.sigmoid(f) * (c * keep[:, t]) + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            kept.append(c)
        else:
            a = a + b_hh + (0 if gh_extra is None else gh_extra.reshape(S, T, -1)[:, t])
            (xr, xz, xn), (ar, az, hn) = x[:, t].chunk(3, 1), a.chunk(3, 1)
            z = torch.sigmoid(xz + az)
            h = (1.0 - z) * torch.tanh(xn + torch.sigmoid(xr + ar) * hn) + z * h
            kept.append(hn)
        outs.append(h)

    def rows(parts):
        return torch.stack(parts, 1).reshape(S * T, -1)
    return rows(outs), rows(kept), rows(entering), h, c


def _poison(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def _launch(ops, cell, packed, gx, w_hh, b_hh, h0, c0, dones, d_out, T, train=True):
    """Forward (and, for a training launch, backward) on NaN-filled output buffers; asserts that none is left."""
    rows, S = gx.shape[0], h0.shape[0]
    r = dict(gates=gx.clone(), out=_poison(rows, H), kept=_poison(rows, H) if train else None,
             hprev=_poison(rows, H) if train else None, hT=_poison(S, H), cT=_poison(S, H) if cell == 'lstm' else None)
    if cell == 'lstm':
        fwd = (r['gates'], w_hh, h0, c0, dones, r['out'], r['kept'], r['hprev'], r['hT'], r['cT'])
    else:
        fwd = (r['gates'], w_hh, b_hh, h0, dones, r['out'], r['kept'], r['hprev'], r['hT'])
    ops.rnn_seq(cell, 'forward', [fwd], T, packed=packed)
    if train:
        r['d_gx'], r['d_gh'] = _poison(*gx.shape), (_poison(*gx.shape) if cell == 'gru' else None)
        if cell == 'lstm':
            bwd = (r['gates'], r['kept'], c0, dones, w_hh, d_out, r['d_gx'])
        else:
            bwd = (r['gates'], r['kept'], r['hprev'], dones, w_hh, d_out, r['d_gx'], r['d_gh'])
        ops.rnn_seq(cell, 'backward', [bwd], T, packed=packed)
    for name, b in r.items():
        assert b is None or not torch.isnan(b).any(), f'NaN left in {name}'
    return r


@functools.lru_cache(maxsize=None)
def _case(cell, S, T):
    """Seeded inputs of one shape (never modified), the kernels' training launch on them, and the fp64 evaluation.
    Dones: a reset at t = 0 of sequence 0 and at t = T - 1 of sequence 1, a 20 % draw elsewhere, none in sequence S // 2
    (where S > 2)."""
    from rl_games_amd import ops
    g = torch.Generator().manual_seed(1000 * NG[cell] + 7 * S + T)
    G = NG[cell] * H
    w_hh = torch.empty(G, H).uniform_(-H ** -0.5, H ** -0.5, generator=g)
    b_hh = torch.empty(G).uniform_(-H ** -0.5, H ** -0.5, generator=g)
    gx, d_out = torch.randn(S * T, G, generator=g), torch.randn(S * T, H, generator=g)
    h0, c0 = 0.5 * torch.randn(S, H, generator=g), 0.5 * torch.randn(S, H, generator=g)
    d = (torch.rand(S, T, generator=g) < 0.2).to(torch.uint8)
    d[0, 0] = 1
    if S > 2:
        d[S // 2] = 0
        d[1, T - 1] = 1
        assert (d.sum(1) == 0).any()
    inp = dict(gx=gx, w_hh=w_hh, b_hh=b_hh, h0=h0, c0=c0, dones=d.reshape(-1), d_out=d_out)

    # the reference: CPU, fp64, the fp32 inputs upcast exactly -> (out, kept, entering, hT, cT, d_gx, d_gh)
    t = {k: (v if k == 'dones' else v.double()) for k, v in inp.items()}
    x, extra = t['gx'].requires_grad_(True), torch.zeros_like(t['gx']).requires_grad_(True)
    res = _steps(cell, x, t['w_hh'], t['b_hh'], t['h0'], t['c0'], t['dones'], T, extra)
    res[0].backward(t['d_out'])
    truth = [v.detach() for v in res] + [x.grad, extra.grad if cell == 'gru' else None]
    dev = {k: v.to(DEV) for k, v in inp.items()}
    packed = torch.empty(ops.rnn_stream_pack_floats(cell, H), device=DEV)
    ops.rnn_stream_pack(cell, dev['w_hh'], packed)
    args = (cell, packed, dev['gx'], dev['w_hh'], dev['b_hh'], dev['h0'], dev['c0'], dev['dones'], dev['d_out'], T)
    return dict(args=args, dev=dev, got=_launch(ops, *args), truth=truth)


@pytest.mark.parametrize('S,T', SHAPES)
@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_stream_kernels_match_fp64(cell, S, T):
    case = _case(cell, S, T)
    got, truth = case['got'], case['truth']
    for k, name in enumerate(('out', 'kept', 'hprev', 'hT', 'cT', 'd_gx', 'd_gh')):
        if got[name] is None:
            continue
        want = truth[k].to(DEV)
        err = (got[name].double() - want).abs()
        # forward: allclose(rtol 1e-5, atol 2e-6); backward: 2e-5 x scale + 1e-7
        bound = 1e-5 * want.abs() + 2e-6 if k < 5 else torch.full_like(err, 2e-5 * want.abs().max().item() + 1e-7)
        print(f'{cell} S {S} T {T} {name}: max |err| {err.max().item():.3e}  largest bound {bound.max().item():.3e}')
        assert (err <= bound).all(), (name, err.max().item())


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_stream_bit_level_contract(cell):
    """hprev is the state entering each step; inference and training launches, and a second call, give equal bits; a
    launch over the first 21 sequences (a full tile and a ragged one) equals those rows of the 64-sequence launch."""
    from rl_games_amd import ops
    S, T, n = 64, 16, 21
    case = _case(cell, S, T)
    got, dev, args = case['got'], case['dev'], case['args']
    enter = torch.cat([dev['h0'].unsqueeze(1), got['out'].reshape(S, T, H)[:, :-1]], 1).reshape(S * T, H)
    assert torch.equal(got['hprev'], enter * (1.0 - dev['dones'].float()).unsqueeze(1))
    inference, again = _launch(ops, *args, train=False), _launch(ops, *args)
    for k in ('gates', 'out', 'hT', 'cT'):
        assert got[k] is None or torch.equal(inference[k], got[k]), k
    for k, v in got.items():
        assert v is None or torch.equal(again[k], v), k
    part = _launch(ops, cell, args[1], dev['gx'][:n * T], dev['w_hh'], dev['b_hh'], dev['h0'][:n], dev['c0'][:n],
                   dev['dones'][:n * T], dev['d_out'][:n * T], T)
    for k, v in got.items():
        assert v is None or torch.equal(part[k], v[:part[k].shape[0]]), k


def test_stream_support_queries():
    from rl_games_amd import ops
    assert ops.rnn_stream_supported('lstm', 256) and ops.rnn_stream_supported('gru', 256)
    assert not any(ops.rnn_stream_supported(cell, h) for cell in ('lstm', 'gru') for h in (100, 128, 512))
    assert not ops.lstm_supported(256) and not ops.gru_supported(256)


def _continuous(key, **over):
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    params = configs.pendulum_lstm_4096(num_actors=32, units=256, horizon_length=4, minibatch_size=64, grad_norm=1e9,
                                        lr_schedule=None, learning_rate=0.0, wide_rnn_kernels=key, **over)
    params['config']['seq_length'] = 4
    params['config']['env_config']['p_done'] = 0.2
    torch.manual_seed(0)
    return A2CAgent('test', params)


def _discrete(key, **over):
    from rl_games_amd import configs
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    params = configs.smac_rnn_discrete(num_actors=32, cell='gru', units=256, horizon_length=4, seq_length=4,
                                       minibatch_size=64, wide_rnn_kernels=key, **over)
    torch.manual_seed(0)
    return DiscreteA2CAgent('test', params)


def test_stream_lstm_engine_matches_autograd_gradients_and_rollout():
    """tests/test_lstm_wide_gpu.py::test_wide_lstm_engine_matches_autograd_gradients_and_rollout at 256 units, 32 envs x
    horizon 4 in sequences of 4, at its tolerances: the engine's rollout against the torch model step by step, and one
    minibatch's scalars and gradients against autograd's."""
    a1, a2 = _continuous(True), _continuous(True, manual_lstm=False)
    assert a1._engine is not None and a1._engine.lstm is not None and a1._engine.stations.packed is not None
    assert a2._engine is None and a1.model.a2c_network.rnn_units == 256
    a2.model.load_state_dict(a1.model.state_dict())
    a1.init_tensors()
    a1.obs = a1.env_reset()
    a1.set_eval()
    with torch.no_grad():
        batch = a1.play_steps_rnn()
    a2.init_tensors()
    a2.set_eval()
    Hz, N = a1.horizon_length, a1.num_actors
    obs = batch['obses'].reshape(N, Hz, -1)
    with torch.no_grad():
        st = [s[:, :N].contiguous() for s in batch['rnn_states']]
        for t in range(Hz):
            keep = (1.0 - a1.experience_buffer.tensor_dict['dones'][t].float()).reshape(1, -1, 1)
            st = [s * keep for s in st] if t > 0 else st
            res = a2.model({'is_train': False, 'obs': obs[:, t], 'rnn_states': st})
            st = res['rnn_states']
            assert torch.allclose(res['mus'], batch['mus'].reshape(N, Hz, -1)[:, t], rtol=1e-4, atol=2e-6), t
            assert torch.allclose(res['values'], batch['values'].reshape(N, Hz, 1)[:, t], rtol=1e-4, atol=2e-5), t
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    grads = []
    for ag in (a1, a2):
        b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'}
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset(b)
        ag.train_actor_critic(ag.dataset[1])
        grads.append({n: p.grad.detach().clone() for n, p in ag.model.named_parameters()})
        res = ag.train_result
        grads[-1]['_scalars'] = torch.stack([res[0], res[1], res[2], res[3], res[8]])
    g1, g2 = grads
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    for n in g2:
        scale = g2[n].abs().max().item() + 1e-12
        print(n, 'max |diff|', (g1[n] - g2[n]).abs().max().item(), 'scale', scale)
        assert torch.allclose(g1[n], g2[n], rtol=1e-4, atol=5e-6 * scale), (n, (g1[n] - g2[n]).abs().max().item(), scale)


def test_stream_gru_discrete_engine_trains_with_masks():
    """Three epochs with finite losses that move weight_hh; the rollout steps are replayed as HIP graphs from the second
    epoch on (each replay packs W_hh again), and the same seed without rollout graphs gives the same losses bit for bit."""
    runs = []
    for graphs in (True, False):
        agent = _discrete(True, rollout_graphs=graphs)
        assert agent._rnn_engine is not None and agent._rnn_engine.stations.packed is not None and agent._fast_rollout_ok()
        agent.init_tensors()
        agent.obs = agent.env_reset()
        before = agent.model.a2c_network.rnn.rnn.weight_hh_l0.detach().clone()
        losses = []
        for _ in range(3):
            agent.epoch_num += 1
            losses += [torch.stack(list(x)).cpu() for x in agent.train_epoch()[4:8]]
        assert all(torch.isfinite(x).all() for x in losses)
        assert not torch.equal(agent.model.a2c_network.rnn.rnn.weight_hh_l0, before)
        assert len(agent._rollout_graphs) == (agent.horizon_length if graphs else 0)
        runs.append(losses)
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_key_off_keeps_the_torch_path():
    assert _continuous(False)._engine is None
    agent = _discrete(False)
    assert agent._rnn_engine is None and not agent._fast_rollout_ok()
