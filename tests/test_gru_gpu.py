"""GPU: single-layer GRU policies on the sequence-persistent kernels (csrc/gru.hip: 16 / 32 / 64 units with W_hh in
LDS; csrc/gru_wide.hip: 128 units with W_hh in registers as MFMA fragments).

Kernel level: against a CPU evaluation in fp64 of torch.nn.GRU stepped with the reference's done resets
(rl_games/common/layers/recurrent.py), backward through autograd on the CPU side - the procedure and the tolerances
of tests/test_lstm_wide_gpu.py, restated here.  Agent level: the engine against torch autograd, one epoch of the real
reference agent (tests/golden/gru.pt.gz, written by tests/golden/make_gru_golden.py), and three training epochs
including the HIP-graph replays."""
import copy
import gzip
import io
import os

import pytest
import torch

from rl_games_amd.synthetic_env import SyntheticTensorEnv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _reference(x, gru, h0, dones, T):
    """x [S*T, I] rows (seq, t).  Returns out [S*T, H], hT [1, S, H], hn_all = W_hn h + b_hn [S*T, H] and the states
    entering each step after the reset [S*T, H]."""
    S = x.shape[0] // T
    H = h0.shape[1]
    xs = x.reshape(S, T, -1).transpose(0, 1)
    d = dones.reshape(S, T).t() if dones is not None else None
    st = h0.unsqueeze(0)
    outs, hns, entering = [], [], []
    for t in range(T):
        if d is not None:
            st = st * (1.0 - d[t].float()).reshape(1, -1, 1).to(st.dtype)
        entering.append(st)
        hns.append(st @ gru.weight_hh_l0[2 * H:].t() + gru.bias_hh_l0[2 * H:])
        o, st = gru(xs[t:t + 1], st)
        outs.append(o)

    def rows(parts):
        return torch.cat(parts, 0).transpose(0, 1).reshape(S * T, -1)
    return rows(outs), st, rows(hns), rows(entering)


def _inputs(S, T, I, H, with_dones):
    """Seeded parameters (a generator of their own, seeded from the shape: a case's weights do not depend on what ran
    before it), inputs, initial states, dones and d_out.  The dones are a 20 % draw in which sequence S // 2 is then
    cleared (an episode that outlasts the window) and a reset is SET at t = 0 of sequence 0 and at t = T - 1 of
    sequence 1: the three places where step_keep and the hprev / h_final stores differ from the middle of a sequence
    are in every case, and asserted to be."""
    g = torch.Generator().manual_seed(S * 7 + T)
    gru32 = torch.nn.GRU(I, H, 1)
    gw = torch.Generator().manual_seed(S * 7 + T + 1000 * H)
    with torch.no_grad():
        for p in gru32.parameters():            # torch.nn.GRU's own initialisation, from a seeded generator
            p.uniform_(-H ** -0.5, H ** -0.5, generator=gw)
    x32 = torch.randn(S * T, I, generator=g)
    h0 = (0.5 * torch.randn(S, H, generator=g)).to(DEV)
    dones = None
    if with_dones:
        d = (torch.rand(S * T, generator=g) < 0.2).to(torch.uint8).reshape(S, T)
        d[S // 2] = 0
        d[0, 0] = 1
        if T > 1 and S > 1:
            d[1, T - 1] = 1
        assert d[:, 0].any() and d[:, T - 1].any() and (d.sum(1) == 0).any() and (d.sum(1) > 0).any()
        dones = d.reshape(S * T).to(DEV)
    d_out = torch.randn(S * T, H, generator=g).to(DEV)
    return gru32, x32, h0, dones, d_out


def _poison(*shape):
    """An output buffer that starts as NaN: a row the kernel never stores cannot pass on stale memory."""
    return torch.full(shape, float('nan'), device=DEV)


def _no_poison_left(**buffers):
    for name, b in buffers.items():
        assert b is None or not torch.isnan(b).any(), f'NaN left in {name}'


def _forward(ops, gru32, x, h0, dones, T, train=True):
    S, H = h0.shape
    w_ih, w_hh = gru32.weight_ih_l0.detach().to(DEV), gru32.weight_hh_l0.detach().to(DEV).contiguous()
    b_ih, b_hh = gru32.bias_ih_l0.detach().to(DEV), gru32.bias_hh_l0.detach().to(DEV)
    gates = torch.addmm(b_ih, x, w_ih.t())
    out = _poison(S * T, H)
    hn_all = _poison(S * T, H) if train else None
    hprev = _poison(S * T, H) if train else None
    hT = _poison(S, H)
    ops.gru_seq_forward(gates, w_hh, b_hh, h0, dones, out, hn_all, hprev, hT, seq_len=T)
    _no_poison_left(gates=gates, out=out, hn_all=hn_all, hprev=hprev, hT=hT)
    return dict(gates=gates, out=out, hn_all=hn_all, hprev=hprev, hT=hT, w_ih=w_ih, w_hh=w_hh)


def _backward(ops, r, dones, d_out, T):
    d_gx, d_gh = _poison(*r['gates'].shape), _poison(*r['gates'].shape)
    ops.gru_seq_backward(r['gates'], r['hn_all'], r['hprev'], dones, r['w_hh'], d_out, d_gx, d_gh, T)
    _no_poison_left(d_gx=d_gx, d_gh=d_gh)
    return d_gx, d_gh


def _check_against_fp64(S, T, I, with_dones, H, inputs=None):
    """One shape against the fp64 CPU GRU at the bounds of test_wide_lstm_forward_backward_match_fp64: out, h_final,
    hn_all, hprev rtol 1e-5 + 2e-6; dx, dW_ih, dW_hh, db_ih, db_hh within 2e-5 max|ref| + 1e-7; repeats bit-identical.
    Returns the kernel's forward results and (d_gx, d_gh)."""
    from rl_games_amd import ops
    gru32, x32, h0, dones, d_out = inputs if inputs is not None else _inputs(S, T, I, H, with_dones)

    # the reference: CPU, fp64, the fp32 parameters and inputs upcast exactly
    gru = torch.nn.GRU(I, H, 1).double()
    gru.load_state_dict({k: v.double() for k, v in gru32.state_dict().items()})
    x = x32.double().requires_grad_(True)
    ref_out, ref_h, ref_hn, ref_enter = _reference(x, gru, h0.cpu().double(), None if dones is None else dones.cpu(), T)
    ref_out.backward(d_out.cpu().double())
    ref_out, ref_h = ref_out.detach().float().to(DEV), ref_h.detach().float().to(DEV)
    ref_hn, ref_enter = ref_hn.detach().float().to(DEV), ref_enter.detach().float().to(DEV)
    ref_grads = {n: getattr(gru, n).grad.float().to(DEV)
                 for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')}
    x_grad = x.grad.float().to(DEV)
    x = x32.to(DEV)

    r = _forward(ops, gru32, x, h0, dones, T)
    tol = dict(rtol=1e-5, atol=2e-6)
    for name, got, want in (('out', r['out'], ref_out), ('hT', r['hT'], ref_h[0]),
                            ('hn_all', r['hn_all'], ref_hn), ('hprev', r['hprev'], ref_enter)):
        print(name, 'max |diff|', (got - want).abs().max().item())
        assert torch.allclose(got, want, **tol), (name, (got - want).abs().max().item())
    # hprev IS the state entering each step: the previous row of out (h0 at t = 0), zeroed where done - bit for bit
    enter = torch.cat([h0.unsqueeze(1), r['out'].reshape(S, T, H)[:, :-1]], 1).reshape(S * T, H)
    if dones is not None:
        enter = enter * (1.0 - dones.float()).unsqueeze(1)
    assert torch.equal(r['hprev'], enter)

    # an inference call (nothing kept for backward) and a second training call: bit-identical
    inf = _forward(ops, gru32, x, h0, dones, T, train=False)
    again = _forward(ops, gru32, x, h0, dones, T)
    for k in ('out', 'hT', 'gates'):
        assert torch.equal(inf[k], r[k]), k
    for k in ('out', 'hT', 'gates', 'hn_all', 'hprev'):
        assert torch.equal(again[k], r[k]), k

    d_gx, d_gh = _backward(ops, r, dones, d_out, T)
    d_gx2, d_gh2 = _backward(ops, r, dones, d_out, T)
    assert torch.equal(d_gx, d_gx2) and torch.equal(d_gh, d_gh2)
    dx = d_gx @ r['w_ih']
    dw_ih = d_gx.t() @ x
    dw_hh = d_gh.t() @ r['hprev']

    def close(a, b, name):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(name, 'max |diff|', err, 'bound', 2e-5 * scale + 1e-7)
        assert err <= 2e-5 * scale + 1e-7, (name, err, scale)
    close(dx, x_grad, 'dx')
    close(dw_ih, ref_grads['weight_ih_l0'], 'dw_ih')
    close(dw_hh, ref_grads['weight_hh_l0'], 'dw_hh')
    close(d_gx.sum(0), ref_grads['bias_ih_l0'], 'db_ih')
    close(d_gh.sum(0), ref_grads['bias_hh_l0'], 'db_hh')
    return r, (d_gx, d_gh)


@pytest.mark.parametrize('H', [16, 32, 64, 128])
@pytest.mark.parametrize('S,T,I,with_dones', [(64, 16, 64, True), (37, 4, 12, True), (1024, 16, 64, True),
                                            (5, 1, 7, False), (130, 8, 20, False), (256, 32, 100, True)])
def test_gru_forward_backward_match_fp64(S, T, I, with_dones, H):
    """The shapes and bounds of test_wide_lstm_forward_backward_match_fp64 at every supported width.  As measured on
    an MI355X every quantity meets these LSTM bounds - no bound was re-derived from an fp32 CPU GRU."""
    _check_against_fp64(S, T, I, with_dones, H)


@pytest.mark.parametrize('H', [16, 32, 64, 128])
@pytest.mark.parametrize('S,T', [(4099, 2), (2050, 3)])
def test_gru_large_tiles_match_fp64_and_small_tiles(S, T, H):
    """csrc/gru.hip picks its tile from the number of sequences: 16 per workgroup (4 per thread at 64 units) once that
    still fills 256 workgroups - the 4,096-env rollout step -, 8 from about 2,048, fewer below.  S = 4,099 and 2,050
    select the 16- and 8-sequence instantiations with a ragged last tile; same bounds as above, and the first five
    sequences are bit-identical to the same five launched alone (the smallest tile), forward and backward."""
    from rl_games_amd import ops
    I, n = 12, 5
    gru32, x32, h0, dones, d_out = inputs = _inputs(S, T, I, H, True)
    full, (gx_full, gh_full) = _check_against_fp64(S, T, I, True, H, inputs)
    part = _forward(ops, gru32, x32[:n * T].to(DEV), h0[:n].contiguous(), dones[:n * T].contiguous(), T)
    for k in ('out', 'gates', 'hn_all', 'hprev'):
        assert torch.equal(full[k][:n * T], part[k]), k
    assert torch.equal(full['hT'][:n], part['hT'])
    gx_part, gh_part = _backward(ops, part, dones[:n * T].contiguous(), d_out[:n * T].contiguous(), T)
    assert torch.equal(gx_full[:n * T], gx_part) and torch.equal(gh_full[:n * T], gh_part)


@pytest.mark.parametrize('H', [16, 32, 64, 128])
def test_gru_rows_do_not_depend_on_tile_neighbours(H):
    """Sequences 0 - 4 of a 130-sequence launch (full tiles) and the same five alone (a ragged tile): bit-identical
    rows, forward and backward - at every width: 16 and 32 units split the tile's sequences over the threads in
    another way (16 and 8 thread groups of one sequence each) than 64 (4 groups) and the 128-unit MFMA columns."""
    from rl_games_amd import ops
    S, T, I, n = 130, 8, 20, 5
    gru32, x32, h0, dones, d_out = _inputs(S, T, I, H, True)
    x = x32.to(DEV)
    full = _forward(ops, gru32, x, h0, dones, T)
    part = _forward(ops, gru32, x[:n * T].contiguous(), h0[:n].contiguous(), dones[:n * T].contiguous(), T)
    for k in ('out', 'gates', 'hn_all', 'hprev'):
        assert torch.equal(full[k][:n * T], part[k]), k
    assert torch.equal(full['hT'][:n], part['hT'])
    gx_full, gh_full = _backward(ops, full, dones, d_out, T)
    gx_part, gh_part = _backward(ops, part, dones[:n * T].contiguous(), d_out[:n * T].contiguous(), T)
    assert torch.equal(gx_full[:n * T], gx_part)
    assert torch.equal(gh_full[:n * T], gh_part)


def test_gru_supported_widths():
    from rl_games_amd import ops
    assert all(ops.gru_supported(h) for h in (16, 32, 64, 128))
    assert not ops.gru_supported(100) and not ops.gru_supported(256)
    with pytest.raises(RuntimeError):
        ops.gru_seq_forward(torch.zeros(4, 768, device=DEV), torch.zeros(768, 256, device=DEV),
                            torch.zeros(768, device=DEV), torch.zeros(4, 256, device=DEV), None,
                            torch.zeros(4, 256, device=DEV))


@pytest.mark.parametrize('U', [64, 128])
def test_gru_engine_matches_autograd_gradients_and_rollout(U):
    """test_wide_lstm_engine_matches_autograd_gradients_and_rollout with a GRU: (i) the engine's rollout step (T = 1
    launches) leaves the values / mus the torch model gives step by step, and (ii) for one minibatch the hand-written
    BPTT produces autograd's scalars and gradients."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    base = configs.pendulum_gru_4096(num_actors=128, units=U, minibatch_size=1024, grad_norm=1e9,
                                     lr_schedule=None, learning_rate=0.0)
    base['config']['env_config']['p_done'] = 0.2          # plenty of mid-sequence resets
    torch.manual_seed(0)
    a1 = A2CAgent('eng', copy.deepcopy(base))
    p2 = copy.deepcopy(base)
    p2['config']['manual_lstm'] = False
    a2 = A2CAgent('auto', p2)
    assert a1._engine is not None and a1._engine.lstm is None and a1._engine.gru is not None and a2._engine is None
    assert a1.model.a2c_network.rnn_units == U and a1.model.a2c_network.rnn_name == 'gru'
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
        assert len(batch['rnn_states']) == 1
        st = [s[:, :N].contiguous() for s in batch['rnn_states']]     # states at t = 0 (one seq per env)
        assert st[0].shape == (1, N, U)
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
    assert a1._engine.last_dw_path == 'mfma'
    print('scalars', g1['_scalars'].tolist(), g2['_scalars'].tolist())
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    for n in g2:
        scale = g2[n].abs().max().item() + 1e-12
        print(n, 'max |diff|', (g1[n] - g2[n]).abs().max().item(), 'scale', scale)
        assert torch.allclose(g1[n], g2[n], rtol=1e-4, atol=5e-6 * scale), (n, (g1[n] - g2[n]).abs().max().item(), scale)


# ---- one epoch of the real reference agent ------------------------------------------------------------------------

COLS = {'a_loss': 0, 'c_loss': 1, 'entropy': 2, 'kl': 3, 'b_loss': 4}
RTOL = {'a_loss': 1e-5, 'c_loss': 1e-5, 'entropy': 1e-5, 'kl': 1e-4, 'b_loss': 1e-5}
ATOL = {'a_loss': 2e-6, 'c_loss': 2e-6, 'entropy': 2e-6, 'kl': 2e-7, 'b_loss': 1e-7}
TRUTH_FACTOR = 1.5      # the agent may be this much farther from the fp64 trajectory than the reference's own fp32 arithmetic
CEILING = 1e-3          # ... and never farther than this fraction of a scalar's scale


def _check_against_truth(got, ref, tru, key):
    """The criterion of tests/test_lstm_wide_gpu.py::_check_against_truth for one scalar's series (steps, or
    mini-epochs for the KL): every entry EITHER agrees with the recorded fp32 value at the plain bound OR the agent is,
    up to there, at most TRUTH_FACTOR x as far from the fp64 trajectory as the recorded fp32 values are (running
    maxima) - and in no case farther than CEILING of the scalar's scale.  Returns the entries that needed the fp64
    yardstick."""
    got, ref, tru = got.double(), ref.double(), tru.double()
    scale = float(ref.abs().max())
    env_a = env_o = 0.0
    needed = []
    for i in range(got.shape[0]):
        strict = bool((got[i] - ref[i]).abs() <= RTOL[key] * ref[i].abs() + ATOL[key])
        env_a = max(env_a, float((got[i] - tru[i]).abs()))
        env_o = max(env_o, float((ref[i] - tru[i]).abs()))
        print(f'{key}[{i}] |agent - ref| {float((got[i] - ref[i]).abs()):.3e} |agent - fp64| {env_a:.3e} '
              f'|ref - fp64| {env_o:.3e} strict {strict}')
        if not strict:
            needed.append(i)
            assert env_a <= TRUTH_FACTOR * env_o + ATOL[key], (key, i, env_a, env_o)
        assert env_a <= CEILING * scale + ATOL[key], (key, i, 'ceiling', env_a, scale)
    return needed


def test_gru_matches_reference_epoch():
    """MLP [64, 64] + GRU 128, obs 3, act 1, 512 envs x seq_len 16, minibatch 2,048 x 4 mini-epochs = 16 optimiser
    steps against one train_epoch of the REAL reference agent on the recorded rollout and rnn states, through the
    register-resident GRU kernels of the manual engine.  Bounds of test_wide_lstm_matches_reference_epoch: a / c /
    entropy losses rtol 1e-5 + 2e-6, b_loss + 1e-7, mini-epoch KL rtol 1e-4 + 2e-7, final learning rate bit for bit.
    An entry outside its plain bound is held to the fp64 trajectory recorded next to it (truth_*;
    _check_against_truth).
    As measured on an MI355X: all 16 steps and all 4 mini-epoch KLs meet the plain bounds (largest |agent - reference|:
    a_loss 7.5e-9, c_loss 2.4e-7, entropy 3.6e-7, b_loss 0, KL 4.7e-9) - no entry needed the fp64 yardstick; the agent
    ends 1.6e-7 from the fp64 c_loss where the recorded fp32 reference ends 2.5e-7 from it."""
    from conftest import GOLDEN_DIR
    from rl_games_amd.agent import A2CAgent
    with gzip.open(os.path.join(GOLDEN_DIR, 'gru.pt.gz'), 'rb') as f:
        cap = torch.load(io.BytesIO(f.read()), map_location='cpu', weights_only=False)
    params = copy.deepcopy(cap['params'])
    params['config'].update(device=DEV, manual_lstm=True)
    env = SyntheticTensorEnv(cap['env']['num_envs'], cap['env']['obs_dim'], cap['env']['act_dim'], device=DEV,
                             seed=cap['env']['seed'])
    params['config']['vec_env'] = env
    params['config']['env_info'] = env.get_env_info()
    agent = A2CAgent('test', params)
    agent.init_tensors()
    assert agent.is_rnn and agent._engine is not None and agent._engine.lstm is None and agent._engine.gru is not None
    assert agent.model.a2c_network.rnn_units == 128 and agent.model.a2c_network.rnn_name == 'gru'
    assert (agent.num_actors, agent.horizon_length, agent.seq_length, agent.minibatch_size) == (512, 16, 16, 2048)
    agent.model.load_state_dict(cap['state_after_rollout'])
    assert len(cap['batch']['rnn_states']) == 1
    batch = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [s.to(DEV) for s in v])
             for k, v in cap['batch'].items()}
    agent.set_train()
    agent.prepare_dataset(batch)
    rows = []
    for mini_ep in range(agent.mini_epochs_num):
        for i in range(len(agent.dataset)):
            a, c, e, kl, lr, lr_mul, mu, sigma, b = agent.train_actor_critic(agent.dataset[i])
            rows.append(torch.stack([a, c, e, kl, b]).clone())
    rows = torch.stack(rows).cpu()
    assert rows.shape[0] == 16
    kls = rows[:, 3].reshape(agent.mini_epochs_num, len(agent.dataset)).mean(1)
    needed = {}
    for key, name in (('a_loss', 'a_losses'), ('c_loss', 'c_losses'), ('entropy', 'entropies'), ('b_loss', 'b_losses')):
        needed[key] = _check_against_truth(rows[:, COLS[key]], cap[name].reshape(-1), cap['truth_' + name].reshape(-1), key)
    needed['kl'] = _check_against_truth(kls, cap['mini_epoch_kls'].reshape(-1), cap['truth_mini_epoch_kls'].reshape(-1), 'kl')
    print('entries that needed the fp64 yardstick:', needed)
    # the learning-rate trajectory of the 16 steps (update_lr calls of the reference), bit for bit
    assert agent.optimizer.last_and_next_lr()[1] == cap['lrs'][-1]


@pytest.mark.parametrize('U', [64, 128])
def test_gru_config_train_epoch_runs(U):
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    params = configs.pendulum_gru_4096(num_actors=256, units=U)
    agent = A2CAgent('gru', params)
    assert agent._engine is not None and agent._engine.lstm is None and agent._engine.gru is not None
    agent.init_tensors()
    agent.obs = agent.env_reset()
    for _ in range(3):                      # 1 eager epoch, then HIP-graph replays on the engine path
        agent.update_epoch()
        out = agent.train_epoch()
    assert len(out[4]) == agent.mini_epochs_num * agent.num_minibatches
    assert all(torch.isfinite(x).item() for x in out[4])
    st = agent.dataset.values_dict
    assert st is not None and isinstance(st['rnn_states'], list) and len(st['rnn_states']) == 1
    assert st['rnn_states'][0].shape == (1, 256 * (16 // 16), U)
