"""GPU: the engines on chain_net.RnnStations.
(a) RecurrentChainNet in plain head mode against the same launches spelled out through ops.* in this file, bit for bit,
    and against an fp64 torch LSTM / GRU with autograd on the CPU.
(b) mlp_engine.ManualMLP's recurrent path with the per-layer trunk (`fused_mlp: False`) against the fused trunk.
"""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OBS, TRUNK, S, T = 12, 32, 6, 4
ROWS = S * T


def _network(cell, H):
    """12 observations -> [32] ELU -> LSTM | GRU of H units -> heads of 1 + 3 columns, in an arena laid out as the
    agents lay theirs out."""
    from rl_games_amd.chain_net import arena_layout
    from rl_games_amd.flat_optim import FlatArena
    torch.manual_seed(100 + H + (cell == 'gru'))
    net = nn.ModuleDict(dict(trunk=nn.Sequential(nn.Linear(OBS, TRUNK), nn.ELU()),
                             rnn=(nn.LSTM if cell == 'lstm' else nn.GRU)(TRUNK, H),
                             value=nn.Linear(H, 1), logits=nn.Linear(H, 3))).to(DEV)
    params = list(net.parameters())
    heads = [net['value'], net['logits']]
    arena = FlatArena(params, layout=arena_layout(params, [heads], first_vectors=[net['trunk'][0].bias]))
    return net, heads, arena


def _inputs(cell, H):
    g = torch.Generator().manual_seed(7 + H)
    x = torch.randn(ROWS, OBS, generator=g).to(DEV)
    states = tuple((0.5 * torch.randn(1, S, H, generator=g)).to(DEV) for _ in range(2 if cell == 'lstm' else 1))
    dones = torch.zeros(S, T, dtype=torch.uint8)
    dones[1, 2] = dones[4, 0] = dones[4, 3] = 1                 # inside two sequences: mid-sequence, first and last step
    d_heads = torch.randn(ROWS, 4, generator=g).to(DEV)
    step_x = torch.randn(2, S, OBS, generator=g).to(DEV)        # two rollout steps
    return x, states, dones.reshape(-1).to(DEV), d_heads, step_x


class _SpelledOut:
    """The launches of RecurrentChainNet (no layer norm, plain head mode, no normaliser) written out, on buffers of this
    object's own, in the engine's order."""

    def __init__(self, cell, net, heads, arena):
        from rl_games_amd import ops
        from rl_games_amd.chain_net import head_span
        self.cell, self.rnn, self.lin = cell, net['rnn'], net['trunk'][0]
        rnn, H = self.rnn, net['rnn'].hidden_size
        self.H, self.G = H, (4 if cell == 'lstm' else 3) * H
        self.head_w, self.head_w_grad, self.head_b, self.head_b_grad, C = head_span(heads, arena)
        assert C == 4
        self.bias = torch.empty(self.G, device=DEV) if cell == 'lstm' else rnn.bias_ih_l0
        self.chain = ops.MlpChain([(self.lin.weight, self.lin.bias, 'elu'), (rnn.weight_ih_l0, self.bias, 'None')], DEV,
                                  weights_version=arena.weights_token)
        self.head_mfma = ops.mlp_rowgemm_supported(H, H) and self.head_w.data_ptr() % 16 == 0

    @torch.no_grad()
    def forward(self, x, states, dones, seq_len, keep):
        from rl_games_amd import ops
        rows, H, rnn = x.shape[0], self.H, self.rnn
        new = lambda *shape: torch.full(shape, float('nan'), device=DEV)
        if self.cell == 'lstm':
            torch.add(rnn.bias_ih_l0, rnn.bias_hh_l0, out=self.bias)
        gates, out, heads = new(rows, self.G), new(rows, H), new(rows, 4)
        act = new(rows, TRUNK) if keep else None
        self.chain.forward(x, gates, act_out=[act] if keep else None, rms=None, eps=1e-5, xn_out=None)
        kept = [new(rows, H), new(rows, H)] if keep else [None, None]          # c_all | hn_all, hprev
        finals = [None if keep else new(rows // seq_len, H) for _ in states]
        if self.cell == 'lstm':
            ops.lstm_seq_forward(gates, rnn.weight_hh_l0, states[0][0], states[1][0], dones, out, kept[0], kept[1],
                                 finals[0], finals[1], seq_len=seq_len)
        else:
            ops.gru_seq_forward(gates, rnn.weight_hh_l0, rnn.bias_hh_l0, states[0][0], dones, out, kept[0], kept[1],
                                finals[0], seq_len=seq_len)
        if self.head_mfma:
            ops.mlp_linear_act_forward(out, self.head_w, self.head_b, heads, act_kind=0)
        else:
            torch.addmm(self.head_b, out, self.head_w.t(), out=heads)
        self.kept = dict(x=x, c0=states[-1][0], dones=dones, T=seq_len, gates=gates, out=out, act=act, kept=kept)
        return heads, finals

    @torch.no_grad()
    def backward(self, d_heads):
        from rl_games_amd import ops
        from rl_games_amd.chain_net import WeightGrads
        k, rnn, G, H = self.kept, self.rnn, self.G, self.H
        rows = d_heads.shape[0]
        new = lambda *shape: torch.full(shape, float('nan'), device=DEV)
        d_out = new(rows, H)
        ops.narrow_dx(d_heads, self.head_w, d_out)              # (4 columns: the narrow kernel)
        nbg = ops.act_bwd_blocks(rows, G)
        gpart = torch.empty(nbg * G, dtype=torch.float64, device=DEV)
        if self.cell == 'lstm':
            dg = dgh = new(rows, G)
            ops.lstm_seq_backward(k['gates'], k['kept'][0], k['c0'], k['dones'], rnn.weight_hh_l0, d_out, dg, k['T'])
            ops.act_bwd_colsum(dg, None, dg, 0, gpart, nbg)
            gpart_h = gpart
        else:
            dg, dgh = new(rows, G), new(rows, G)
            ops.gru_seq_backward(k['gates'], k['kept'][0], k['kept'][1], k['dones'], rnn.weight_hh_l0, d_out, dg, dgh,
                                 k['T'])
            gpart_h = torch.empty_like(gpart)
            ops.act_bwd_colsum(dg, None, dg, 0, gpart, nbg)
            ops.act_bwd_colsum(dgh, None, dgh, 0, gpart_h, nbg)
        nblk = self.chain.num_blocks(rows, 1)
        dz = new(rows, TRUNK)
        part = torch.empty(nblk * TRUNK, dtype=torch.float64, device=DEV)
        self.chain.backward(dg, [k['act']], [dz], [part])
        torch.sum(d_heads, dim=0, out=self.head_b_grad)
        jobs = [(d_heads, k['out'], self.head_w_grad), (dgh, k['kept'][1], rnn.weight_hh_l0.grad),
                (dg, k['act'], rnn.weight_ih_l0.grad), (dz, k['x'], self.lin.weight.grad)]
        colsums = [(gpart, nbg, G, rnn.bias_ih_l0.grad), (gpart_h, nbg, G, rnn.bias_hh_l0.grad),
                   (part, nblk, TRUNK, self.lin.bias.grad)]
        # (the finisher both engines share: one MFMA launch whose finalise takes the column sums)
        finisher = WeightGrads()
        finisher.finish(jobs, rows, colsums)
        return finisher.last_dw_path


def _fp64(cell, net, x, states, dones, d_heads):
    """The same network on the CPU in fp64, step by step with the reference's done resets
    (rl_games/common/layers/recurrent.py:26-58), gradients by autograd.  Returns heads and gradients by parameter name."""
    ref = copy.deepcopy(net).cpu().double()
    for p in ref.parameters():
        p.grad = None
    feat = ref['trunk'](x.cpu().double()).reshape(S, T, -1).transpose(0, 1)
    keep = (1.0 - dones.cpu().double()).reshape(S, T).t().reshape(T, 1, S, 1)
    st = tuple(s.cpu().double() for s in states)
    outs = []
    for t in range(T):
        st = tuple(s * keep[t] for s in st)
        o, st = ref['rnn'](feat[t:t + 1], st if cell == 'lstm' else st[0])
        st = st if cell == 'lstm' else (st,)
        outs.append(o)
    out = torch.cat(outs, 0).transpose(0, 1).reshape(ROWS, -1)
    heads = torch.cat([ref['value'](out), ref['logits'](out)], 1)
    heads.backward(d_heads.cpu().double())
    return heads.detach(), {n: p.grad for n, p in ref.named_parameters()}


@pytest.mark.parametrize('cell,H', [('lstm', 16), ('gru', 16), ('lstm', 128), ('gru', 128)])
def test_recurrent_chain_net_is_its_launches_spelled_out_and_matches_fp64_autograd(cell, H):
    from rl_games_amd.chain_net import RecurrentChainNet
    net, heads, arena = _network(cell, H)
    x, states, dones, d_heads, step_x = _inputs(cell, H)
    eng = RecurrentChainNet(net['trunk'], net['rnn'], None, heads, arena, ROWS, infer_rows=S)
    assert (eng.lstm is net['rnn'], eng.gru is net['rnn']) == (cell == 'lstm', cell == 'gru')
    ref_net, ref_heads_mods, ref_arena = _network(cell, H)     # the same seed: the same weights, in an arena of its own
    assert torch.equal(ref_arena.flat_params, arena.flat_params)
    spelled = _SpelledOut(cell, ref_net, ref_heads_mods, ref_arena)

    # training forward + backward
    for t in eng.stations._state_buf[0] + eng.stations._state_buf[1]:
        t.fill_(7.0)
    got_heads = eng.forward(x, None, 1e-5, states, dones, T, keep=True)
    assert eng.last_states is None
    eng.d_heads[:ROWS].copy_(d_heads)
    arena.flat_grads.fill_(float('nan'))
    eng.backward()
    want_heads, _ = spelled.forward(x, states, dones, T, keep=True)
    ref_arena.flat_grads.fill_(float('nan'))
    assert spelled.backward(d_heads) == eng.last_dw_path == 'mfma'
    torch.cuda.synchronize()
    assert torch.equal(got_heads, want_heads)
    assert torch.isfinite(arena.grads).all()                    # every gradient of the arena was written
    assert torch.equal(arena.grads, ref_arena.grads)
    assert all(bool((t == 7.0).all()) for pair in eng.stations._state_buf for t in pair)    # the live states: untouched

    # ... and the fp64 network with autograd, at the engine-vs-autograd tolerance of the agents' tests
    heads64, grads64 = _fp64(cell, net, x, states, dones, d_heads)
    scale = heads64.abs().max().item()
    print('heads max |diff|', (got_heads.cpu().double() - heads64).abs().max().item(), 'scale', scale)
    assert torch.allclose(got_heads.cpu().double(), heads64, rtol=1e-4, atol=5e-6 * scale)
    for n, p in net.named_parameters():
        want = grads64[n]
        scale = want.abs().max().item() + 1e-12
        print(n, 'max |diff|', (p.grad.cpu().double() - want).abs().max().item(), 'scale', scale)
        assert torch.allclose(p.grad.cpu().double(), want, rtol=1e-4, atol=5e-6 * scale), n

    # two rollout steps on the same weights, the first one's final states fed back in
    st_eng, st_ref = states, states
    for k in range(2):
        got = eng.forward(step_x[k], None, 1e-5, st_eng, None, 1, keep=False)
        want, finals = spelled.forward(step_x[k], st_ref, None, 1, keep=False)
        torch.cuda.synchronize()
        assert torch.equal(got, want), k
        st_eng, st_ref = eng.last_states, tuple(f.unsqueeze(0) for f in finals)
        assert len(st_eng) == len(st_ref)
        for a, b in zip(st_eng, st_ref):
            assert a.shape == (1, S, H) and torch.equal(a, b), k


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_manual_mlp_recurrent_per_layer_trunk_equals_the_fused_trunk(cell):
    """ManualMLP behind a recurrent policy with `fused_mlp: False` - per-layer library products in front of the RNN
    stations, the path no other test runs - against the fused `chain_rnn` trunk: same weights, same minibatch through
    train_actor_critic, at the tolerances of test_mlp_chain_gpu.py::test_engine_fused_chain_equals_per_layer_engine."""
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    make = configs.pendulum_lstm_4096 if cell == 'lstm' else configs.pendulum_gru_4096
    agents = []
    for fused in (True, False):
        torch.manual_seed(11)
        kw = {} if fused else {'fused_mlp': False}
        agents.append(A2CAgent(cell, make(num_actors=64, minibatch_size=256, hip_graphs=False, learning_rate=0, **kw)))
    a1, a2 = agents
    assert (a1._engine.chain_rnn is not None, a2._engine.chain_rnn is None) == (True, True)
    assert getattr(a1._engine, cell) is not None and getattr(a2._engine, cell) is not None
    a2.model.load_state_dict(a1.model.state_dict())
    a1.init_tensors()
    a2.init_tensors()
    a1.obs = a1.env_reset()
    a1.set_eval()
    with torch.no_grad():
        batch = a1.play_steps_rnn()
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    outs = []
    for ag in (a1, a2):
        b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'}
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset(b)
        ag.train_actor_critic(ag.dataset[1])
        torch.cuda.synchronize()
        mb = ag.minibatch_size
        outs.append((ag._engine.heads[:mb].clone(),
                     {n: p.grad.detach().clone() for n, p in ag.model.a2c_network.named_parameters()}))
    (heads, grads), (heads_pl, grads_pl) = outs
    print('heads max |diff|', (heads - heads_pl).abs().max().item())
    assert torch.allclose(heads, heads_pl, rtol=2e-5, atol=2e-6)
    assert set(grads) == set(grads_pl)
    for n, gref in grads_pl.items():
        assert torch.isfinite(gref).all(), n
        scale = max(1.0, gref.abs().max().item())
        print(n, 'max |diff|', (grads[n] - gref).abs().max().item(), 'scale', gref.abs().max().item())
        assert torch.allclose(grads[n], gref, rtol=1e-4, atol=1e-5 * scale), n
