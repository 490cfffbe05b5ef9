"""CPU: chain_net.RnnStations - the LSTM / GRU stations RecurrentChainNet and mlp_engine.ManualMLP share - and
chain_net.trunk_jobs, the one statement of a trunk's weight-gradient list, with every launch replaced by a recorder:
which buffers go into the sequence kernels' argument tuples, where the final states land, what the bias sum and the
gate-gradient column sums launch, and which jobs come out.  No kernel runs.
"""
import types

import pytest
import torch
from torch import nn

from test_weight_grads_cpu import ROWS, _Plan, _colsum, _is, _job, rec  # noqa: F401  (rec: that file's recorder fixture)

H, S, T, IN = 16, 3, 4, 8
CELLS = ('lstm', 'gru')


@pytest.fixture
def launches(monkeypatch):
    from rl_games_amd import ops
    calls = types.SimpleNamespace(add=[], colsum=[])
    real_add = torch.add

    def add(a, b, out=None):
        calls.add.append((a, b, out))
        return real_add(a, b, out=out)
    monkeypatch.setattr(ops, 'lstm_supported', lambda h: h in (16, 32, 64, 128))
    monkeypatch.setattr(ops, 'gru_supported', lambda h: h in (16, 32, 64, 128))
    monkeypatch.setattr(ops, 'act_bwd_blocks', lambda rows, cols: (rows + 7) // 8)
    monkeypatch.setattr(ops, 'act_bwd_colsum', lambda d_out, pre, d_pre, kind, part, nb:
                        calls.colsum.append((d_out, pre, d_pre, kind, part, nb)))
    monkeypatch.setattr(torch, 'add', add)
    return calls


def _stations(cell, rows=S * T):
    from rl_games_amd.chain_net import RnnStations
    rnn = (nn.LSTM if cell == 'lstm' else nn.GRU)(IN, H)
    for p in rnn.parameters():
        p.grad = torch.zeros_like(p)
    return RnnStations(rnn, rows, torch.device('cpu'))


def _states(cell, seqs=S):
    return tuple(torch.randn(1, seqs, H) for _ in range(2 if cell == 'lstm' else 1))


def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


@pytest.mark.parametrize('cell', CELLS)
def test_a_kept_forward_hands_the_kernel_the_stations_own_buffers_and_leaves_the_states_alone(launches, cell):
    st = _stations(cell, rows=S * T + 4)                        # (buffers larger than the forward: row views)
    assert (st.lstm is st.rnn, st.gru is st.rnn) == (cell == 'lstm', cell == 'gru')
    assert st.Hr == H and st.Gr == (4 if cell == 'lstm' else 3) * H
    for pair in st._state_buf:
        for t in pair:
            t.fill_(7.0)
    states = _states(cell)
    dones = torch.zeros(S * T, dtype=torch.uint8)
    rows = S * T
    args = st.forward_args(rows, states, dones, T, keep=True)
    w_hh = st.rnn.weight_hh_l0
    if cell == 'lstm':
        gates, w, h0, c0, d, out, c_all, hprev, hT, cT = args
        assert _same_view(c0, states[1][0]) and _same_view(c_all, st.c_all[:rows]) and cT is None
    else:
        gates, w, b_hh, h0, d, out, hn_all, hprev, hT = args
        assert b_hh is st.rnn.bias_hh_l0 and _same_view(hn_all, st.hn_all[:rows])
    assert w is w_hh and _same_view(d, dones) and _same_view(h0, states[0][0])
    assert _same_view(gates, st.gates[:rows]) and _same_view(out, st.rnn_out[:rows])
    assert _same_view(hprev, st.hprev[:rows]) and hT is None
    assert st.last_states is None and st.seq_length == T
    assert all(bool((t == 7.0).all()) for pair in st._state_buf for t in pair)
    assert st.gates.shape == (rows + 4, st.Gr) and st.rnn_out.shape == st.d_rnn_out.shape == (rows + 4, H)


@pytest.mark.parametrize('cell', CELLS)
def test_an_inference_forward_keeps_nothing_and_ping_pongs_the_final_states(launches, cell):
    st = _stations(cell)
    n = 2 if cell == 'lstm' else 1

    def step(states, seqs=S):
        args = st.forward_args(seqs, states, None, 1, keep=False)
        kept, finals = args[6:8], args[8:]                      # (c_all | hn_all, hprev), (hT[, cT])
        assert kept == (None, None) and len(finals) == n and args[4] is None
        assert len(st.last_states) == n
        for last, final in zip(st.last_states, finals):
            assert last.shape == (1, seqs, H) and _same_view(last[0], final)
        return st.last_states

    def pair_of(states):
        return [k for k in (0, 1) if all(s.data_ptr() == b.data_ptr() for s, b in zip(states, st._state_buf[k]))]

    first = step(_states(cell))                                 # foreign inputs: pair 0
    assert pair_of(first) == [0]
    second = step(first)                                        # pair 0's views in: pair 1
    assert pair_of(second) == [1]
    assert pair_of(step(second)) == [0]                         # ... and back again
    fewer = step(_states(cell, 2), seqs=2)                      # fewer sequences than the buffers hold
    assert pair_of(fewer) == [0] and fewer[0].shape == (1, 2, H)


def test_lstm_sums_its_biases_once_per_forward_and_both_bias_gradients_share_one_column_sum(launches):
    st = _stations('lstm')
    assert st.gate_bias is st.bias_sum and st.bias_sum.shape == (4 * H,)
    rnn, rows = st.rnn, S * T
    st.forward_args(rows, _states('lstm'), None, T, keep=True)
    assert len(launches.add) == 1
    a, b, out = launches.add[0]
    assert a is rnn.bias_ih_l0 and b is rnn.bias_hh_l0 and out is st.bias_sum
    assert torch.equal(st.bias_sum, rnn.bias_ih_l0 + rnn.bias_hh_l0)
    st.forward_args(S, _states('lstm'), None, 1, keep=False)
    assert len(launches.add) == 2
    d_out = st.d_rnn_out[:rows]
    gates, c_all, c0, dones, w_hh, d, d_gates = st.backward_args(d_out)          # (the kept forward's, not the step's)
    assert _same_view(gates, st.gates[:rows]) and _same_view(c_all, st.c_all[:rows]) and dones is None
    assert w_hh is rnn.weight_hh_l0 and d is d_out and _same_view(d_gates, st.d_gates[:rows]) and c0.shape == (S, H)
    rnn_in = torch.randn(rows, IN)
    dg, jobs, colsums = st.gate_gradients(rnn_in)
    assert _same_view(dg, st.d_gates[:rows])
    assert len(launches.colsum) == 1
    d_in, pre, d_pre, kind, part, nb = launches.colsum[0]
    assert d_in is dg and d_pre is dg and pre is None and kind == 0 and nb == (rows + 7) // 8
    assert _same_view(part, st.gate_partials[:nb * 4 * H])
    assert colsums[0][3] is rnn.bias_ih_l0.grad and colsums[1][3] is rnn.bias_hh_l0.grad
    assert colsums[0][0] is part and colsums[1][0] is part                       # d b_hh = d b_ih
    assert all(c[1:3] == (nb, 4 * H) for c in colsums)
    assert jobs[0][0] is dg and _same_view(jobs[0][1], st.hprev[:rows]) and jobs[0][2] is rnn.weight_hh_l0.grad
    assert _is(jobs[1], (dg, rnn_in, rnn.weight_ih_l0.grad)) and len(jobs) == 2


def test_gru_takes_b_ih_as_the_gate_bias_and_sums_the_two_gate_gradients_apart(launches):
    st = _stations('gru')
    rnn, rows = st.rnn, S * T
    assert st.gate_bias is rnn.bias_ih_l0 and st.bias_sum is None
    dones = torch.zeros(rows, dtype=torch.uint8)
    st.forward_args(rows, _states('gru'), dones, T, keep=True)
    st.forward_args(S, _states('gru'), None, 1, keep=False)
    assert launches.add == []
    d_out = st.d_rnn_out[:rows]
    gates, hn_all, hprev, d, w_hh, d_o, d_gx, d_gh = st.backward_args(d_out)
    assert _same_view(gates, st.gates[:rows]) and _same_view(hn_all, st.hn_all[:rows]) and _same_view(d, dones)
    assert _same_view(hprev, st.hprev[:rows]) and w_hh is rnn.weight_hh_l0 and d_o is d_out
    assert _same_view(d_gx, st.d_gx[:rows]) and _same_view(d_gh, st.d_gh[:rows])
    rnn_in = torch.randn(rows, IN)
    dg, jobs, colsums = st.gate_gradients(rnn_in)
    dgh = jobs[0][0]
    assert dg is not dgh and _same_view(dg, st.d_gx[:rows]) and _same_view(dgh, st.d_gh[:rows])
    assert len(launches.colsum) == 2
    (a_in, _, a_out, a_kind, a_part, nb), (b_in, _, b_out, b_kind, b_part, nb_h) = launches.colsum
    assert a_in is dg and a_out is dg and b_in is dgh and b_out is dgh and a_kind == b_kind == 0
    assert nb == nb_h == (rows + 7) // 8
    assert a_part.data_ptr() != b_part.data_ptr()
    assert _same_view(a_part, st.gate_partials[:nb * 3 * H]) and _same_view(b_part, st.gate_partials_h[:nb * 3 * H])
    assert colsums[0][0] is a_part and colsums[0][3] is rnn.bias_ih_l0.grad
    assert colsums[1][0] is b_part and colsums[1][3] is rnn.bias_hh_l0.grad
    assert _same_view(jobs[0][1], st.hprev[:rows]) and jobs[0][2] is rnn.weight_hh_l0.grad
    assert _is(jobs[1], (dg, rnn_in, rnn.weight_ih_l0.grad)) and len(jobs) == 2


@pytest.mark.parametrize('cell', CELLS)
def test_done_flags_reach_the_kernel_as_contiguous_uint8(launches, cell):
    st = _stations(cell)
    flags = torch.tensor([0., 1.] * (S * T // 2)).view(S, T)
    d = st.forward_args(S * T, _states(cell), flags, T, keep=True)[4]
    assert d.dtype == torch.uint8 and d.is_contiguous() and d.shape == (S * T,)
    assert torch.equal(d, flags.reshape(-1).to(torch.uint8))


@pytest.mark.parametrize('cell', CELLS)
def test_rows_and_states_that_do_not_fit_are_value_errors(launches, cell):
    st = _stations(cell)
    with pytest.raises(ValueError, match='multiple of seq_length'):
        st.forward_args(S * T - 1, _states(cell), None, T, keep=True)
    with pytest.raises(ValueError, match='rnn_states'):
        st.forward_args(S * T, _states(cell, S + 1), None, T, keep=True)            # one sequence too many
    with pytest.raises(ValueError, match='rnn_states'):
        st.forward_args(S * T, tuple(torch.randn(1, S, H + 1) for _ in range(2)), None, T, keep=True)
    strided = tuple(torch.randn(1, H, S).transpose(1, 2) for _ in range(2))
    assert strided[0].shape == (1, S, H) and not strided[0][0].is_contiguous()
    with pytest.raises(ValueError, match='rnn_states'):
        st.forward_args(S * T, strided, None, T, keep=True)
    if cell == 'lstm':
        with pytest.raises(ValueError, match='rnn_states'):
            st.forward_args(S * T, (torch.randn(1, S, H), strided[1]), None, T, keep=True)
    assert launches.add == [] and st.last_states is None


def test_cells_outside_the_kernels_are_declined(launches):
    from rl_games_amd.chain_net import RnnStations
    cpu = torch.device('cpu')
    for rnn in (nn.RNN(IN, H), nn.LSTM(IN, H, num_layers=2), nn.GRU(IN, 48), nn.LSTM(IN, H, bidirectional=True),
                nn.GRU(IN, H, bias=False), nn.LSTM(IN, 32, proj_size=16)):
        with pytest.raises(NotImplementedError):
            RnnStations(rnn, 8, cpu)


def _trunk(widths, x_cols):
    linears, cols = [], x_cols
    for w in widths:
        lin = nn.Linear(cols, w)
        lin.weight.grad, lin.bias.grad = torch.full_like(lin.weight, float('nan')), torch.empty_like(lin.bias)
        linears.append(lin)
        cols = w
    return linears


def test_trunk_jobs_lists_the_last_layer_first_with_x_under_layer_0_and_every_layer_index():
    from rl_games_amd.chain_net import trunk_jobs, trunk_views
    linears = _trunk([32, 64], 12)
    buffers = dict(acts=[torch.randn(ROWS + 8, 32), torch.randn(ROWS + 8, 64)],
                   dzs=[torch.randn(ROWS + 8, 32), torch.randn(ROWS + 8, 64)],
                   partials=[torch.zeros(7 * 32, dtype=torch.float64), torch.zeros(7 * 64, dtype=torch.float64)])
    nblk = 6
    acts, dzs, parts = trunk_views(linears, buffers['acts'], buffers['dzs'], buffers['partials'], ROWS, nblk)
    for views, full in ((acts, buffers['acts']), (dzs, buffers['dzs'])):
        assert all(_same_view(v, f[:ROWS]) for v, f in zip(views, full))
    assert [p.shape for p in parts] == [(nblk * 32,), (nblk * 64,)]
    assert all(p.data_ptr() == f.data_ptr() for p, f in zip(parts, buffers['partials']))
    x = torch.randn(ROWS, 12)
    jobs, colsums = trunk_jobs(linears, x, acts, dzs, parts, nblk)
    assert _is(jobs[0], (dzs[1], acts[0], linears[1].weight.grad, 1))
    assert _is(jobs[1], (dzs[0], x, linears[0].weight.grad, 0)) and len(jobs) == 2
    assert _is(colsums[0], (parts[1], nblk, 64, linears[1].bias.grad))
    assert _is(colsums[1], (parts[0], nblk, 32, linears[0].bias.grad)) and len(colsums) == 2


def test_finish_without_maxima_takes_jobs_with_a_layer_index_exactly_as_it_takes_triples(rec):  # noqa: F811
    from rl_games_amd.chain_net import WeightGrads
    triples = [_job(4, 32), _job(32, 64), _job(64, 12), _job(64, 9)]
    indexed = [t + (k,) for k, t in enumerate(triples)]
    colsums = [_colsum(32), _colsum(64)]
    seen = []
    for jobs in (triples, indexed, [indexed[0]] + triples[1:]):            # (and a mixed list: a recurrent engine's)
        _Plan.built.clear(), rec.mm.clear()
        wg = WeightGrads()
        assert wg.finish(jobs, ROWS, colsums, maxima=None) is None
        launched, plan, mx = wg.last_dw_jobs
        launch = plan.launches[0]
        assert mx is None and launch.maxima is None and all(len(j) == 3 for j in launch.jobs)
        assert [_is(got, want) for got, want in zip(launch.jobs, (triples[1], triples[2], triples[0]))] == [True] * 3
        assert _is([c[3] for c in launch.colsums], [c[3] for c in colsums])
        assert _is(rec.mm, [triples[3][2]]) and wg.last_dw_library_jobs == 1 and wg.last_dw_path == 'mfma'
        seen.append(list(_Plan.built))
    assert seen[0] == seen[1] == seen[2] == [([(32, 64), (64, 12), (4, 32)], ROWS)]
