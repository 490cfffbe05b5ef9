"""CPU: the GRU configuration (configs.pendulum_gru_4096), the boundary of the GRU kernels' wrappers, and the maths
the kernels implement (csrc/gru.hip, csrc/gru_wide.hip) stated in plain fp64 torch and held against autograd."""

import pytest
import torch


def _same(a, b):
    """Deep equality that also tells 2 from 2.0 and a list from a tuple."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_gru_config_differs_from_config5_in_the_cell_name_only():
    from rl_games_amd import configs
    want = configs.pendulum_lstm_4096()
    want['network']['rnn']['name'] = 'gru'
    assert _same(configs.pendulum_gru_4096(), want)
    assert configs.pendulum_gru_4096()['network']['rnn'] == {'name': 'gru', 'units': 64, 'layers': 1}
    wide = configs.pendulum_lstm_4096(units=128)
    wide['network']['rnn']['name'] = 'gru'
    assert _same(configs.pendulum_gru_4096(units=128), wide)


def test_gru_config_units_reach_the_network_section_only():
    from rl_games_amd import configs
    small = configs.pendulum_gru_4096(num_actors=128, units=128, minibatch_size=1024)
    assert small['network']['rnn']['units'] == 128
    assert small['config']['num_actors'] == 128 and small['config']['minibatch_size'] == 1024
    assert 'units' not in small['config']
    want = configs.pendulum_lstm_4096(num_actors=128, units=128, minibatch_size=1024)
    want['network']['rnn']['name'] = 'gru'
    assert _same(small, want)


@pytest.mark.parametrize('H', [64, 128])
def test_gru_ops_reject_cpu_tensors(H):
    from rl_games_amd import ops
    from rl_games_amd._lib import HipLibraryError
    S, T = 4, 2
    gates = torch.zeros(S * T, 3 * H)
    w_hh = torch.zeros(3 * H, H)
    b_hh = torch.zeros(3 * H)
    state = torch.zeros(S, H)
    rows = torch.zeros(S * T, H)
    with pytest.raises(HipLibraryError):
        ops.gru_seq_forward(gates, w_hh, b_hh, state, None, rows, seq_len=T)
    with pytest.raises(HipLibraryError):
        ops.gru_seq_backward(gates, rows, rows, None, w_hh, rows, torch.zeros(S * T, 3 * H), torch.zeros(S * T, 3 * H), T)


def test_gru_ops_reject_rows_that_are_no_multiple_of_seq_len():
    from rl_games_amd import ops
    H = 16
    gates = torch.zeros(7, 3 * H)
    w_hh = torch.zeros(3 * H, H)
    b_hh = torch.zeros(3 * H)
    rows = torch.zeros(7, H)
    with pytest.raises(ValueError, match='multiple of seq_len'):
        ops.gru_seq_forward(gates, w_hh, b_hh, torch.zeros(3, H), None, rows, seq_len=2)
    with pytest.raises(ValueError, match='multiple of seq_len'):
        ops.gru_seq_backward(gates, rows, rows, None, w_hh, rows, torch.zeros(7, 3 * H), torch.zeros(7, 3 * H), 2)


# ---- the maths of the kernels ---------------------------------------------------------------------------------------

def _gru_forward(gx, w_hh, b_hh, h0, dones, T):
    """gx [S*T, 3H] = x W_ih^T + b_ih, rows (seq, t).  Returns the activated gates (r, z, n) [S*T, 3H], out, hn_all
    (W_hn h + b_hn) and hprev (the state entering each step after the reset), each [S*T, H]."""
    S, H = h0.shape
    gx = gx.reshape(S, T, 3 * H)
    h = h0
    gates, out, hn_all, hprev = [], [], [], []
    for t in range(T):
        if dones is not None:
            h = h * (1.0 - dones.reshape(S, T)[:, t].to(h.dtype)).unsqueeze(1)
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, t, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = torch.tanh(gx[:, t, 2 * H:] + r * hn)
        hprev.append(h)
        h = (1.0 - z) * n + z * h
        gates.append(torch.cat([r, z, n], 1))
        out.append(h)
        hn_all.append(hn)

    def rows(parts):
        return torch.stack(parts, 1).reshape(S * T, -1)
    return rows(gates), rows(out), rows(hn_all), rows(hprev)


def _gru_backward(gates, hn_all, hprev, dones, w_hh, d_out, T):
    """The backward of the kernels: d_gx = (dr_pre, dz_pre, dn_pre), d_gh = (dr_pre, dz_pre, dn_pre * r)."""
    B, H = d_out.shape
    S = B // T
    g = gates.reshape(S, T, 3 * H)
    hn_all, hprev, d_out = hn_all.reshape(S, T, H), hprev.reshape(S, T, H), d_out.reshape(S, T, H)
    d_gx = torch.zeros(S, T, 3 * H, dtype=d_out.dtype)
    d_gh = torch.zeros(S, T, 3 * H, dtype=d_out.dtype)
    dh_next = torch.zeros(S, H, dtype=d_out.dtype)
    for t in range(T - 1, -1, -1):
        r, z, n = g[:, t, :H], g[:, t, H:2 * H], g[:, t, 2 * H:]
        dh = d_out[:, t] + dh_next
        dn = dh * (1.0 - z) * (1.0 - n * n)
        dz = dh * (hprev[:, t] - n) * z * (1.0 - z)
        dr = dn * hn_all[:, t] * r * (1.0 - r)
        d_gx[:, t] = torch.cat([dr, dz, dn], 1)
        d_gh[:, t] = torch.cat([dr, dz, dn * r], 1)
        dh_next = dh * z + d_gh[:, t] @ w_hh
        if dones is not None:
            dh_next = dh_next * (1.0 - dones.reshape(S, T)[:, t].to(dh.dtype)).unsqueeze(1)
    return d_gx.reshape(B, 3 * H), d_gh.reshape(B, 3 * H)


def test_gru_backward_formulas_equal_autograd_through_torch_gru():
    """S = 5, T = 4, H = 16, 20 % dones, fp64: the formulas above against autograd through torch.nn.GRU stepped with
    done resets - d_gx, d_gh and the derived dx, dW_ih, dW_hh, db_ih, db_hh to 1e-12 relative."""
    S, T, H, I = 5, 4, 16, 7
    g = torch.Generator().manual_seed(3)
    gru = torch.nn.GRU(I, H, 1).double()
    x = torch.randn(S * T, I, generator=g, dtype=torch.float64).requires_grad_(True)
    h0 = 0.5 * torch.randn(S, H, generator=g, dtype=torch.float64)
    dones = (torch.rand(S * T, generator=g) < 0.2).to(torch.uint8)
    assert 0 < int(dones.sum()) < S * T
    d_out = torch.randn(S * T, H, generator=g, dtype=torch.float64)

    # autograd: torch.nn.GRU one step at a time
    xs = x.reshape(S, T, I).transpose(0, 1)
    d = dones.reshape(S, T).t()
    st = h0.unsqueeze(0)
    outs = []
    for t in range(T):
        st = st * (1.0 - d[t].double()).reshape(1, -1, 1)
        o, st = gru(xs[t:t + 1], st)
        outs.append(o)
    ref_out = torch.cat(outs, 0).transpose(0, 1).reshape(S * T, H)
    ref_out.backward(d_out)
    ref = {k: getattr(gru, k).grad.clone() for k in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')}
    ref_dx = x.grad.clone()

    with torch.no_grad():
        w_ih, w_hh = gru.weight_ih_l0.detach(), gru.weight_hh_l0.detach()
        xd = x.detach()
        gx = xd @ w_ih.t() + gru.bias_ih_l0.detach()
        gates, out, hn_all, hprev = _gru_forward(gx, w_hh, gru.bias_hh_l0.detach(), h0, dones, T)
        d_gx, d_gh = _gru_backward(gates, hn_all, hprev, dones, w_hh, d_out, T)

    def close(a, b, name):
        err = (a - b).abs().max().item()
        scale = b.abs().max().item()
        assert err <= 1e-12 * scale, (name, err, scale)
    close(out, ref_out.detach(), 'out')
    close(d_gx @ w_ih, ref_dx, 'dx')
    close(d_gx.t() @ xd, ref['weight_ih_l0'], 'dW_ih')
    close(d_gh.t() @ hprev, ref['weight_hh_l0'], 'dW_hh')
    close(d_gx.sum(0), ref['bias_ih_l0'], 'db_ih')
    close(d_gh.sum(0), ref['bias_hh_l0'], 'db_hh')

    # d_gx and d_gh themselves: autograd with respect to per-row offsets of the two pre-activation sides
    off_x = torch.zeros(S * T, 3 * H, dtype=torch.float64, requires_grad=True)
    off_h = torch.zeros(S * T, 3 * H, dtype=torch.float64, requires_grad=True)
    h = h0
    outs = []
    ox, oh = off_x.reshape(S, T, 3 * H), off_h.reshape(S, T, 3 * H)
    gxr = gx.reshape(S, T, 3 * H)
    for t in range(T):
        h = h * (1.0 - dones.reshape(S, T)[:, t].double()).unsqueeze(1)
        a = gxr[:, t] + ox[:, t]
        b = h @ w_hh.t() + gru.bias_hh_l0.detach() + oh[:, t]
        r = torch.sigmoid(a[:, :H] + b[:, :H])
        z = torch.sigmoid(a[:, H:2 * H] + b[:, H:2 * H])
        n = torch.tanh(a[:, 2 * H:] + r * b[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        outs.append(h)
    torch.stack(outs, 1).reshape(S * T, H).backward(d_out)
    close(d_gx, off_x.grad, 'd_gx')
    close(d_gh, off_h.grad, 'd_gh')
