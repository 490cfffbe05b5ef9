"""GPU: the sequence-persistent LSTM kernels with W_hh in LDS (csrc/lstm.hip: 16 / 32 / 64 units) against a CPU
evaluation in fp64 of torch.nn.LSTM run step by step with the reference's done-reset semantics
(rl_games/common/layers/recurrent.py:26-58; host mirror policy.RnnWithDones), forward and - through autograd on the CPU
side - backward.  The reference is independent of any GPU library.

Tolerance: the kernels are fp32, the reference exact to fp32 resolution: rtol 1e-5 north_star tolerance on O(1)
activations plus an absolute term for values near zero; gradients are compared relative to the tensor scale - the
bounds of tests/test_lstm_wide_gpu.py.  Every width is taken through every tile the launcher can pick for it
(lstm_seq_per_block: 16 sequences per workgroup from S > 4,080, 8 from S > 2,040, 4 below; never fewer than 256 / H),
so the one-, two- and four-sequences-per-thread instantiations are all held to the same fp64 reference, and their rows
to the bits of the one-sequence-per-thread launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = [16, 32, 64]


def _reference(x, lstm, h0, c0, dones, T):
    """x [S*T, I] rows (seq, t).  Returns out [S*T, H], (hT, cT), the cell states [S*T, H] and the states entering
    each step after the reset [S*T, H]."""
    S = x.shape[0] // T
    xs = x.reshape(S, T, -1).transpose(0, 1)
    d = dones.reshape(S, T).t() if dones is not None else None
    st = (h0.unsqueeze(0), c0.unsqueeze(0))
    outs, cells, entering = [], [], []
    for t in range(T):
        if d is not None:
            keep = (1.0 - d[t].float()).reshape(1, -1, 1).to(st[0].dtype)
            st = (st[0] * keep, st[1] * keep)
        entering.append(st[0])
        o, st = lstm(xs[t:t + 1], st)
        outs.append(o)
        cells.append(st[1])

    def rows(parts):
        return torch.cat(parts, 0).transpose(0, 1).reshape(S * T, -1)
    return rows(outs), st, rows(cells), rows(entering)


def _inputs(S, T, I, H, with_dones):
    """Seeded parameters, inputs, initial states, dones and d_out.  A random draw of dones (20 % of the steps; one
    sequence, S // 2, is then cleared - an episode that outlasts the window, which a draw over 16 or 32 steps hardly
    ever holds) must contain a reset at t = 0, one at t = T - 1 and a sequence without any, or the case tests less
    than it says."""
    g = torch.Generator().manual_seed(S * 7 + T)
    lstm32 = torch.nn.LSTM(I, H, 1)
    gw = torch.Generator().manual_seed(S * 7 + T + 1000 * H)
    with torch.no_grad():
        for p in lstm32.parameters():           # torch.nn.LSTM's own initialisation, from a seeded generator
            p.uniform_(-H ** -0.5, H ** -0.5, generator=gw)
    x32 = torch.randn(S * T, I, generator=g)
    h0 = (0.5 * torch.randn(S, H, generator=g)).to(DEV)
    c0 = (0.5 * torch.randn(S, H, generator=g)).to(DEV)
    dones = None
    if with_dones:
        d = (torch.rand(S * T, generator=g) < 0.2).to(torch.uint8).reshape(S, T)
        d[S // 2] = 0
        assert d[:, 0].any() and d[:, T - 1].any() and (d.sum(1) == 0).any() and (d.sum(1) > 0).any()
        dones = d.reshape(S * T).to(DEV)
    d_out = torch.randn(S * T, H, generator=g).to(DEV)
    return lstm32, x32, h0, c0, dones, d_out


def _poison(*shape):
    """An output buffer that starts as NaN: a row the kernel never stores cannot pass on stale memory."""
    return torch.full(shape, float('nan'), device=DEV)


def _no_poison_left(**buffers):
    for name, b in buffers.items():
        assert b is None or not torch.isnan(b).any(), f'NaN left in {name}'


def _forward(ops, lstm32, x, h0, c0, dones, T, train=True, finals=True):
    S, H = h0.shape
    w_ih, w_hh = lstm32.weight_ih_l0.detach().to(DEV), lstm32.weight_hh_l0.detach().to(DEV).contiguous()
    bias = (lstm32.bias_ih_l0 + lstm32.bias_hh_l0).detach().to(DEV)
    gates = torch.addmm(bias, x, w_ih.t())
    out = _poison(S * T, H)
    c_all = _poison(S * T, H) if train else None
    hprev = _poison(S * T, H) if train else None
    hT = _poison(S, H) if finals else None
    cT = _poison(S, H) if finals else None
    ops.lstm_seq_forward(gates, w_hh, h0, c0, dones, out, c_all, hprev, hT, cT, seq_len=T)
    _no_poison_left(gates=gates, out=out, c_all=c_all, hprev=hprev, hT=hT, cT=cT)
    return dict(gates=gates, out=out, c_all=c_all, hprev=hprev, hT=hT, cT=cT, w_ih=w_ih, w_hh=w_hh)


def _backward(ops, r, c0, dones, d_out, T):
    d_gates = _poison(*r['gates'].shape)
    ops.lstm_seq_backward(r['gates'], r['c_all'], c0, dones, r['w_hh'], d_out, d_gates, T)
    _no_poison_left(d_gates=d_gates)
    return d_gates


def _check_against_fp64(S, T, I, with_dones, H, inputs=None, dones=None):
    """One shape against the fp64 CPU LSTM at the bounds of test_wide_lstm_forward_backward_match_fp64: out, h_final,
    c_final, c_all, hprev rtol 1e-5 + 2e-6; hprev the bits of the previous row of out; dx, dW_ih, dW_hh, db within
    2e-5 max|ref| + 1e-7; an inference call and repeats bit-identical.  `dones` replaces the drawn ones.  Returns the
    kernel's forward results and d_gates."""
    from rl_games_amd import ops
    lstm32, x32, h0, c0, drawn, d_out = inputs if inputs is not None else _inputs(S, T, I, H, with_dones)
    dones = drawn if dones is None else dones

    # the reference: CPU, fp64, the fp32 parameters and inputs upcast exactly
    lstm = torch.nn.LSTM(I, H, 1).double()
    lstm.load_state_dict({k: v.double() for k, v in lstm32.state_dict().items()})
    x = x32.double().requires_grad_(True)
    ref_out, (ref_h, ref_c), ref_cells, ref_enter = _reference(x, lstm, h0.cpu().double(), c0.cpu().double(),
                                                               None if dones is None else dones.cpu(), T)
    ref_out.backward(d_out.cpu().double())
    ref_out, ref_h, ref_c = ref_out.detach().float().to(DEV), ref_h.detach().float().to(DEV), ref_c.detach().float().to(DEV)
    ref_cells, ref_enter = ref_cells.detach().float().to(DEV), ref_enter.detach().float().to(DEV)
    ref_grads = {n: getattr(lstm, n).grad.float().to(DEV)
                 for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')}
    x_grad = x.grad.float().to(DEV)
    x = x32.to(DEV)

    r = _forward(ops, lstm32, x, h0, c0, dones, T)
    tol = dict(rtol=1e-5, atol=2e-6)
    for name, got, want in (('out', r['out'], ref_out), ('hT', r['hT'], ref_h[0]), ('cT', r['cT'], ref_c[0]),
                            ('c_all', r['c_all'], ref_cells), ('hprev', r['hprev'], ref_enter)):
        print(name, 'max |diff|', (got - want).abs().max().item())
        assert torch.allclose(got, want, **tol), (name, (got - want).abs().max().item())
    # hprev IS the state entering each step: the previous row of out (h0 at t = 0), zeroed where done - bit for bit
    enter = torch.cat([h0.unsqueeze(1), r['out'].reshape(S, T, H)[:, :-1]], 1).reshape(S * T, H)
    if dones is not None:
        enter = enter * (1.0 - dones.float()).unsqueeze(1)
    assert torch.equal(r['hprev'], enter)

    # an inference call (nothing kept for backward) and a second training call: bit-identical
    inf = _forward(ops, lstm32, x, h0, c0, dones, T, train=False)
    again = _forward(ops, lstm32, x, h0, c0, dones, T)
    for k in ('out', 'hT', 'cT', 'gates'):
        assert torch.equal(inf[k], r[k]), k
    for k in ('out', 'hT', 'cT', 'gates', 'c_all', 'hprev'):
        assert torch.equal(again[k], r[k]), k

    d_gates = _backward(ops, r, c0, dones, d_out, T)
    assert torch.equal(d_gates, _backward(ops, r, c0, dones, d_out, T))
    dx = d_gates @ r['w_ih']
    dw_ih = d_gates.t() @ x
    dw_hh = d_gates.t() @ r['hprev']
    db = d_gates.sum(0)

    def close(a, b, name):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(name, 'max |diff|', err, 'bound', 2e-5 * scale + 1e-7)
        assert err <= 2e-5 * scale + 1e-7, (name, err, scale)
    close(dx, x_grad, 'dx')
    close(dw_ih, ref_grads['weight_ih_l0'], 'dw_ih')
    close(dw_hh, ref_grads['weight_hh_l0'], 'dw_hh')
    close(db, ref_grads['bias_ih_l0'], 'db_ih')
    close(db, ref_grads['bias_hh_l0'], 'db_hh')
    return r, d_gates


FORWARD_KEYS = ('out', 'gates', 'c_all', 'hprev', 'hT', 'cT')


def _same_bits(a, b, da, db, what):
    """Forward results and d_gates of two launches over the same rows."""
    for k in FORWARD_KEYS:
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(da, db), (what, 'd_gates')


def _head(r, n, T):
    """The first n sequences of a launch's forward results."""
    return {k: r[k][:n if k in ('hT', 'cT') else n * T] for k in FORWARD_KEYS}


def _first_sequences_alone(ops, inputs, n, T):
    """Sequences 0 .. n-1 launched on their own (the smallest tile of their width): forward results and d_gates."""
    lstm32, x32, h0, c0, dones, d_out = inputs
    d = None if dones is None else dones[:n * T].contiguous()
    h0, c0 = h0[:n].contiguous(), c0[:n].contiguous()
    part = _forward(ops, lstm32, x32[:n * T].to(DEV), h0, c0, d, T)
    return part, _backward(ops, part, c0, d, d_out[:n * T].contiguous(), T)


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('S,T,I,with_dones', [(64, 16, 64, True), (37, 4, 12, True), (1024, 16, 64, True),
                                            (5, 1, 7, False), (130, 8, 20, False), (256, 32, 100, True)])
def test_lstm_forward_backward_match_fp64(S, T, I, with_dones, H):
    """The shapes and bounds of test_wide_lstm_forward_backward_match_fp64 at every width of csrc/lstm.hip, all in the
    smallest tile of the width (S <= 1,024: 16 / 8 / 4 sequences per workgroup at 16 / 32 / 64 units, one per thread).
    As measured on an MI355X, the largest |diff| over the 18 cases: out 6.2e-7, hT 3.9e-7, cT 5.4e-7, c_all 7.7e-7,
    hprev 6.2e-7, dx 4.8e-7, dW_ih 5.0e-4, dW_hh 8.1e-5, db 2.3e-5 (gradients against bounds of 2e-5 max|ref|)."""
    _check_against_fp64(S, T, I, with_dones, H)


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('S,T', [(4099, 2), (2050, 3)])
def test_lstm_large_tiles_match_fp64_and_small_tiles(S, T, H):
    """lstm_seq_per_block(S, H) of csrc/lstm.hip starts at 16 sequences per workgroup and halves while that leaves
    fewer than 256 workgroups and more than 256 / H sequences (one per thread group):
      S = 4,099: ceil(4099 / 16) = 257 workgroups >= 256 - tile 16 at every width: <64,16> (4 sequences per thread),
                 <32,16> (2), <16,16> (1); last tile ragged, 4099 = 256 * 16 + 3.
      S = 2,050: ceil(2050 / 16) = 129 < 256, ceil(2050 / 8) = 257 - tile 8 at 64 and 32 units: <64,8> (2 per thread),
                 <32,8> (1); 16 units cannot go below 16: <16,16>; last tile ragged, 2050 = 256 * 8 + 2 = 128 * 16 + 2.
    Same bounds as above, and the first five sequences are bit-identical to the same five launched alone (S = 5: the
    smallest tile of the width, <64,4>, <32,8>, <16,16>), forward and backward - the k-loop order of a row does not
    depend on how many sequences a thread carries.
    As measured on an MI355X, the largest |diff| over the 6 cases: out 3.0e-7, hT 1.2e-7, cT 2.4e-7, c_all 4.2e-7,
    hprev 3.0e-7, dx 1.6e-7, dW_ih 7.2e-5, dW_hh 6.8e-5, db 2.3e-5; every bit-identity holds."""
    from rl_games_amd import ops
    I, n = 12, 5
    inputs = _inputs(S, T, I, H, True)
    full, dg_full = _check_against_fp64(S, T, I, True, H, inputs)
    part, dg_part = _first_sequences_alone(ops, inputs, n, T)
    _same_bits(_head(full, n, T), part, dg_full[:n * T], dg_part, (S, T, H))


@pytest.mark.parametrize('H', WIDTHS)
def test_lstm_rows_do_not_depend_on_tile_neighbours(H):
    """Sequences 0 - 4 of a 130-sequence launch (full tiles) and the same five alone (a ragged tile): bit-identical
    rows, forward and backward."""
    from rl_games_amd import ops
    S, T, I, n = 130, 8, 20, 5
    inputs = lstm32, x32, h0, c0, dones, d_out = _inputs(S, T, I, H, True)
    full = _forward(ops, lstm32, x32.to(DEV), h0, c0, dones, T)
    dg_full = _backward(ops, full, c0, dones, d_out, T)
    part, dg_part = _first_sequences_alone(ops, inputs, n, T)
    _same_bits(_head(full, n, T), part, dg_full[:n * T], dg_part, H)


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('pattern', ['first', 'last', 'all', 'zeros'])
def test_lstm_done_patterns(pattern, H):
    """S = 37, T = 4, I = 12 with explicit dones, each held to the fp64 reference at the bounds above, and
      first: every sequence reset at t = 0 only - the bits of the run with h0 = c0 = 0 and no dones (forward, d_gates);
      last:  reset at t = T - 1 only;
      all:   every step reset - each row the bits of the launch that takes the S * T rows as S * T sequences of one
             step with zero initial states;
      zeros: an all-zero dones tensor - the bits of dones = None.
    As measured on an MI355X, the largest |diff| over the 12 cases: out 8.9e-8, hT 6.0e-8, cT 1.2e-7, c_all 1.8e-7,
    hprev 8.9e-8, dx 3.0e-7, dW_ih 7.6e-6, dW_hh 1.8e-6, db 1.9e-6; every bit-identity holds."""
    from rl_games_amd import ops
    S, T, I = 37, 4, 12
    inputs = lstm32, x32, h0, c0, _, d_out = _inputs(S, T, I, H, False)
    d = torch.zeros(S, T, dtype=torch.uint8)
    if pattern == 'first':
        d[:, 0] = 1
    elif pattern == 'last':
        d[:, T - 1] = 1
    elif pattern == 'all':
        d[:] = 1
    dones = d.reshape(S * T).to(DEV)
    r, d_gates = _check_against_fp64(S, T, I, False, H, inputs, dones=dones)
    x = x32.to(DEV)
    if pattern == 'first':
        zero = torch.zeros_like(h0)
        other = _forward(ops, lstm32, x, zero, zero, None, T)
        _same_bits(r, other, d_gates, _backward(ops, other, zero, None, d_out, T), pattern)
    elif pattern == 'all':
        zero = torch.zeros(S * T, H, device=DEV)
        other = _forward(ops, lstm32, x, zero, zero, None, 1)
        dg_other = _backward(ops, other, zero, None, d_out, 1)
        for k in ('out', 'gates', 'c_all', 'hprev'):
            assert torch.equal(r[k], other[k]), k
        last = slice(T - 1, S * T, T)
        assert torch.equal(r['hT'], other['hT'][last]) and torch.equal(r['cT'], other['cT'][last])
        assert torch.equal(r['hT'], r['out'][last]) and torch.equal(r['cT'], r['c_all'][last])
        assert torch.equal(d_gates, dg_other)
    elif pattern == 'zeros':
        other = _forward(ops, lstm32, x, h0, c0, None, T)
        _same_bits(r, other, d_gates, _backward(ops, other, c0, None, d_out, T), pattern)


@pytest.mark.parametrize('H', WIDTHS)
def test_lstm_single_sequence_single_step_and_optional_finals(H):
    """S = 1, T = 1 (one live row in the tile; without and with its reset) against fp64, and a training call without
    h_final / c_final: the bits of the call that asks for them.
    As measured on an MI355X, the largest |diff| at S = T = 1: out 6.0e-8, cT 8.9e-8, dx 7.5e-8, dW_ih 1.2e-7,
    dW_hh 8.9e-8, db 8.9e-8."""
    from rl_games_amd import ops
    _check_against_fp64(1, 1, 3, False, H)
    _check_against_fp64(1, 1, 3, False, H, dones=torch.ones(1, dtype=torch.uint8, device=DEV))
    S, T, I = 37, 4, 12
    lstm32, x32, h0, c0, dones, _ = _inputs(S, T, I, H, True)
    x = x32.to(DEV)
    full = _forward(ops, lstm32, x, h0, c0, dones, T)
    bare = _forward(ops, lstm32, x, h0, c0, dones, T, finals=False)
    assert bare['hT'] is None and bare['cT'] is None
    for k in ('out', 'gates', 'c_all', 'hprev'):
        assert torch.equal(full[k], bare[k]), k


def test_lstm_rejects_unsupported_hidden_and_cpu():
    from rl_games_amd import ops
    assert ops.lstm_supported(64) and not ops.lstm_supported(100)
    g = torch.zeros(4, 400, device=DEV)
    with pytest.raises(RuntimeError):
        ops.lstm_seq_forward(g, torch.zeros(400, 100, device=DEV), torch.zeros(4, 100, device=DEV),
                             torch.zeros(4, 100, device=DEV), None, torch.zeros(4, 100, device=DEV))
    with pytest.raises(Exception):
        ops.lstm_seq_forward(torch.zeros(4, 256), torch.zeros(256, 64), torch.zeros(4, 64), torch.zeros(4, 64),
                             None, torch.zeros(4, 64))
