"""GPU: the edges of the eight sequence-persistent recurrent kernels - LSTM and GRU, forward and backward, in the narrow
scheme (csrc/lstm.hip, gru.hip: 16 / 32 / 64 units) and the wide one (csrc/lstm_wide.hip, gru_wide.hip: 128 units).

What tests/test_lstm_gpu.py does for the narrow LSTM is done here for the other kernels (done patterns, single steps,
optional outputs), and four regimes are entered that no other recurrent test reaches, for all eight: saturated gates,
a non-finite sequence, long sequences - every launch on NaN-poisoned output buffers.

The reference is a CPU evaluation in fp64 of torch.nn.LSTM / torch.nn.GRU stepped with the reference's done resets
(rl_games/common/layers/recurrent.py:26-58: the states are MULTIPLIED by 1 - done before the step), backward through
autograd on the CPU side.  Bounds, unless a test says otherwise, are those of _check_against_fp64 in
tests/test_lstm_gpu.py and tests/test_gru_gpu.py: forward outputs rtol 1e-5 + atol 2e-6; dx, dW_ih, dW_hh and the bias
gradients within 2e-5 max|ref| + 1e-7.

Shapes are tiny: S = 37, T = 4, I = 12 unless stated - 37 leaves a ragged last tile in every scheme (narrow tiles of
16 / 8 / 4 sequences; the wide tile holds 5 live and 11 aliased slots)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = [16, 32, 64, 128]
NG = {'lstm': 4, 'gru': 3}
ALL = [(cell, H) for cell in ('lstm', 'gru') for H in WIDTHS]
# the kernels without a done-pattern / optional-output suite of their own (the narrow LSTM has tests/test_lstm_gpu.py)
UNCOVERED = [('gru', H) for H in WIDTHS] + [('lstm', 128)]
NAN = float('nan')


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _inputs(cell, S, T, I, H, quantised=False):
    """Seeded fp32 parameters, inputs, initial states and d_out, on the CPU.  `quantised`: x, W_ih and the biases
    are drawn on grids (x: 1/32 within +-4; W_ih, biases: 1/256 within +-1/2) so that every input projection
    x W_ih^T + b is EXACT in fp32 in any order of summation, also after a power-of-two scale (12 products of 8 x 8 bits,
    unit 2^-13, |sum| < 32: 18 bits)."""
    g = torch.Generator().manual_seed(10007 * NG[cell] + 131 * S + 17 * T + I + 1000 * H)
    mod = (torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(I, H, 1)
    with torch.no_grad():
        for p in mod.parameters():              # torch's own initialisation, from a seeded generator
            p.uniform_(-H ** -0.5, H ** -0.5, generator=g)
        x = torch.randn(S * T, I, generator=g)
        if quantised:
            x = (x * 32).round().clamp(-128, 128) / 32
            for name in ('weight_ih_l0', 'bias_ih_l0', 'bias_hh_l0'):
                p = getattr(mod, name)
                p.copy_(torch.randint(-128, 129, p.shape, generator=g).float() / 256)
    inp = dict(cell=cell, S=S, T=T, I=I, H=H, x=x, h0=0.5 * torch.randn(S, H, generator=g), scale=None,
               params={k: v.detach().clone() for k, v in mod.state_dict().items()})
    if cell == 'lstm':
        inp['c0'] = 0.5 * torch.randn(S, H, generator=g)
    inp['d_out'] = torch.randn(S * T, H, generator=g)
    return inp


def _drawn_dones(S, T, seed=0):
    """A 20 % draw with sequence S // 2 cleared, a reset set at t = 0 of sequence 0 and at t = T - 1 of sequence 1."""
    g = torch.Generator().manual_seed(7 * S + T + seed)
    d = (torch.rand(S, T, generator=g) < 0.2).to(torch.uint8)
    d[S // 2] = 0
    d[0, 0] = 1
    d[1, T - 1] = 1
    assert d[:, 0].any() and d[:, T - 1].any() and (d.sum(1) == 0).any() and (d.sum(1) > 0).any()
    return d


# ---- the reference: CPU, torch.nn module stepped with the done resets -----------------------------------------------

def _reference(cell, mod, x, h0, c0, dones, T):
    """x [S*T, I] rows (seq, t); dones [S*T] or None.  out [S*T, H], the final states, what the kernels keep for
    backward (LSTM: the cell states; GRU: W_hn h + b_hn) and the states entering each step after the reset."""
    S, H = h0.shape
    xs = x.reshape(S, T, -1).transpose(0, 1)
    d = dones.reshape(S, T).t() if dones is not None else None
    h, c = h0.unsqueeze(0), (c0.unsqueeze(0) if cell == 'lstm' else None)
    outs, kept, entering = [], [], []
    for t in range(T):
        if d is not None:
            keep = (1.0 - d[t].float()).reshape(1, -1, 1).to(h.dtype)
            h = h * keep                        # recurrent.py: 0 * NaN stays NaN
            c = c * keep if cell == 'lstm' else None
        entering.append(h)
        if cell == 'lstm':
            o, (h, c) = mod(xs[t:t + 1], (h, c))
            kept.append(c)
        else:
            kept.append(h @ mod.weight_hh_l0[2 * H:].t() + mod.bias_hh_l0[2 * H:])
            o, h = mod(xs[t:t + 1], h)
        outs.append(o)

    def rows(parts):
        return torch.cat(parts, 0).transpose(0, 1).reshape(S * T, -1)
    r = dict(out=rows(outs), hT=h[0], kept=rows(kept), hprev=rows(entering))
    if cell == 'lstm':
        r['cT'] = c[0]
    return r


def _cpu_run(inp, dones, dtype):
    """Forward and autograd backward on the CPU in `dtype` (fp64: the reference; fp32: torch's own arithmetic, the
    yardstick of the new regimes).  The gate inputs are formed as the kernels get them - the input projection, then
    the per-column scale - and enter the torch.nn module through an identity W_ih and a zero b_ih; the GRU's b_hh stays
    in the module, the LSTM's is part of the gate inputs.  Every quantity as an fp64 CPU tensor."""
    cell, T, H = inp['cell'], inp['T'], inp['H']
    G = NG[cell] * H
    p = {k: v.to(dtype).requires_grad_(True) for k, v in inp['params'].items()}
    x = inp['x'].to(dtype).requires_grad_(True)
    bias = p['bias_ih_l0'] + p['bias_hh_l0'] if cell == 'lstm' else p['bias_ih_l0']
    gx = x @ p['weight_ih_l0'].t() + bias
    if inp['scale'] is not None:
        gx = gx * inp['scale'].to(dtype)
    mod = (torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(G, H, 1).to(dtype)
    with torch.no_grad():
        mod.weight_ih_l0.copy_(torch.eye(G, dtype=dtype))
        mod.bias_ih_l0.zero_()
        mod.weight_hh_l0.copy_(p['weight_hh_l0'])
        mod.bias_hh_l0.copy_(torch.zeros(G, dtype=dtype) if cell == 'lstm' else p['bias_hh_l0'])
    c0 = inp['c0'].to(dtype) if cell == 'lstm' else None
    r = _reference(cell, mod, gx, inp['h0'].to(dtype), c0, dones, T)
    r['out'].backward(inp['d_out'].to(dtype))
    r = {k: v.detach().double() for k, v in r.items()}
    db_hh = p['bias_hh_l0'].grad if cell == 'lstm' else mod.bias_hh_l0.grad
    r.update(dx=x.grad.double(), dw_ih=p['weight_ih_l0'].grad.double(), dw_hh=mod.weight_hh_l0.grad.double(),
             db_ih=p['bias_ih_l0'].grad.double(), db_hh=db_hh.double())
    return r


FORWARD = ('out', 'hT', 'cT', 'kept', 'hprev')
GRADS = ('dx', 'dw_ih', 'dw_hh', 'db_ih', 'db_hh')


def _forward_errors(got, ref):
    """{name: (max |diff|, whether within rtol 1e-5 + atol 2e-6)}"""
    return {k: ((got[k] - ref[k]).abs().max().item(), torch.allclose(got[k], ref[k], rtol=1e-5, atol=2e-6))
            for k in FORWARD if k in ref}


def _grad_errors(got, ref):
    """{name: (max |diff|, the bound 2e-5 max|ref| + 1e-7)}"""
    return {k: ((got[k] - ref[k]).abs().max().item(), 2e-5 * ref[k].abs().max().item() + 1e-7) for k in GRADS}


# ---- the kernels ----------------------------------------------------------------------------------------------------

def _poison(*shape):
    return torch.full(shape, NAN, device=DEV)


def _gate_inputs(inp):
    """[S*T, NG*H] on the device: the input projection (+ b_ih; LSTM: + b_hh), then the per-column scale."""
    p = inp['params']
    bias = p['bias_ih_l0'] + p['bias_hh_l0'] if inp['cell'] == 'lstm' else p['bias_ih_l0']
    gx = torch.addmm(bias.to(DEV), inp['x'].to(DEV), p['weight_ih_l0'].to(DEV).t())
    return gx if inp['scale'] is None else gx * inp['scale'].to(DEV)


def _launch(ops, inp, dones, T=None, gx=None, h0=None, c0=None, train=True, finals=True, poison_check=True):
    """One forward launch on NaN-poisoned output buffers.  gx / h0 / c0 replace the inputs' own; T their seq_len.
    Returns the buffers by the names of _reference (gates: the activated gates)."""
    cell, H = inp['cell'], inp['H']
    T = inp['T'] if T is None else T
    gates = (_gate_inputs(inp) if gx is None else gx).clone()
    S = gates.shape[0] // T
    h0 = (inp['h0'] if h0 is None else h0).to(DEV)
    w_hh = inp['params']['weight_hh_l0'].to(DEV).contiguous()
    dones = None if dones is None else dones.reshape(-1).to(DEV)
    r = dict(gates=gates, out=_poison(S * T, H), kept=_poison(S * T, H) if train else None,
             hprev=_poison(S * T, H) if train else None, hT=_poison(S, H) if finals else None)
    if cell == 'lstm':
        c0 = (inp['c0'] if c0 is None else c0).to(DEV)
        r['cT'] = _poison(S, H) if finals else None
        ops.lstm_seq_forward(gates, w_hh, h0, c0, dones, r['out'], r['kept'], r['hprev'], r['hT'], r['cT'], seq_len=T)
    else:
        ops.gru_seq_forward(gates, w_hh, inp['params']['bias_hh_l0'].to(DEV), h0, dones, r['out'], r['kept'],
                            r['hprev'], r['hT'], seq_len=T)
    torch.cuda.synchronize()
    if poison_check:
        for k, v in r.items():
            assert v is None or not torch.isnan(v).any(), f'NaN left in {k}'
    r.update(w_hh=w_hh, h0=h0, c0=c0, dones=dones, T=T)
    return r


def _launch_backward(ops, inp, r, d_out=None, poison_check=True):
    """(d_gx, d_gh) of one backward launch on what `r` kept; for the LSTM both are d_gates."""
    d_out = (inp['d_out'] if d_out is None else d_out).to(DEV)
    if inp['cell'] == 'lstm':
        d_gx = d_gh = _poison(*r['gates'].shape)
        ops.lstm_seq_backward(r['gates'], r['kept'], r['c0'], r['dones'], r['w_hh'], d_out, d_gx, r['T'])
    else:
        d_gx, d_gh = _poison(*r['gates'].shape), _poison(*r['gates'].shape)
        ops.gru_seq_backward(r['gates'], r['kept'], r['hprev'], r['dones'], r['w_hh'], d_out, d_gx, d_gh, r['T'])
    torch.cuda.synchronize()
    if poison_check:
        assert not torch.isnan(d_gx).any() and not torch.isnan(d_gh).any(), 'NaN left in the gate gradients'
    return d_gx, d_gh


def _kernel_quantities(inp, r, d_gx, d_gh):
    """What _cpu_run returns, from the kernels' outputs (the weight gradients are whole-sequence products outside the
    kernels, here in fp64 so that the comparison sees the kernels' error alone)."""
    q = {k: r[k].double().cpu() for k in FORWARD if r.get(k) is not None}
    d_gx, d_gh = d_gx.double().cpu(), d_gh.double().cpu()
    d_pre = d_gx if inp['scale'] is None else d_gx * inp['scale'].double()       # gradient of the unscaled projection
    q.update(dx=d_pre @ inp['params']['weight_ih_l0'].double(), dw_ih=d_pre.t() @ inp['x'].double(),
             dw_hh=d_gh.t() @ q['hprev'], db_ih=d_pre.sum(0), db_hh=d_pre.sum(0) if inp['cell'] == 'lstm' else d_gh.sum(0))
    return q


def _same_bits(a, b, what, keys=('out', 'gates', 'kept', 'hprev', 'hT', 'cT')):
    for k in keys:
        if k in a and a[k] is not None:
            assert torch.equal(a[k], b[k]), (what, k)


def _check_against_fp64(ops, inp, dones, yardstick=False):
    """One problem against the fp64 CPU module at the fixed bounds; hprev the bits of the previous row of out, zeroed
    where done; an inference call and repeats bit-identical.  `yardstick`: torch's fp32 CPU module is evaluated on the
    same inputs first and must itself meet the bounds (else the inputs, not the kernel, are at fault).  Returns the
    forward results, (d_gx, d_gh) and the measured errors."""
    cell, S, T, H = inp['cell'], inp['S'], inp['T'], inp['H']
    ref = _cpu_run(inp, dones, torch.float64)
    if yardstick:
        own = _cpu_run(inp, dones, torch.float32)
        for k, (err, ok) in _forward_errors(own, ref).items():
            print('torch fp32', k, 'max |diff|', err)
            assert ok, ('torch fp32', k, err)
        for k, (err, bound) in _grad_errors(own, ref).items():
            print('torch fp32', k, 'max |diff|', err, 'bound', bound)
            assert err <= bound, ('torch fp32', k, err, bound)

    r = _launch(ops, inp, dones)
    d_gx, d_gh = _launch_backward(ops, inp, r)
    for v in list(r.values()) + [d_gx, d_gh]:
        assert not torch.is_tensor(v) or v.dtype != torch.float32 or torch.isfinite(v).all()
    got = _kernel_quantities(inp, r, d_gx, d_gh)
    errors = {}
    for k, (err, ok) in _forward_errors(got, ref).items():
        print(cell, H, k, 'max |diff|', err)
        assert ok, (k, err)
        errors[k] = err
    for k, (err, bound) in _grad_errors(got, ref).items():
        print(cell, H, k, 'max |diff|', err, 'bound', bound)
        assert err <= bound, (k, err, bound)
        errors[k] = err

    # hprev IS the state entering each step: the previous row of out (h0 at t = 0), zeroed where done - bit for bit
    enter = torch.cat([r['h0'].unsqueeze(1), r['out'].reshape(S, T, H)[:, :-1]], 1).reshape(S * T, H)
    if dones is not None:
        enter = enter * (1.0 - r['dones'].float()).unsqueeze(1)
    assert torch.equal(r['hprev'], enter)
    last = slice(T - 1, S * T, T)
    assert torch.equal(r['hT'], r['out'][last])
    if cell == 'lstm':
        assert torch.equal(r['cT'], r['kept'][last])

    # an inference call (nothing kept for backward) and a second training call: bit-identical
    _same_bits(_launch(ops, inp, dones, train=False), r, 'inference', keys=('out', 'gates', 'hT', 'cT'))
    _same_bits(_launch(ops, inp, dones), r, 'repeat')
    again = _launch_backward(ops, inp, r)
    assert torch.equal(again[0], d_gx) and torch.equal(again[1], d_gh)
    return r, (d_gx, d_gh), errors


# ---- a. done patterns -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cell,H', UNCOVERED)
@pytest.mark.parametrize('pattern', ['first', 'last', 'all', 'zeros'])
def test_done_patterns(pattern, cell, H):
    """test_lstm_done_patterns for the GRU at every width and the LSTM at 128 units: S = 37, T = 4, I = 12 with
    explicit dones, each held to the fp64 reference at the fixed bounds, and
      first: every sequence reset at t = 0 only - the bits of the run with zero initial states and no dones;
      last:  reset at t = T - 1 only;
      all:   every step reset - each row the bits of the launch that takes the S * T rows as S * T sequences of one
             step with zero initial states (that launch goes through the T = 1 branch of the backward, which loads no
             W_hh); the finals are the last rows of out (and of c_all);
      zeros: an all-zero dones tensor - the bits of dones = None.
    As measured on an MI355X, the largest |diff| over the 20 cases, all at the fixed bounds: out 2.4e-7, hT 1.2e-7,
    cT 8.6e-8, c_all / hn_all 5.0e-7, hprev 2.4e-7, dx 1.5e-7, dW_ih 2.6e-6, dW_hh 6.4e-7, db_ih 1.5e-6, db_hh 1.1e-6
    (no gradient beyond 1 % of its bound); every bit-identity holds."""
    from rl_games_amd import ops
    S, T, I = 37, 4, 12
    inp = _inputs(cell, S, T, I, H)
    d = torch.zeros(S, T, dtype=torch.uint8)
    if pattern == 'first':
        d[:, 0] = 1
    elif pattern == 'last':
        d[:, T - 1] = 1
    elif pattern == 'all':
        d[:] = 1
    r, (d_gx, d_gh), _ = _check_against_fp64(ops, inp, d)
    zero = torch.zeros(S, H)
    if pattern == 'first':
        other = _launch(ops, inp, None, h0=zero, c0=zero)
    elif pattern == 'zeros':
        other = _launch(ops, inp, None)
    elif pattern == 'all':
        zero = torch.zeros(S * T, H)
        other = _launch(ops, inp, None, T=1, h0=zero, c0=zero)
        last = slice(T - 1, S * T, T)
        assert torch.equal(r['hT'], other['hT'][last]) and torch.equal(r['hT'], r['out'][last])
        if cell == 'lstm':
            assert torch.equal(r['cT'], other['cT'][last]) and torch.equal(r['cT'], r['kept'][last])
    else:
        return
    _same_bits(r, other, pattern, keys=('out', 'gates', 'kept', 'hprev') + (() if pattern == 'all' else ('hT', 'cT')))
    o_gx, o_gh = _launch_backward(ops, inp, other)
    assert torch.equal(d_gx, o_gx) and torch.equal(d_gh, o_gh)


# ---- b. single step -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cell,H', ALL)
def test_single_step(cell, H):
    """S = 1, T = 1 (one live slot in the tile) against fp64, without and with its reset, and S = 17, T = 1 with a
    reset on every other sequence: the rollout form, one sequence past the wide tile, through the T = 1 shortcut of
    the GRU and wide-LSTM backwards (no W_hh loaded, `break` at t = 0) with dones present; then S = 17, T = 2, the
    other side of that shortcut, which no other test takes the wide LSTM backward through.  Fixed bounds.
    As measured on an MI355X, the largest |diff| over the 8 kernels' four problems: out 1.1e-7, hT 1.1e-7, cT 1.3e-7,
    c_all / hn_all 3.0e-7, hprev 1.0e-7, dx 8.4e-8, dW_ih 1.0e-6, dW_hh 3.1e-7, db_ih 8.7e-7, db_hh 5.5e-7 (no
    gradient beyond 3 % of its bound)."""
    from rl_games_amd import ops
    inp = _inputs(cell, 1, 1, 3, H)
    _check_against_fp64(ops, inp, None)
    _check_against_fp64(ops, inp, torch.ones(1, 1, dtype=torch.uint8))
    inp = _inputs(cell, 17, 1, 12, H)
    d = (torch.arange(17) % 2 == 0).to(torch.uint8).reshape(17, 1)
    _check_against_fp64(ops, inp, d)
    # and the first length past that shortcut, T = 2: one product W_hh^T . dgates, one state handed back
    inp = _inputs(cell, 17, 2, 12, H)
    d = torch.stack([torch.arange(17) % 2 == 0, torch.arange(17) % 3 == 0], 1).to(torch.uint8)
    _check_against_fp64(ops, inp, d)


# ---- c. optional outputs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cell,H', UNCOVERED)
def test_optional_outputs(cell, H):
    """A training call without h_final (and c_final) gives the bits of the call that asks for them; an inference
    call that asks for the finals and keeps nothing for backward gives the finals' bits."""
    from rl_games_amd import ops
    S, T, I = 37, 4, 12
    inp = _inputs(cell, S, T, I, H)
    d = _drawn_dones(S, T)
    full = _launch(ops, inp, d)
    bare = _launch(ops, inp, d, finals=False)
    assert bare['hT'] is None and bare.get('cT') is None
    _same_bits(bare, full, 'no finals', keys=('out', 'gates', 'kept', 'hprev'))
    infer = _launch(ops, inp, d, train=False)
    assert infer['kept'] is None and infer['hprev'] is None
    _same_bits(infer, full, 'inference', keys=('out', 'gates', 'hT', 'cT'))
    both = _launch_backward(ops, inp, full), _launch_backward(ops, inp, dict(full, kept=bare['kept'],
                                                                             hprev=bare['hprev'], gates=bare['gates']))
    assert torch.equal(both[0][0], both[1][0]) and torch.equal(both[0][1], both[1][1])


# ---- e. saturated gates ---------------------------------------------------------------------------------------------

def _saturated_inputs(cell, H):
    """S = 37, T = 4, I = 12 on the exact grids of _inputs (gate inputs of about unit spread), and a power-of-two scale
    per gate column chosen by the hidden unit: unit j % 3 == 0 x 512, == 1 x 16, == 2 x 1.  The scaled gate inputs are
    exact in fp32, so the kernel and the fp64 reference see the same numbers."""
    inp = _inputs(cell, 37, 4, 12, H, quantised=True)
    per_unit = torch.tensor([512.0, 16.0, 1.0])[torch.arange(H) % 3]
    inp['scale'] = per_unit.repeat(NG[cell])
    return inp


def _assert_saturated_regime(inp, gx):
    """The three groups hold what the test claims: beyond +-100 with both signs, +-10 .. +-30, O(1)."""
    H = inp['H']
    gx = gx.double().cpu().reshape(gx.shape[0], NG[inp['cell']], H)
    unit = torch.arange(H) % 3
    big, mid, small = gx[:, :, unit == 0], gx[:, :, unit == 1], gx[:, :, unit == 2]
    assert (big > 100).double().mean() > 0.3 and (big < -100).double().mean() > 0.3
    assert (big.abs() > 100).all(1).any(), 'a unit with every gate of a step saturated'
    assert ((mid.abs() >= 10) & (mid.abs() <= 30)).double().mean() > 0.3
    assert (small.abs() < 4).double().mean() > 0.95
    # exact: the fp64 product of the same fp32 numbers, scaled
    p = {k: v.double() for k, v in inp['params'].items()}
    bias = p['bias_ih_l0'] + (p['bias_hh_l0'] if inp['cell'] == 'lstm' else 0.0)
    assert torch.equal(gx.reshape(gx.shape[0], -1), (inp['x'].double() @ p['weight_ih_l0'].t() + bias) * inp['scale'])


@pytest.mark.parametrize('cell,H', ALL)
def test_saturated_gates(cell, H):
    """Pre-activations of a third of the hidden units beyond +-100 (expf overflows in sigmoid_f from 88; the backward
    forms g (1 - g) and 1 - n^2 at exactly 0 and 1), a third in +-10 .. +-30, a third O(1): every forward and backward
    output finite, held to fp64 at the fixed bounds, repeats bit-identical.  torch's fp32 CPU module meets the fixed
    bounds on these inputs (asserted), so the fixed bounds are the yardstick; the 8 x rule of
    tests/test_rnn_layer_norm_gpu.py was not needed.
    As measured on an MI355X, the largest |diff| over the 8 cases (torch's fp32 CPU module on the same inputs in
    brackets): out 2.5e-7 (3.7e-7), hT 2.5e-7 (3.7e-7), cT 4.7e-7 (2.7e-7), c_all / hn_all 7.1e-7 (6.6e-7), hprev
    2.1e-7 (3.1e-7), dx 9.8e-5 (9.8e-5), dW_ih 6.6e-4 (6.6e-4), dW_hh 1.6e-6 (1.5e-6), db_ih 2.1e-4 (2.2e-4), db_hh
    7.3e-5 (7.3e-5); the gradients of the input side carry the scale of 512, their bounds (2e-5 max|ref|) are 2e-3 and
    more, and no gradient is beyond 7 % of its bound."""
    from rl_games_amd import ops
    inp = _saturated_inputs(cell, H)
    _assert_saturated_regime(inp, _gate_inputs(inp))
    _check_against_fp64(ops, inp, _drawn_dones(37, 4), yardstick=True)


# ---- f. a non-finite sequence stays in its sequence -----------------------------------------------------------------

def _assert_confined(inp, clean, dirty, bad, first_bad_t, what):
    """`dirty`: (forward results, (d_gx, d_gh)) of a launch whose sequence `bad` turns NaN at step first_bad_t.  Every
    other sequence has the clean launch's bits in every output; the bad one has them before first_bad_t (forward), and
    its out rows from first_bad_t on, and its final h, are NaN in every element."""
    S, T = inp['S'], inp['T']
    (rc, gc), (rd, gd) = clean, dirty
    others = torch.arange(S, device=DEV) != bad
    tensors = [(k, rc[k], rd[k]) for k in ('out', 'gates', 'kept', 'hprev', 'hT', 'cT') if rc.get(k) is not None]
    tensors += [('d_gx', gc[0], gd[0]), ('d_gh', gc[1], gd[1])]
    for k, a, b in tensors:
        assert not torch.isnan(a).any(), (what, k, 'the clean launch')
        per_seq = (lambda v: v) if a.shape[0] == S else (lambda v: v.reshape(S, T, -1))
        assert torch.equal(per_seq(a)[others], per_seq(b)[others]), (what, k, 'another sequence changed')
        if a.shape[0] != S and not k.startswith('d_'):
            assert torch.equal(per_seq(a)[bad, :first_bad_t], per_seq(b)[bad, :first_bad_t]), (what, k, 'before the NaN')
    assert torch.isnan(rd['out'].reshape(S, T, -1)[bad, first_bad_t:]).all(), (what, 'out after the NaN')
    assert torch.isnan(rd['hT'][bad]).all(), (what, 'h_final')


@pytest.mark.parametrize('cell,H', ALL)
def test_non_finite_sequence_stays_in_its_sequence(cell, H):
    """S = 37, T = 4: a NaN in the whole gate-input row of one sequence at t = 2 - sequence 3 (a live slot among live
    slots; in the wide scheme one of the 16 columns of an MFMA) and sequence S - 1 (the one the dead slots of the
    ragged tile alias, all of which turn NaN with it).  Both carry a reset at t = 3: the reference multiplies the
    state by 1 - done (rl_games/common/layers/recurrent.py:26-58), so 0 * NaN stays NaN and the kernels, which
    multiply by `keep` likewise, must not clean the row either.  A variant puts the NaN into the sequence's row of h0.
    This is data, not a fault: every launch succeeds."""
    from rl_games_amd import ops
    S, T, I = 37, 4, 12
    inp = _inputs(cell, S, T, I, H)
    d = _drawn_dones(S, T, seed=5)
    for bad in (3, S - 1):
        d[bad] = torch.tensor([0, 0, 0, 1], dtype=torch.uint8)
    gx = _gate_inputs(inp)

    def run(**kw):
        r = _launch(ops, inp, d, poison_check=False, **kw)
        return r, _launch_backward(ops, inp, r, poison_check=False)
    clean = run(gx=gx)
    for bad in (3, S - 1):
        dirty_gx = gx.clone()
        dirty_gx[bad * T + 2] = NAN
        _assert_confined(inp, clean, run(gx=dirty_gx), bad, 2, f'gate inputs of sequence {bad}')
        h0 = inp['h0'].clone()
        h0[bad] = NAN
        _assert_confined(inp, clean, run(gx=gx, h0=h0), bad, 0, f'h0 of sequence {bad}')


# ---- g. long sequences ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cell,H', ALL)
def test_long_sequences(cell, H):
    """S = 3, T = 160 (five times the longest sequence of any other test), resets at t = 0 of sequence 0, t = 159 of
    sequence 1 and t = 80 of sequence 2: fp64 at the fixed bounds, hprev the bits of the previous row of out.
    torch's fp32 CPU module meets the fixed bounds on these inputs (asserted), so the fixed bounds are the yardstick.
    As measured on an MI355X, the largest |diff| over the 8 cases (torch's fp32 CPU module in brackets): out 1.2e-7
    (1.3e-7), hT 7.4e-8 (5.5e-8), cT 8.5e-8 (8.5e-8), c_all / hn_all 3.4e-7 (1.6e-7), hprev 1.2e-7 (1.3e-7), dx 1.2e-7
    (5.2e-7), dW_ih 4.2e-6 (1.5e-5), dW_hh 8.9e-7 (4.7e-6), db_ih 3.8e-6 (8.0e-6), db_hh 3.4e-6 (8.0e-6); no gradient
    beyond 1 % of its bound."""
    from rl_games_amd import ops
    S, T = 3, 160
    inp = _inputs(cell, S, T, 12, H)
    d = torch.zeros(S, T, dtype=torch.uint8)
    d[0, 0] = d[1, 159] = d[2, 80] = 1
    _check_against_fp64(ops, inp, d, yardstick=True)
