"""GPU: a paired sequence launch computes, bit for bit, what the two single launches compute.

ops.lstm_seq_forward_pair / _backward_pair and ops.gru_seq_forward_pair / _backward_pair run two problems of one shape
in one launch whose grid has a second row (csrc/rnn_seq.hpp, "paired launches").  A workgroup of a paired launch runs
the body of the single kernel on the tile rule of a single launch, so every output must be torch.equal to the single
launches' - no tolerance.

Shapes: (1, 1) one lone sequence; (5, 4) a partial tile; (17, 4) one sequence past the wide tile of 16 and past
several narrow tiles; (17, 1) the same in the rollout form.  The two problems get different weights, gate inputs,
initial states and dones patterns (with resets inside the sequences), so that a mix-up of their pointers cannot
cancel; every output buffer starts as NaN, and none may be left.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WIDTHS = [16, 32, 64, 128]
SHAPES = [(1, 1), (5, 4), (17, 4), (17, 1)]
NG = {'lstm': 4, 'gru': 3}


# the single wrappers' positional order (without seq_len): what the paired wrappers take per problem
ORDER = {
    ('lstm', 'forward'): ('gates', 'w_hh', 'h0', 'c0', 'dones', 'out', 'c_all', 'hprev', 'h_final', 'c_final'),
    ('lstm', 'backward'): ('gates', 'c_all', 'c0', 'dones', 'w_hh', 'd_out', 'd_gates'),
    ('gru', 'forward'): ('gates', 'w_hh', 'b_hh', 'h0', 'dones', 'out', 'hn_all', 'hprev', 'h_final'),
    ('gru', 'backward'): ('gates', 'hn_all', 'hprev', 'dones', 'w_hh', 'd_out', 'd_gx', 'd_gh'),
}


def _positional(cell, direction, args):
    return tuple(args.get(k) for k in ORDER[cell, direction])


def _poison(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def _problem(cell, S, T, H, seed):
    """inputs of one problem; `seed` also shifts the dones pattern"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * S + T + H)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(DEV)
    p = dict(gx=r(S * T, NG[cell] * H), w_hh=r(NG[cell] * H, H, scale=H ** -0.5), h0=r(S, H), d_out=r(S * T, H))
    if cell == 'lstm':
        p['c0'] = r(S, H)
    else:
        p['b_hh'] = r(NG[cell] * H, scale=0.3)
    dones = (torch.arange(S * T) * (3 + 2 * seed) + seed) % 5 == 0       # resets at t = 0 and inside the sequences
    p['dones'] = dones.to(torch.uint8).to(DEV)
    return p


def _forward_args(cell, p, S, T, H, form):
    """(arguments of the single forward by name, the output buffers among them); the gates start as the inputs"""
    out = dict(gates=p['gx'].clone(), out=_poison(S * T, H))
    if form == 'train':
        out.update({'c_all' if cell == 'lstm' else 'hn_all': _poison(S * T, H), 'hprev': _poison(S * T, H)})
    else:
        out['h_final'] = _poison(S, H)
        if cell == 'lstm':
            out['c_final'] = _poison(S, H)
    args = dict(out, w_hh=p['w_hh'], h0=p['h0'], dones=p['dones'])
    args.update({'c0': p['c0']} if cell == 'lstm' else {'b_hh': p['b_hh']})
    return args, out


def _run_forward(ops, cell, pa, pb, S, T, H, forms, paired):
    (a, out_a), (b, out_b) = (_forward_args(cell, p, S, T, H, f) for p, f in zip((pa, pb), forms))
    if paired:
        getattr(ops, f'{cell}_seq_forward_pair')(_positional(cell, 'forward', a), _positional(cell, 'forward', b),
                                                 seq_len=T)
    else:
        for args in (a, b):
            getattr(ops, f'{cell}_seq_forward')(**args, seq_len=T)
    return out_a, out_b


def _assert_same(pair, single, what):
    assert set(pair) == set(single)
    for k in pair:
        assert not torch.isnan(pair[k]).any(), f'{what}: poison left in the paired launch\'s {k}'
        assert not torch.isnan(single[k]).any(), f'{what}: poison left in the single launch\'s {k}'
        assert torch.equal(pair[k], single[k]), f'{what}: {k} differs by {(pair[k] - single[k]).abs().max().item():.3e}'


@pytest.mark.parametrize('S,T', SHAPES)
@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_paired_forward_equals_two_single_launches(cell, H, S, T):
    from rl_games_amd import ops
    pa, pb = _problem(cell, S, T, H, 1), _problem(cell, S, T, H, 2)
    # training form, inference form, A keeping the training outputs while B keeps the final states, and - optional
    # inputs as well - B without done flags
    pb_no_dones = dict(pb, dones=None)
    for forms, b_in in ((('train', 'train'), pb), (('infer', 'infer'), pb), (('train', 'infer'), pb),
                        (('train', 'train'), pb_no_dones)):
        pair = _run_forward(ops, cell, pa, b_in, S, T, H, forms, paired=True)
        single = _run_forward(ops, cell, pa, b_in, S, T, H, forms, paired=False)
        for side, got, ref in zip('AB', pair, single):
            _assert_same(got, ref, f'{forms} problem {side}')
    # the two problems did not compute the same thing
    assert not torch.equal(pair[0]['out'], pair[1]['out'])


@pytest.mark.parametrize('S,T', SHAPES)
@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_paired_backward_equals_two_single_launches(cell, H, S, T):
    from rl_games_amd import ops
    pa, pb = _problem(cell, S, T, H, 3), _problem(cell, S, T, H, 4)
    pa = dict(pa, dones=None)                             # done flags for one problem only
    kept = _run_forward(ops, cell, pa, pb, S, T, H, ('train', 'train'), paired=False)

    def args_of(p, k):
        if cell == 'lstm':
            outs = dict(d_gates=_poison(S * T, 4 * H))
            return dict(outs, gates=k['gates'], c_all=k['c_all'], c0=p['c0'], dones=p['dones'], w_hh=p['w_hh'],
                        d_out=p['d_out']), outs
        outs = dict(d_gx=_poison(S * T, 3 * H), d_gh=_poison(S * T, 3 * H))
        return dict(outs, gates=k['gates'], hn_all=k['hn_all'], hprev=k['hprev'], dones=p['dones'], w_hh=p['w_hh'],
                    d_out=p['d_out']), outs

    (a, pair_a), (b, pair_b) = args_of(pa, kept[0]), args_of(pb, kept[1])
    getattr(ops, f'{cell}_seq_backward_pair')(_positional(cell, 'backward', a), _positional(cell, 'backward', b),
                                              seq_len=T)
    single = []
    for p, k in zip((pa, pb), kept):
        args, outs = args_of(p, k)
        getattr(ops, f'{cell}_seq_backward')(**args, seq_len=T)
        single.append(outs)
    _assert_same(pair_a, single[0], 'problem A')
    _assert_same(pair_b, single[1], 'problem B')
    first = 'd_gates' if cell == 'lstm' else 'd_gx'
    assert not torch.equal(pair_a[first], pair_b[first])


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_paired_launch_keeps_a_non_finite_problem_to_itself(cell, H):
    """Problem A carries a NaN in the whole gate-input row of sequence 3 at t = 2
    (tests/test_rnn_edges_gpu.py::test_non_finite_sequence_stays_in_its_sequence), problem B is clean: B's outputs are
    the bits of the single clean launch, forward and backward, and hold no NaN; A's sequence did turn NaN."""
    from rl_games_amd import ops
    S, T, bad = 37, 4, 3
    pa, pb = _problem(cell, S, T, H, 5), _problem(cell, S, T, H, 6)
    pa = dict(pa, gx=pa['gx'].clone())
    pa['gx'][bad * T + 2] = float('nan')
    pair_a, pair_b = _run_forward(ops, cell, pa, pb, S, T, H, ('train', 'train'), paired=True)
    b_args, alone = _forward_args(cell, pb, S, T, H, 'train')
    getattr(ops, f'{cell}_seq_forward')(**b_args, seq_len=T)
    _assert_same(pair_b, alone, 'forward, problem B')
    assert torch.isnan(pair_a['out'].reshape(S, T, H)[bad, 2:]).all()
    assert not torch.isnan(pair_a['out'].reshape(S, T, H)[torch.arange(S, device=DEV) != bad]).any()

    def args_of(p, k):
        if cell == 'lstm':
            outs = dict(d_gates=_poison(S * T, 4 * H))
            return dict(outs, gates=k['gates'], c_all=k['c_all'], c0=p['c0'], dones=p['dones'], w_hh=p['w_hh'],
                        d_out=p['d_out']), outs
        outs = dict(d_gx=_poison(S * T, 3 * H), d_gh=_poison(S * T, 3 * H))
        return dict(outs, gates=k['gates'], hn_all=k['hn_all'], hprev=k['hprev'], dones=p['dones'], w_hh=p['w_hh'],
                    d_out=p['d_out']), outs

    (a, _), (b, back_b) = args_of(pa, pair_a), args_of(pb, pair_b)
    getattr(ops, f'{cell}_seq_backward_pair')(_positional(cell, 'backward', a), _positional(cell, 'backward', b),
                                              seq_len=T)
    b, back_alone = args_of(pb, alone)
    getattr(ops, f'{cell}_seq_backward')(**b, seq_len=T)
    _assert_same(back_b, back_alone, 'backward, problem B')


def test_paired_wrappers_refuse_two_shapes_and_shared_outputs():
    from rl_games_amd import _lib, ops
    S, T, H = 5, 4, 32
    pa, pb = _problem('gru', S, T, H, 1), _problem('gru', S, T, H, 2)
    a, _ = _forward_args('gru', pa, S, T, H, 'train')
    b, _ = _forward_args('gru', pb, S, T, H, 'train')
    with pytest.raises(_lib.HipLibraryError):
        ops.gru_seq_forward_pair(_positional('gru', 'forward', a), _positional('gru', 'forward', dict(b, out=a['out'])),
                                 seq_len=T)
    other, _ = _forward_args('gru', _problem('gru', S + 1, T, H, 2), S + 1, T, H, 'train')
    with pytest.raises(ValueError):
        ops.gru_seq_forward_pair(_positional('gru', 'forward', a), _positional('gru', 'forward', other), seq_len=T)
