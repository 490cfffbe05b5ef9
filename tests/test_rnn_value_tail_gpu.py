"""GPU: csrc/rnn_value_tail.hip - value column + clipped value loss + its backward behind the recurrent layer of a
central value critic, one launch.  Every bound is derived: the value is one rounding of an fp64 sum of exact products
(2^-24 relative, plus 2^-45 of the terms' magnitude for the fp64 summation: at most 128 terms of 2^-53 each); the row
loss is the device function of rlg_value_loss, so d_values has its bits; d_feat is one fp32 product; the partial sums
are fp64 (2^-40 of the terms' magnitude covers 1029 rows of 2^-53 each with room) rounded to fp32 once.  The formulas
themselves are pinned on the CPU (tests/test_rnn_value_tail_cpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_CLIP = 0.2
WIDTHS = [16, 32, 64, 128]
ROWS = [1, 15, 17, 37, 1029]
_cache = {}


def _head(feat, w, b):
    from rl_games_amd import ops
    values = torch.full((feat.shape[0],), float('nan'), device=DEV)
    ops.rnn_value_head(feat, w, b, values)
    return values


def _case(H, rows):
    """Inputs of one shape; computed once, shared, never modified.  old_values are built from a first head-only run so
    that every branch of the row formula is taken: exactly on either edge of the clip range, equal branches, far outside,
    and ordinary rows on both sides."""
    key = (H, rows)
    if key not in _cache:
        g = torch.Generator().manual_seed(H * 10007 + rows)
        feat = torch.randn(rows, H, generator=g).to(DEV)
        w = (torch.randn(H, generator=g) / H ** 0.5).to(DEV)
        b = torch.randn(1, generator=g).to(DEV)
        v = _head(feat, w, b)
        e = torch.tensor(E_CLIP, dtype=torch.float32, device=DEV)
        old = v + (torch.randn(rows, generator=g) * 0.3).to(DEV)
        returns = v + torch.randn(rows, generator=g).to(DEV)
        kind = torch.arange(rows, device=DEV) % 8
        old = torch.where(kind == 1, v + e, old)
        old = torch.where(kind == 2, v - e, old)
        old = torch.where(kind == 3, v, old)                       # delta 0: c1 == c2
        old = torch.where(kind == 4, v + 5.0, old)
        old = torch.where(kind == 5, v - 5.0, old)
        mask = (torch.rand(rows, generator=g) < 0.7).float().to(DEV)
        if rows > 1:
            mask[0] = 1.0                                           # (rows == 1 stays as drawn)
        _cache[key] = dict(feat=feat, w=w, b=b, old=old, returns=returns, mask=mask, head=v)
    return _cache[key]


def _tail(c, clip_value, mask=None, mask_sum=None, rows=None, feat=None):
    from rl_games_amd import ops
    feat = c['feat'] if feat is None else feat
    old, returns = c['old'], c['returns']
    if rows is not None:
        feat, old, returns = feat[:rows].contiguous(), old[:rows].contiguous(), returns[:rows].contiguous()
        mask = None if mask is None else mask[:rows].contiguous()
    rows, H = feat.shape
    nb = ops.rnn_value_tail_blocks(rows, H)
    assert 1 <= nb <= 256
    nan = float('nan')
    out = dict(values=torch.full((rows,), nan, device=DEV), d_values=torch.full((rows,), nan, device=DEV),
               d_feat=torch.full((rows, H), nan, device=DEV),
               loss_partials=torch.full((nb * 7,), nan, dtype=torch.float64, device=DEV),
               d_w_partials=torch.full((nb * H,), nan, dtype=torch.float64, device=DEV),
               d_b_partials=torch.full((nb,), nan, dtype=torch.float64, device=DEV), nb=nb)
    if mask is not None and mask_sum is None:
        mask_sum = mask.sum().reshape(1)
    ops.rnn_value_tail(feat, c['w'], c['b'], old, returns, out['values'], out['d_values'], out['d_feat'],
                       out['loss_partials'], out['d_w_partials'], out['d_b_partials'], nb, E_CLIP, clip_value, mask,
                       mask_sum)
    out.update(feat=feat, old=old, returns=returns, mask=mask, mask_sum=mask_sum)
    return out


def _finalised_row(partials, nb, rows, masked):
    from rl_games_amd import ops
    row = torch.full((8,), float('nan'), device=DEV)
    ops.ppo_loss_finalize(partials, nb, 0, rows, masked, 2.0, 0.0, 0.0, row, torch.zeros(1, device=DEV))
    return row


def _check(c, got, clip_value):
    from rl_games_amd import ops
    feat, w, b = got['feat'], c['w'], c['b']
    rows, H = feat.shape
    mask, mask_sum = got['mask'], got['mask_sum']
    # values: one rounding of the fp64 product; the head entry's bits
    terms = feat.double() * w.double()
    v64 = b.double() + terms.sum(1)
    bound = 2.0 ** -24 * v64.abs() + 2.0 ** -45 * (b.double().abs() + terms.abs().sum(1))
    err = (got['values'].double() - v64).abs()
    print(f'values: max err {err.max().item():.3e}, smallest bound {bound.min().item():.3e}')
    assert bool((err <= bound).all()), (err.max().item(), bound.min().item())
    assert torch.equal(got['values'], _head(feat, w, b))
    # d_values: the bits of rlg_value_loss on the kernel's own values
    want_d = torch.full((rows,), float('nan'), device=DEV)
    nbl = (rows + 255) // 256
    want_part = torch.full((nbl, 7), float('nan'), dtype=torch.float64, device=DEV)
    ops.value_loss(got['values'], got['old'], got['returns'], want_d, want_part, E_CLIP, clip_value, mask, mask_sum)
    assert torch.equal(got['d_values'], want_d)
    # d_feat: one fp32 product
    assert torch.equal(got['d_feat'], got['d_values'][:, None] * w[None, :])
    # the finalised loss row: the same fp64 terms in another order, rounded to fp32 once
    row = _finalised_row(got['loss_partials'], got['nb'], rows, mask is not None).cpu().numpy()
    want_row = _finalised_row(want_part, nbl, rows, mask is not None).cpu().numpy()
    print(f'loss row: {row.tolist()} against {want_row.tolist()}')
    ulp = np.spacing(np.abs(want_row))
    assert np.all(np.abs(row.astype(np.float64) - want_row.astype(np.float64)) <= ulp), (row, want_row)
    # finalised d_w, d_b: fp64 sums of the kernel's own d_values
    d_w, d_b = torch.full((H,), float('nan'), device=DEV), torch.full((1,), float('nan'), device=DEV)
    ops.colsum_finalize(got['d_w_partials'], got['nb'], H, d_w)
    ops.colsum_finalize(got['d_b_partials'], got['nb'], 1, d_b)
    tw = got['d_values'].double()[:, None] * feat.double()
    for name, val, truth, mag in (('d_w', d_w, tw.sum(0), tw.abs().sum(0)),
                                  ('d_b', d_b, got['d_values'].double().sum().reshape(1),
                                   got['d_values'].double().abs().sum().reshape(1))):
        err = (val.double() - truth).abs()
        bound = 2.0 ** -24 * truth.abs() + 2.0 ** -40 * mag
        print(f'{name}: max err {err.max().item():.3e}')
        assert bool((err <= bound).all()), (name, err.max().item())


@pytest.mark.parametrize('clip_value', [0, 1])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('H', WIDTHS)
def test_value_tail_outputs(H, rows, masked, clip_value):
    c = _case(H, rows)
    got = _tail(c, clip_value, c['mask'] if masked else None)
    if clip_value and rows >= 17:
        delta = got['values'] - got['old']
        assert bool((delta == 0).any()) and bool((delta > 1).any()) and bool((delta < -1).any())
        assert bool(((delta.abs() - E_CLIP).abs() < 1e-6).any())           # rows on the edges of the clip range
    _check(c, got, clip_value)


@pytest.mark.parametrize('clip_value', [0, 1])
def test_value_tail_with_every_row_masked_out(clip_value):
    """sum(mask) = 0: the denominator clamps to 1, every gradient is zero (not NaN)."""
    c = _case(64, 37)
    got = _tail(c, clip_value, torch.zeros(37, device=DEV))
    _check(c, got, clip_value)
    assert bool((got['d_values'] == 0).all()) and bool((got['d_feat'] == 0).all())


@pytest.mark.parametrize('H', WIDTHS)
def test_value_tail_rows_are_independent(H):
    """The first 37 rows of the 1,029-row launch and the 37-row launch with the same denominator: the same bits."""
    c = _case(H, 1029)
    ones, msum = torch.ones(1029, device=DEV), torch.full((1,), 1029.0, device=DEV)
    full, part = _tail(c, 1, ones, msum), _tail(c, 1, ones, msum, rows=37)
    for name in ('values', 'd_values', 'd_feat'):
        assert torch.equal(full[name][:37], part[name]), name


@pytest.mark.parametrize('H', WIDTHS)
def test_value_tail_nan_row_stays_in_its_row(H):
    c = _case(H, 37)
    clean = _tail(c, 1)
    feat = c['feat'].clone()
    feat[5, H // 2] = float('nan')
    got = _tail(c, 1, feat=feat)
    keep = torch.arange(37, device=DEV) != 5
    for name in ('values', 'd_values', 'd_feat'):
        assert bool(torch.isnan(got[name][5]).all()), name
        assert torch.equal(got[name][keep], clean[name][keep]), name
    assert bool(torch.isnan(_head(feat, c['w'], c['b'])[5]))


def test_value_tail_bad_arguments_raise_without_launching():
    from rl_games_amd import ops
    assert ops.rnn_value_tail_blocks(64, 100) == 0 and ops.rnn_value_tail_blocks(0, 64) == 0
    assert ops.rnn_value_tail_blocks(10 ** 7, 128) == 256
    H, rows = 64, 8
    feat = torch.zeros(rows, H, device=DEV)
    d_feat = torch.full_like(feat, 7.0)
    w, b = torch.ones(H, device=DEV), torch.zeros(1, device=DEV)
    vec = torch.zeros(rows, device=DEV)
    values, d_values = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    lp = torch.zeros(2048 * 7, dtype=torch.float64, device=DEV)
    pw = torch.zeros(2048 * 128, dtype=torch.float64, device=DEV)
    pb = torch.zeros(2048, dtype=torch.float64, device=DEV)

    def tail(feat=feat, d_feat=d_feat, w=w, nb=1, mask=None, mask_sum=None, n=rows):
        ops.rnn_value_tail(feat, w, b, vec[:n], vec[:n], values[:n], d_values[:n], d_feat, lp, pw, pb, nb, E_CLIP, True,
                           mask, mask_sum)
    wide = torch.zeros(rows, 100, device=DEV)
    odd = torch.zeros(rows * H + 4, device=DEV)[1:1 + rows * H].view(rows, H)          # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError):                       # width outside 16 / 32 / 64 / 128
        tail(feat=wide, d_feat=torch.empty_like(wide), w=torch.ones(100, device=DEV))
    with pytest.raises(RuntimeError):
        ops.rnn_value_head(wide, torch.ones(100, device=DEV), b, values)
    with pytest.raises(RuntimeError):                       # no rows
        tail(feat=feat[:0], d_feat=d_feat[:0], n=0)
    with pytest.raises(RuntimeError):
        ops.rnn_value_head(feat[:0], w, b, values[:0])
    for nb in (0, 1025):                                    # block count outside the launcher's range
        with pytest.raises(RuntimeError):
            tail(nb=nb)
    with pytest.raises(RuntimeError):
        tail(feat=odd)
    with pytest.raises(RuntimeError):
        tail(d_feat=odd)
    with pytest.raises(RuntimeError):
        ops.rnn_value_head(odd, w, b, values)
    with pytest.raises(RuntimeError):                       # a mask without its sum
        tail(mask=torch.ones(rows, device=DEV))
    with pytest.raises(ValueError):                         # a required pointer missing
        ops.rnn_value_head(feat, w, None, values)
    torch.cuda.synchronize()
    assert bool((d_feat == 7.0).all()) and bool((values == 7.0).all()) and bool((d_values == 7.0).all())   # nothing ran
