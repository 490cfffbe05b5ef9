"""CPU: the host side of `use_diagnostics` (rl_games_amd/diagnostics.py) against the REAL reference's diagnostics of one
epoch (tests/golden/epoch_diagnostics.pt, tests/golden/make_diagnostics_golden.py).  The recorded per-minibatch tensors
are reduced to table rows in fp64 (diagnostics.reference_row, the kernel's contract) and folded by PpoDiagnostics; the
result must be the reference's diag_dict, key for key, and reach the writer in the reference's order."""
import pytest
import torch

from rl_games_amd import diagnostics as D

VARIANTS = ('default', 'smooth_reg_ema', 'lstm', 'discrete_masked', 'multi_discrete_masked')


class _Agent:
    """The attributes PpoDiagnostics.epoch reads, holding the recorded statistics."""

    def __init__(self, diag_dict):
        self.normalize_rms_advantage = 'diagnostics/rms_advantage/mean' in diag_dict
        self.normalize_value = 'diagnostics/rms_value/mean' in diag_dict
        if self.normalize_value:
            self.value_mean_std = type('V', (), {'running_mean': diag_dict['diagnostics/rms_value/mean'],
                                                 'running_var': diag_dict['diagnostics/rms_value/var']})()
        if self.normalize_rms_advantage:
            mean, var = diag_dict['diagnostics/rms_advantage/mean'], diag_dict['diagnostics/rms_advantage/var']
            self.advantage_mean_std = type('A', (), {'get_mean_std': lambda s: (mean, torch.sqrt(var))})()


class _Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, float(value.reshape(-1)[0]), step))


def _replay(rec):
    """PpoDiagnostics fed the recorded minibatches (CPU tensors) in the reference's call pattern."""
    diag = rec['diag']
    d = D.PpoDiagnostics()
    agent = _Agent(diag['diag_dict'])
    mbs = diag['minibatches']
    nmb = len(mbs) // diag['mini_epochs']
    for me in range(diag['mini_epochs']):
        for i in range(nmb):
            d.mini_batch(agent, mbs[me * nmb + i], mbs[me * nmb + i]['e_clip'], i)
        d.mini_epoch(agent, me)
    d.epoch(agent, current_epoch=1)
    return d


@pytest.mark.parametrize('variant', VARIANTS)
def test_host_fold_matches_reference(golden, variant):
    rec = golden('epoch_diagnostics.pt')[variant]
    want = rec['diag']['diag_dict']
    d = _replay(rec)
    assert list(d.diag_dict) == list(want)
    for k, v in want.items():
        got = d.diag_dict[k]
        assert got.dtype == v.dtype and got.shape == v.shape, k
        if k.startswith('diagnostics/rms_'):
            assert torch.equal(got, v), k
        else:
            # reference: fp32 arithmetic; here: fp64 rounded once
            assert torch.allclose(got, v, rtol=0, atol=1e-5), (k, got, v)
    if 'masked' in variant and variant.startswith('discrete'):
        assert any(m['masks'] is not None and (m['masks'] == 0).any() for m in rec['diag']['minibatches'])


@pytest.mark.parametrize('variant', ('default', 'discrete_masked'))
def test_writer_sequence_matches_reference(golden, variant):
    rec = golden('epoch_diagnostics.pt')[variant]
    d = _replay(rec)
    w = _Writer()
    d.send_info(w)
    want = [(k, float(v.reshape(-1)[0]), 1) for k, v in rec['diag']['diag_dict'].items()]
    assert [c[0] for c in w.calls] == [c[0] for c in want]
    assert all(c[2] == 1 for c in w.calls)
    for (_, got, _), (k, v, _) in zip(w.calls, want):
        assert abs(got - v) <= 1e-5, k
    d.send_info(None)       # no writer: nothing happens


def test_masked_forms_are_the_reference_quirks():
    """Masked explained variance uses var(values) (not var(returns)); masked clip fraction is divided by the rows."""
    g = torch.Generator().manual_seed(3)
    v, r = torch.randn(64, 1, generator=g), torch.randn(64, 1, generator=g) * 3
    old, new = torch.randn(64, generator=g) * 0.2, torch.randn(64, generator=g) * 0.2
    m = (torch.rand(64, generator=g) > 0.3).float()
    row = D.reference_row(v, r, new, old, 0.2, m)
    clip, ev = D.fold_rows(row[None], masked=True)
    mm = m.double()
    vv, dd = v.reshape(-1).double(), (r - v).reshape(-1).double()
    W = mm.sum()
    var = lambda x: ((x * mm).pow(2).sum() / W - ((x * mm).sum() / W) ** 2) * W / (W - 1)
    assert torch.allclose(ev[0], 1 - var(dd) / var(vv), rtol=1e-10)
    lr = old - new
    c = ((lr < torch.tensor(float(torch.log(torch.tensor(0.8, dtype=torch.float64))), dtype=torch.float32))
         | (lr > torch.tensor(float(torch.log(torch.tensor(1.2, dtype=torch.float64))), dtype=torch.float32))).double()
    assert torch.allclose(clip, (c * mm).sum() / W / 64, rtol=1e-12)
    # no valid row: NaN, as sum(m) is not clamped in the reference's clip fraction
    row0 = D.reference_row(v, r, new, old, 0.2, torch.zeros(64))
    assert torch.isnan(D.fold_rows(row0[None], masked=True)[0])


def test_default_diagnostics_is_a_no_op():
    d = D.DefaultDiagnostics()
    w = _Writer()
    assert d.mini_batch(None, {}, 0.2, 0) is None
    assert d.mini_epoch(None, 0) is None
    assert d.epoch(None, 1) is None
    d.send_info(w)
    assert w.calls == [] and not hasattr(d, 'diag_dict')


def test_masked_value_columns_follow_the_reference_broadcast():
    """value_size > 1 with masks: get_mean_var_with_masks of a [rows, V] tensor under the [rows, 1] mask (sum_mask = the
    valid ROWS), formed from the element moments of the table row; the masked clip fraction divides by the rows."""
    g = torch.Generator().manual_seed(5)
    rows, V = 40, 3
    v, r = torch.randn(rows, V, generator=g), torch.randn(rows, V, generator=g) * 2
    old, new = torch.randn(rows, generator=g) * 0.3, torch.randn(rows, generator=g) * 0.3
    m = (torch.rand(rows, generator=g) > 0.4).float()
    row = D.reference_row(v, r, new, old, 0.2, m)
    clip, ev = D.fold_rows(row[None], masked=True)

    def ref_var(x):                      # torch_ext.get_mean_var_with_masks, in fp64
        mm = m.double().unsqueeze(1)
        S = mm.sum().clamp(min=1.0)
        xm = x.double() * mm
        return ((xm ** 2 / S).sum() - (xm / S).sum() ** 2) * S / (S - 1).clamp(min=1.0)
    assert torch.allclose(ev[0], 1 - ref_var(r - v) / ref_var(v), rtol=1e-9)
    assert row[D.ROWS] == rows and row[D.ELEMENTS] == rows * V
    lo, hi = D.ops.ppo_diag_log_bounds(0.2)
    lr = old - new
    c = ((lr < lo) | (lr > hi)).double()
    assert torch.allclose(clip, (c * m.double() / m.double().sum()).mean(), rtol=1e-12)
