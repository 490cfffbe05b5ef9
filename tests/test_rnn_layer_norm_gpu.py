"""GPU: csrc/rnn_layer_norm.hip - layer normalisation behind the recurrent layer - against fp64 layer_norm with
autograd on the same values.  The bound is the one of tests/test_discrete_gpu.py for the loss kernel's gradients: the
kernel may be at most 8 x as far from fp64 as torch's own fp32 layer_norm on the same device and inputs, or 2e-6 of the
output's scale.  The formulas themselves are pinned on the CPU (tests/test_rnn_layer_norm_cpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
WIDTHS = [16, 32, 64, 128]
ROWS = [1, 37, 64, 1029]
_cache = {}


def _case(H, rows, offset):
    """Inputs, the fp64 truth and torch's fp32 results for one shape; computed once, shared, never modified."""
    key = (H, rows, offset)
    if key not in _cache:
        g = torch.Generator().manual_seed(H * 10007 + rows * 3 + int(offset))
        x = (offset + torch.randn(rows, H, generator=g)).to(DEV)
        gamma = (1.0 + 0.5 * torch.randn(H, generator=g)).to(DEV)
        beta = torch.randn(H, generator=g).to(DEV)
        d_y = torch.randn(rows, H, generator=g).to(DEV)

        def run(dtype):
            xx = x.to(dtype).requires_grad_(True)
            gg, bb = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
            y = torch.nn.functional.layer_norm(xx, (H,), gg, bb, EPS)
            y.backward(d_y.to(dtype))
            return {'y': y.detach(), 'd_x': xx.grad, 'd_gamma': gg.grad, 'd_beta': bb.grad}
        _cache[key] = dict(x=x, gamma=gamma, beta=beta, d_y=d_y, truth=run(torch.float64), torch32=run(torch.float32))
    return _cache[key]


def _kernel(c, rows=None, train=True):
    from rl_games_amd import ops
    x, d_y = c['x'], c['d_y']
    if rows is not None:
        x, d_y = x[:rows].contiguous(), d_y[:rows].contiguous()
    rows, H = x.shape
    y = torch.full_like(x, float('nan'))
    stats = torch.full((rows, 2), float('nan'), device=DEV) if train else None
    ops.rnn_layer_norm_forward(x, c['gamma'], c['beta'], EPS, y, stats)
    if not train:
        return {'y': y}
    nb = ops.rnn_layer_norm_blocks(rows, H)
    assert 1 <= nb <= 256
    d_x = torch.full_like(x, float('nan'))
    pg = torch.full((nb * H,), float('nan'), dtype=torch.float64, device=DEV)
    pb = torch.full((nb * H,), float('nan'), dtype=torch.float64, device=DEV)
    ops.rnn_layer_norm_backward(d_y, x, stats, c['gamma'], d_x, pg, pb, nb)
    d_gamma, d_beta = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    ops.colsum_finalize(pg, nb, H, d_gamma)
    ops.colsum_finalize(pb, nb, H, d_beta)
    return {'y': y, 'stats': stats, 'd_x': d_x, 'd_gamma': d_gamma, 'd_beta': d_beta}


@pytest.mark.parametrize('offset', [0.0, 100.0])
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('H', WIDTHS)
def test_layer_norm_matches_fp64(H, rows, offset):
    """N(0,1) rows and 100 + N(0,1) rows (the offset is what an uncentred variance would not survive): y, d_x and the
    finalised d gamma / d beta."""
    c = _case(H, rows, offset)
    got = _kernel(c)
    for name in ('y', 'd_x', 'd_gamma', 'd_beta'):
        truth = c['truth'][name]
        err_k = (got[name].double() - truth).abs().max().item()
        err_t = (c['torch32'][name].double() - truth).abs().max().item()
        scale = truth.abs().max().item()
        print(f'{name}: kernel {err_k:.3e} torch fp32 {err_t:.3e} scale {scale:.3e}')
        assert err_k <= max(8 * err_t, 2e-6 * scale), (name, err_k, err_t, scale)


@pytest.mark.parametrize('H', WIDTHS)
def test_layer_norm_rows_are_independent(H):
    """The first 37 rows of the 1,029-row launch and the 37-row launch: the same bits, forward and backward."""
    c = _case(H, 1029, 100.0)
    full, part = _kernel(c), _kernel(c, rows=37)
    for name in ('y', 'stats', 'd_x'):
        assert torch.equal(full[name][:37], part[name]), name


@pytest.mark.parametrize('H', WIDTHS)
def test_layer_norm_inference_form_equals_training_form(H):
    c = _case(H, 1029, 0.0)
    assert torch.equal(_kernel(c, train=False)['y'], _kernel(c)['y'])


def test_layer_norm_bad_arguments_raise_without_launching():
    from rl_games_amd import ops
    assert ops.rnn_layer_norm_blocks(64, 100) == 0 and ops.rnn_layer_norm_blocks(0, 64) == 0
    H, rows = 64, 8
    x = torch.zeros(rows, H, device=DEV)
    y = torch.full_like(x, 7.0)
    w = torch.ones(H, device=DEV)
    stats = torch.zeros(rows, 2, device=DEV)
    part = torch.zeros(H, dtype=torch.float64, device=DEV)
    wide = torch.zeros(rows, 100, device=DEV)
    with pytest.raises(RuntimeError):                       # width outside 16 / 32 / 64 / 128
        ops.rnn_layer_norm_forward(wide, torch.ones(100, device=DEV), torch.ones(100, device=DEV), EPS, torch.empty_like(wide))
    with pytest.raises(RuntimeError):                       # no rows
        ops.rnn_layer_norm_forward(x[:0], w, w, EPS, y[:0])
    odd = torch.zeros(rows * H + 4, device=DEV)[1:1 + rows * H].view(rows, H)          # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError):
        ops.rnn_layer_norm_forward(odd, w, w, EPS, y)
    with pytest.raises(RuntimeError):
        ops.rnn_layer_norm_forward(x, w, w, EPS, odd)
    with pytest.raises(ValueError):                         # a required pointer missing
        ops.rnn_layer_norm_forward(x, None, w, EPS, y)
    with pytest.raises(ValueError):
        ops.rnn_layer_norm_backward(x, x, None, w, y, part, part, 1)
    with pytest.raises(RuntimeError):
        ops.rnn_layer_norm_backward(odd, x, stats, w, y, part, part, 1)
    with pytest.raises(RuntimeError):                       # block count outside the launcher's range
        ops.rnn_layer_norm_backward(x, x, stats, w, y, part, part, 0)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                           # nothing ran
