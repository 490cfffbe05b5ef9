"""CPU: the formulas csrc/rnn_layer_norm.hip implements - layer normalisation behind the recurrent layer
(`rnn: {layer_norm: True}`, rl_games/algos_torch/network_builder.py:447-500) - stated in fp64 and held to autograd
through torch.nn.LayerNorm, as tests/test_gru_cpu.py does for the GRU cell."""
import pytest
import torch


def layer_norm_forward(x, gamma, beta, eps):
    """y = (x - mean) * rstd * gamma + beta: the mean first, then the biased variance from the centred values,
    rstd = 1 / sqrt(var + eps).  Returns y and the per-row (mean, rstd) the backward reads."""
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return d * rstd * gamma + beta, torch.cat([mean, rstd], 1)


def layer_norm_backward(d_y, x, stats, gamma):
    """g = d_y * gamma, xh = (x - mean) * rstd:  d_x = rstd * (g - mean_H(g) - xh * mean_H(g * xh)),
    d gamma = sum_rows d_y * xh, d beta = sum_rows d_y."""
    mean, rstd = stats[:, :1], stats[:, 1:]
    g = d_y * gamma
    xh = (x - mean) * rstd
    d_x = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return d_x, (d_y * xh).sum(0), d_y.sum(0)


@pytest.mark.parametrize('H', [16, 32, 64, 128])
@pytest.mark.parametrize('offset', [0.0, 100.0])
def test_layer_norm_formulas_match_autograd_fp64(H, offset):
    g = torch.Generator().manual_seed(H + int(offset))
    rows = 37
    ln = torch.nn.LayerNorm(H).double()
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.5 * torch.randn(H, generator=g, dtype=torch.float64))
        ln.bias.copy_(torch.randn(H, generator=g, dtype=torch.float64))
    x = (offset + torch.randn(rows, H, generator=g, dtype=torch.float64)).requires_grad_(True)
    d_y = torch.randn(rows, H, generator=g, dtype=torch.float64)
    want = ln(x)
    want.backward(d_y)
    y, stats = layer_norm_forward(x.detach(), ln.weight.detach(), ln.bias.detach(), ln.eps)
    d_x, d_gamma, d_beta = layer_norm_backward(d_y, x.detach(), stats, ln.weight.detach())
    for name, got, ref in (('y', y, want.detach()), ('d_x', d_x, x.grad), ('d_gamma', d_gamma, ln.weight.grad),
                           ('d_beta', d_beta, ln.bias.grad)):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12, (name, err)
