"""CPU: the formulas csrc/rnn_value_tail.hip implements - the value column behind the recurrent layer of a central value
critic, the clipped value loss of `CentralValueTrain.calc_loss` (rl_games/algos_torch/central_value.py:262-276,
common_losses.py:16-29) and its backward down to the features, the head's weight and bias - stated in fp64 and held to
autograd through nn.Linear(H, 1), as tests/test_rnn_layer_norm_cpu.py does for its kernel."""
import pytest
import torch


def value_tail(feat, w, b, old_values, returns, e_clip, clip_value, mask=None):
    """values = b + feat w; the row loss and gradient of value_loss_row (csrc/value_loss_row.hpp): torch.max's tie rule,
    clamp's inclusive range; mean over the rows or masked mean over max(sum(mask), 1).  Returns values, loss, d_values,
    d_feat, d_w, d_b."""
    v = b + feat @ w
    if clip_value:
        delta = v - old_values
        d1, d2 = v - returns, old_values + delta.clamp(-e_clip, e_clip) - returns
        c1, c2 = d1 * d1, d2 * d2
        c = torch.maximum(c1, c2)
        inside = ((delta >= -e_clip) & (delta <= e_clip)).to(v.dtype)
        g = torch.where(c1 > c2, 2 * d1, torch.where(c2 > c1, 2 * d2 * inside, 0.5 * (2 * d1) + 0.5 * (2 * d2 * inside)))
    else:
        d = returns - v
        c, g = d * d, -2 * d
    m = torch.ones_like(v) if mask is None else mask
    denom = float(v.numel()) if mask is None else max(float(mask.sum()), 1.0)
    d_values = g * (m / denom)
    return v, (c * m).sum() / denom, d_values, d_values[:, None] * w[None, :], d_values @ feat, d_values.sum()


def reference_loss(values, old_values, returns, e_clip, clip_value, mask):
    """common_losses.critic_loss + torch_ext.apply_masks as the reference writes them."""
    if clip_value:
        clipped = old_values + (values - old_values).clamp(-e_clip, e_clip)
        c = torch.max((values - returns) ** 2, (clipped - returns) ** 2)
    else:
        c = (returns - values) ** 2
    if mask is None:
        return c.mean()
    return (c * mask).sum() / mask.sum()


@pytest.mark.parametrize('H', [16, 32, 64, 128])
@pytest.mark.parametrize('clip_value', [False, True])
@pytest.mark.parametrize('masked', [False, True])
def test_value_tail_formulas_match_autograd_fp64(H, clip_value, masked):
    g = torch.Generator().manual_seed(H * 4 + 2 * clip_value + masked)
    rows, e_clip = 37, 0.2
    lin = torch.nn.Linear(H, 1).double()
    feat = torch.randn(rows, H, generator=g, dtype=torch.float64).requires_grad_(True)
    with torch.no_grad():
        v0 = lin(feat)[:, 0]
    # inside the clip range, outside on both sides, and returns on either side of both branches
    old_values = v0 + torch.randn(rows, generator=g, dtype=torch.float64) * 0.4
    returns = v0 + torch.randn(rows, generator=g, dtype=torch.float64)
    mask = (torch.rand(rows, generator=g) < 0.7).double() if masked else None
    loss = reference_loss(lin(feat)[:, 0], old_values, returns, e_clip, clip_value, mask)
    loss.backward()
    v, got_loss, d_values, d_feat, d_w, d_b = value_tail(feat.detach(), lin.weight.detach()[0], lin.bias.detach()[0],
                                                         old_values, returns, e_clip, clip_value, mask)
    if clip_value:
        outside = (v - old_values).abs() > e_clip
        assert outside.any() and (~outside).any()
    for name, got, ref in (('values', v, v0), ('loss', got_loss, loss.detach()), ('d_feat', d_feat, feat.grad),
                           ('d_w', d_w, lin.weight.grad[0]), ('d_b', d_b, lin.bias.grad[0])):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12, (name, err)
    # d_values is what d_feat / d_w / d_b are made of: d_b = sum d_values pins its scale, d_feat its rows
    assert (d_values[:, None] * lin.weight.detach() - feat.grad).abs().max().item() <= 1e-12


def test_value_tail_ties_split_the_gradient_as_torch_max_does():
    """old_values == values: both branches are equal, torch.max hands each half of the gradient."""
    H, rows, e_clip = 16, 9, 0.2
    g = torch.Generator().manual_seed(5)
    lin = torch.nn.Linear(H, 1).double()
    feat = torch.randn(rows, H, generator=g, dtype=torch.float64).requires_grad_(True)
    with torch.no_grad():
        old_values = lin(feat)[:, 0].clone()
    returns = torch.randn(rows, generator=g, dtype=torch.float64)
    reference_loss(lin(feat)[:, 0], old_values, returns, e_clip, True, None).backward()
    _, _, _, d_feat, d_w, d_b = value_tail(feat.detach(), lin.weight.detach()[0], lin.bias.detach()[0], old_values,
                                           returns, e_clip, True)
    assert (d_feat - feat.grad).abs().max().item() <= 1e-12
    assert (d_w - lin.weight.grad[0]).abs().max().item() <= 1e-12 and abs(d_b - lin.bias.grad[0]).item() <= 1e-12
