"""GPU: csrc/mlp_chain_d2rl.hip (ops.MlpChainD2rl) against policy.D2RLNet + a linear head on the same weights in fp64
under torch autograd on the CPU.  Exact fp32 products, so the tolerance is tests/test_chain_twin_gpu.py's for that scheme:
per quantity the max-abs error against fp64 is at most the larger of 4 x the error of the same modules run by torch in fp32
and 1e-5 of the tensor's largest magnitude; the ratio error / bound is printed.  chain_net.WeightGrads finishes the gradients from the
kernels' [H | xn] rows and dZ on its exact-product form (its split forms have their bounds in tests/test_weight_grads_gpu.py)."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = 5                                      # head columns: [value | 4 logits]
PAD = 3                                    # rows behind the launch in every buffer: NaN going in, NaN coming out
# (obs, units, act, rows, groups, normaliser on, strided observation view)
CASES = [(3, [8, 4], 'tanh', 1, 0, False, False),
         (17, [64, 64], 'elu', 65, 0, True, False),             # obs off a multiple of 4, ragged last tile
         (98, [256, 128, 64], 'relu', 130, 0, True, False),
         (12, [512, 512, 512, 512], 'elu', 33, 0, False, False),  # the envelope's corner
         (60, [256, 128], 'elu', 16400, 4, True, False),        # G = 4: 256 whole tiles and a ragged one
         (18, [64, 32, 16], 'relu', 40, 0, True, True)]


def _modules(obs, units, act):
    from rl_games_amd.policy import D2RLNet
    torch.manual_seed(obs + sum(units))
    return D2RLNet(obs, units, act), nn.Linear(units[-1], C)


def _inputs(obs, rows):
    g = torch.Generator().manual_seed(rows * 7 + obs)
    x = torch.randn(rows, obs, generator=g) * 2.0 + 0.5
    rms = (torch.randn(obs, generator=g).double() * 0.5, torch.rand(obs, generator=g).double() + 0.5)
    return x, rms, torch.randn(rows, C, generator=g)


def _torch_run(mods, x, rms, d_heads, dtype, device):
    """heads, xn, the head's input and dw; per hidden layer l: in{l} (the Linear's input, [H_{l-1} | xn] for l >= 1), dz, dw, db"""
    net, head = (copy.deepcopy(m).to(device, dtype) for m in mods)
    x0 = x.to(device, dtype)
    if rms is not None:
        x0 = torch.clamp((x0 - rms[0].to(device, dtype)) / torch.sqrt(rms[1].to(device, dtype) + 1e-5), -5.0, 5.0)
    seen = []

    def keep(module, inputs, output):
        output.retain_grad()
        seen.append((inputs[0], output))
    for lin in list(net.linears) + [head]:
        lin.register_forward_hook(keep)
    heads = head(net(x0))
    heads.backward(d_heads.to(device, dtype))
    out = {'heads': heads, 'xn': x0, 'in_head': seen[-1][0], 'dw_head': head.weight.grad}
    for k, (lin, (inp, z)) in enumerate(zip(net.linears, seen)):
        out.update({f'in{k}': inp, f'dz{k}': z.grad, f'dw{k}': lin.weight.grad, f'db{k}': lin.bias.grad})
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _kernel_run(mods, act, x, rms, d_heads, groups, strided):
    from rl_games_amd import chain_net, ops
    net, head = (copy.deepcopy(m).to(DEV) for m in mods)
    lins, rows, in0 = list(net.linears), x.shape[0], x.shape[1]
    widths = [l.out_features for l in lins]
    chain = ops.MlpChainD2rl([(l.weight.data, l.bias.data, act) for l in lins] + [(head.weight.data, head.bias.data, 'None')], DEV)

    def nan(cols, dtype=torch.float32, r=rows + PAD):
        return torch.full((r, cols), float('nan'), dtype=dtype, device=DEV)
    xg = nan(in0 + 7)[:, 5:5 + in0] if strided else nan(in0)
    xg[:rows] = x.to(DEV)
    rg = None if rms is None else tuple(t.to(DEV) for t in rms)
    heads, infer, xn, dh = nan(C), nan(C), nan(in0), nan(C)
    dh[:rows] = d_heads.to(DEV)
    acts, dz = [nan(w + (in0 if k + 1 < len(widths) else 0)) for k, w in enumerate(widths)], [nan(w) for w in widths]
    rv = lambda ts: [t[:rows] for t in ts]                                  # noqa: E731
    chain.forward(xg[:rows], infer[:rows], rms=rg, groups=groups)
    chain.forward(xg[:rows], heads[:rows], act_out=rv(acts), rms=rg, xn_out=xn[:rows], groups=groups)
    assert torch.equal(infer.nan_to_num(7.0), heads.nan_to_num(7.0))       # inference = training forward, PAD rows untouched
    nblk = chain.num_blocks(rows, 1, groups)
    parts = [nan(w, torch.float64, nblk + 1) for w in widths]
    flat = [p[:nblk].view(-1) for p in parts]
    chain.backward(dh[:rows], rv(acts), rv(dz), flat, groups=groups)
    assert all(torch.isnan(p[nblk:]).all() and not torch.isnan(p[:nblk]).any() for p in parts)
    for p in list(net.parameters()) + list(head.parameters()):
        p.grad = torch.full_like(p, float('nan'))
    jobs, colsums = chain_net.trunk_jobs(lins, xn[:rows], rv(acts), rv(dz), flat, nblk)      # (xn: x itself without rms)
    finisher = chain_net.WeightGrads()
    finisher.form = 'exact'
    finisher.finish([(dh[:rows], acts[-1][:rows], head.weight.grad)] + jobs, rows, colsums)
    torch.cuda.synchronize()
    out = {'heads': heads, 'xn': xn, 'in0': xn, 'in_head': acts[-1], 'dw_head': head.weight.grad}
    for k, lin in enumerate(lins):
        out.update({f'dz{k}': dz[k], f'dw{k}': lin.weight.grad, f'db{k}': lin.bias.grad})
        if k > 0:
            out[f'in{k}'] = acts[k - 1]
    return out, chain.groups(rows, 2, groups)


@pytest.mark.parametrize('obs,units,act,rows,groups,norm,strided', CASES)
def test_d2rl_chain_matches_fp64_modules(obs, units, act, rows, groups, norm, strided):
    mods = _modules(obs, units, act)
    x, rms, d_heads = _inputs(obs, rows)
    rms = rms if norm else None
    ref = _torch_run(mods, x, rms, d_heads, torch.float64, 'cpu')
    t32 = _torch_run(mods, x, rms, d_heads, torch.float32, DEV)
    got, ran_groups = _kernel_run(mods, act, x, rms, d_heads, groups, strided)
    assert ran_groups == (groups or 1)
    worst = {}
    for name, have in got.items():
        want, w32 = ref[name], t32[name]
        if have.shape[0] == rows + PAD and not name.startswith(('dw', 'db')):
            assert torch.isnan(have[rows:]).all(), f'{name}: rows behind the launch were written'
            have = have[:rows]
        err, err32 = (have.double().cpu() - want).abs().max().item(), (w32 - want).abs().max().item()
        bound = max(4.0 * err32, 1e-5 * want.abs().max().item())
        worst[name] = round(err / bound, 3) if bound > 0 else float(err > 0)
        assert err <= bound, (name, err, err32, want.abs().max().item())
    print('error / bound', obs, units, act, rows, worst)


def test_d2rl_query_declines_and_the_entries_launch_nothing():
    from rl_games_amd import ops
    from rl_games_amd._lib import HipLibraryError

    def layers(units, d2rl=True, obs=9):
        lins, last = [], obs
        for w in units:
            lins.append(nn.Linear(last, w).to(DEV))
            last = w + (obs if d2rl else 0)
        head = nn.Linear(units[-1], C).to(DEV)
        return [(l.weight.data, l.bias.data, 'elu') for l in lins] + [(head.weight.data, head.bias.data, 'None')]
    assert ops.MlpChainD2rl.supported(layers([64, 32])) == 1
    gamma = torch.ones(64, device=DEV)
    outside = {'1 layer': (layers([32]), None), 'width 516': (layers([516, 516]), None), 'width 6': (layers([6, 6]), None),
               'a layer norm': (layers([64, 32]), [(gamma, gamma, 1e-5), None, None]),
               'a plain shape': (layers([32, 32], d2rl=False), None)}
    x = torch.randn(4, 9, device=DEV)
    for name, (ls, norms) in outside.items():
        assert ops.MlpChainD2rl.supported(ls, norms) == 0, name
        with pytest.raises(NotImplementedError):
            ops.MlpChainD2rl(ls, DEV, norms=norms)
        if norms is None:                    # (the entries see the net alone: a normed trunk is the query's to decline)
            chain = ops.MlpChainD2rl.__new__(ops.MlpChainD2rl)
            chain._state(ls, DEV, None, None)
            heads = torch.full((4, C), float('nan'), device=DEV)
            for call in (lambda: chain.forward(x, heads), lambda: chain.backward(heads, [heads] * (len(ls) - 1), [heads] * (len(ls) - 1))):
                with pytest.raises(HipLibraryError):
                    call()
            torch.cuda.synchronize()
            assert torch.isnan(heads).all(), name
