"""GPU: csrc/mlp_chain_twin.hip - separate actor / critic MLPs as one twin-trunk chain (ops.MlpChainTwin) - against the
same torch modules evaluated in fp64 on the CPU (autograd for the backward).  The kernels run exact fp32 products, so the
tolerance is that of tests/test_chain_ln_gpu.py for the same product form: per quantity the max-abs error against fp64 may
be at most the larger of 4 x the error of the same modules run by torch in fp32 and 1e-5 of the tensor's largest
magnitude; the ratio error / bound is printed.  Rows: 1, tile - 1, tile + 1, 2 tile + 2 for a tile of 16 G rows."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ACTS = {'relu': nn.ReLU, 'elu': nn.ELU, 'tanh': nn.Tanh}
TRUNKS = {'equal': ([32, 16], [32, 16]), 'unequal': ([64], [32, 16, 8]), 'widest': ([512], [512, 64])}
A = 5                                      # mu columns
PAD = 3                                    # rows behind the launch in every buffer: NaN going in, NaN coming out
CASES = [(t, g) for t in ('equal', 'unequal') for g in (1, 2, 4)] + [('widest', 1), ('widest', 2)]   # (512 at G = 4: no LDS)


def _modules(obs, trunks, act):
    torch.manual_seed(obs + sum(trunks[0]) + 3 * sum(trunks[1]))
    out = []
    for hidden, cols in zip(trunks, (A, 1)):
        lins, last = [], obs
        for w in hidden:
            lins.append(nn.Linear(last, w))
            nn.init.normal_(lins[-1].bias, 0.0, 0.3)
            last = w
        out.append((lins, nn.Linear(last, cols)))
    return out


def _inputs(obs, rows):
    g = torch.Generator().manual_seed(rows * 7 + obs)
    x = torch.randn(rows, obs, generator=g) * 2.0 + 0.5
    rms = (torch.randn(obs, generator=g).double() * 0.5, torch.rand(obs, generator=g).double() + 0.5)
    return x, rms, torch.randn(rows, A, generator=g), torch.randn(rows, 1, generator=g)


def _torch_run(mods, act, x, rms, d_heads, dtype, device):
    """heads [rows, 1 + A] = [value | mu], xn, and per trunk t and layer k: act / dz (the weight gradients' operands)."""
    h0 = x.to(device, dtype)
    h0 = torch.clamp((h0 - rms[0].to(device, dtype)) / torch.sqrt(rms[1].to(device, dtype) + 1e-5), -5.0, 5.0)
    out, heads = {'xn': h0}, []
    for t, ((lins, head), d) in enumerate(zip(mods, d_heads)):
        h, zs = h0, []
        for k, lin in enumerate(lins):
            z = copy.deepcopy(lin).to(device, dtype)(h)
            z.retain_grad()
            zs.append(z)
            out[f'act{t}{k}'] = h = ACTS[act]()(z)
        heads.append(copy.deepcopy(head).to(device, dtype)(h))
        heads[-1].backward(d.to(device, dtype))
        for k, z in enumerate(zs):
            out[f'dz{t}{k}'] = z.grad
    out['heads'] = torch.cat([heads[1], heads[0]], 1)
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _chain(mods, act):
    from rl_games_amd import ops
    dev = [([copy.deepcopy(l).to(DEV) for l in lins], copy.deepcopy(head).to(DEV)) for lins, head in mods]
    layers = [[(l.weight.data, l.bias.data, act) for l in lins] + [(head.weight.data, head.bias.data, 'None')] for lins, head in dev]
    return ops.MlpChainTwin(layers[0], layers[1], DEV), [[l.out_features for l in lins] for lins, _ in dev]


def _kernel_run(mods, act, x, rms, d_heads, groups=0, train=True, fold=None):
    """The same quantities from the kernels (+ dbias per layer); every buffer has PAD NaN rows behind the launch's."""
    from rl_games_amd import ops
    chain, widths = _chain(mods, act)
    rows = x.shape[0]

    def nan(cols, dtype=torch.float32, r=rows + PAD):
        return torch.full((r, cols), float('nan'), dtype=dtype, device=DEV)
    xg = nan(x.shape[1])
    xg[:rows] = x.to(DEV)
    rg = tuple(t.to(DEV) for t in rms)
    heads, xn = nan(1 + A), nan(x.shape[1])
    if not train:
        chain.forward(xg[:rows], heads[:rows, 1:], heads[:rows, :1], rms=rg, groups=groups)
        return {'heads': heads}
    acts, dz = ([[nan(w) for w in ws] for ws in widths] for _ in range(2))
    dh = [nan(A), nan(1)]
    for d, src in zip(dh, d_heads):
        d[:rows] = src.to(DEV)
    rv = lambda ts: [t[:rows] for t in ts]                                  # noqa: E731
    chain.forward(xg[:rows], heads[:rows, 1:], heads[:rows, :1], act_out=[rv(a) for a in acts], rms=rg, xn_out=xn[:rows],
                  groups=groups, rms_fold=fold)
    nblk = chain.num_blocks(rows, 1, groups)
    parts = [[nan(w, torch.float64, nblk + 1) for w in ws] for ws in widths]
    chain.backward(dh[0][:rows], dh[1][:rows], [rv(a) for a in acts], [rv(d) for d in dz],
                   [[p[:nblk].view(-1) for p in ps] for ps in parts], groups=groups)
    out = {'heads': heads, 'xn': xn}
    for t, ws in enumerate(widths):
        for k, w in enumerate(ws):
            out[f'act{t}{k}'], out[f'dz{t}{k}'] = acts[t][k], dz[t][k]
            assert torch.isnan(parts[t][k][nblk:]).all() and not torch.isnan(parts[t][k][:nblk]).any()
            out[f'dbias{t}{k}'] = torch.empty(w, device=DEV)
            ops.colsum_finalize(parts[t][k][:nblk].view(-1), nblk, w, out[f'dbias{t}{k}'])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('obs', [3, 17, 32])
@pytest.mark.parametrize('act', ['elu', 'relu', 'tanh'])
@pytest.mark.parametrize('trunks,groups', CASES)
def test_twin_chain_matches_fp64_modules(trunks, groups, act, obs):
    tile = 16 * groups
    mods = _modules(obs, TRUNKS[trunks], act)
    x, rms, d_mu, d_v = _inputs(obs, 2 * tile + 2)
    ref = _torch_run(mods, act, x, rms, (d_mu, d_v), torch.float64, 'cpu')          # once: a row's reference is the row's
    t32 = _torch_run(mods, act, x, rms, (d_mu, d_v), torch.float32, DEV)
    worst = {}
    for rows in (1, tile - 1, tile + 1, 2 * tile + 2):
        got = _kernel_run(mods, act, x[:rows], rms, (d_mu[:rows], d_v[:rows]), groups)
        inf = _kernel_run(mods, act, x[:rows], rms, None, groups, train=False)
        assert torch.equal(inf['heads'][:rows], got['heads'][:rows]) and torch.isnan(inf['heads'][rows:]).all()
        for name, have in got.items():
            if name.startswith('dbias'):
                want, w32 = (r['dz' + name[5:]][:rows].sum(0) for r in (ref, t32))
            else:
                assert torch.isnan(have[rows:]).all(), f'{name}: rows behind the launch were written'
                want, w32, have = ref[name][:rows], t32[name][:rows], have[:rows]
            err, err32 = (have.double().cpu() - want).abs().max().item(), (w32 - want).abs().max().item()
            bound = max(4.0 * err32, 1e-5 * want.abs().max().item())
            worst[name] = max(worst.get(name, 0.0), round(err / bound, 3) if bound > 0 else float(err > 0))
            assert err <= bound, (name, rows, err, err32, want.abs().max().item())
    print('error / bound', trunks, groups, act, obs, worst)


def test_twin_chain_rows_do_not_see_their_neighbours_and_runs_repeat():
    mods = _modules(17, TRUNKS['unequal'], 'elu')
    x, rms, d_mu, d_v = _inputs(17, 77)
    a = _kernel_run(mods, 'elu', x, rms, (d_mu, d_v), 2)
    b = _kernel_run(mods, 'elu', x, rms, (d_mu, d_v), 2)
    one = _kernel_run(mods, 'elu', x[37:38], rms, (d_mu[37:38], d_v[37:38]), 1)
    for k in a:
        assert torch.equal(a[k].nan_to_num(7.0), b[k].nan_to_num(7.0)), k
        if not k.startswith('dbias'):
            assert torch.equal(one[k][0], a[k][37]), k


def test_twin_chain_folds_the_minibatch_statistics_before_it_normalises():
    """rms_fold: the heads are those of a plain forward on the state the launch published, and that state is the Chan
    merge of the minibatch's moments (running_mean_std.py:55-67) in fp64."""
    from rl_games_amd import ops
    mods = _modules(17, TRUNKS['equal'], 'elu')
    x, rms, d_mu, d_v = _inputs(17, 50)
    table, _ = ops.column_moments_segments(x.to(DEV), 50)
    count = torch.tensor(20, dtype=torch.int64, device=DEV)
    new = (torch.empty(17, dtype=torch.float64, device=DEV), torch.empty(17, dtype=torch.float64, device=DEV), torch.empty_like(count))
    got = _kernel_run(mods, 'elu', x, rms, (d_mu, d_v), fold=(table[0], count, *new))
    again = _kernel_run(mods, 'elu', x, (new[0].cpu(), new[1].cpu()), (d_mu, d_v))
    assert torch.equal(got['heads'][:50], again['heads'][:50]) and torch.equal(got['xn'][:50], again['xn'][:50])
    bm, bv = x.mean(0).double(), x.var(0, unbiased=False).double()
    delta, tot = bm - rms[0], 70.0
    mean = rms[0] + delta * 50.0 / tot
    var = (rms[1] * 20.0 + bv * 50.0 + delta * delta * 20.0 * 50.0 / tot) / tot
    assert int(new[2]) == 70
    assert torch.allclose(new[0].cpu(), mean, rtol=1e-6, atol=1e-7) and torch.allclose(new[1].cpu(), var, rtol=1e-6, atol=1e-7)


def test_twin_chain_query_declines_what_the_kernels_do_not_take():
    from rl_games_amd import ops

    def layers(hidden, cols, act='elu'):
        lins, last = [], 9
        for w in hidden:
            lins.append(nn.Linear(last, w).to(DEV))
            last = w
        head = nn.Linear(last, cols).to(DEV)
        return [(l.weight.data, l.bias.data, act) for l in lins] + [(head.weight.data, head.bias.data, 'None')]
    ok = ops.MlpChainTwin.supported
    assert ok(layers([64, 32], A), layers([32], 1)) == 1
    assert ok(layers([256, 128, 64], A), layers([256, 128, 64], 1), rows=32768, direction=2) == 2       # 4 groups: > 80 KiB
    gamma = torch.ones(64, device=DEV)
    outside = {'a hidden width of 18': (layers([18], A), layers([32], 1)),
               'five layers': (layers([32] * 5, A), layers([32], 1)),
               'two activation kinds': (layers([32], A), layers([32], 1, 'tanh')),
               'two value columns': (layers([32], A), layers([32], 2)),
               'a layer norm': (layers([64], A), layers([32], 1), ([(gamma, gamma, 1e-5), None], None))}
    for name, args in outside.items():
        assert ok(*args) == 0, name
        with pytest.raises(NotImplementedError):
            ops.MlpChainTwin(args[0], args[1], DEV, norms=args[2] if len(args) > 2 else (None, None))
