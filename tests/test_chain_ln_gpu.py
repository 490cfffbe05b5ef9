"""GPU: csrc/mlp_chain_ln.hip - the fused chain for trunks whose layers end in a layer norm (ops.MlpChainLn) - against
the same torch modules evaluated in fp64 on the CPU (autograd for the backward).  Tolerance per quantity: the kernel's
max-abs error against fp64 may be at most the larger of 4 x the error of the same modules run by torch in fp32 and 1e-5
of the tensor's largest magnitude; the ratio error / bound is printed per quantity."""
import copy
import ctypes

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ACTS = {'relu': nn.ReLU, 'elu': nn.ELU, 'tanh': nn.Tanh}
W_TINY, W_MID, W_WIDE, W_SMAC = (9, [20], 3), (33, [64, 36], 6), (12, [272, 132], 15), (98, [512, 256], 15)
PAD = 3                                    # rows behind the launch in every output buffer: they must stay NaN


def _modules(widths, act, first_only, dead):
    torch.manual_seed(sum(widths[1]) + widths[0])
    n_in, hidden, head = widths
    groups, last = [], n_in
    for k, w in enumerate(hidden):
        ln = nn.LayerNorm(w) if (k == 0 or not first_only) else None
        if ln is not None:
            nn.init.normal_(ln.weight, 1.0, 0.5)
            nn.init.normal_(ln.bias, 0.0, 0.5)
            ln.weight.data[w // 3] = 0.0                            # one gamma element exactly 0
        groups.append((nn.Linear(last, w), ACTS[act](), ln))
        nn.init.normal_(groups[-1][0].bias, 0.0, 0.3)
        last = w
    if dead:                                                        # positive weights, bias -5: a zero input row is dead
        groups[0][0].weight.data.abs_()
        groups[0][0].bias.data.fill_(-5.0)
    return groups, nn.Linear(last, head)


def _torch_run(groups, head, x, rms, d_heads, dtype, device):
    """The quantities the kernels produce, from the modules themselves in `dtype` on `device`."""
    groups = [tuple(None if m is None else copy.deepcopy(m).to(device, dtype) for m in g) for g in groups]
    head = copy.deepcopy(head).to(device, dtype)
    h = x.to(device, dtype)
    if rms is not None:
        mean, var = (t.to(device) for t in rms)
        h = torch.clamp((h - mean.to(dtype)) / torch.sqrt(var.to(dtype) + 1e-5), -5.0, 5.0)
    out = {'xn': h}
    zs = []
    for k, (lin, act, ln) in enumerate(groups):
        z = lin(h)
        z.retain_grad()
        zs.append(z)
        a = act(z)
        if ln is not None:
            out[f'pre{k}'] = a
            mu, var = a.mean(1), a.var(1, unbiased=False)
            out[f'stats{k}'] = torch.stack([mu, 1.0 / torch.sqrt(var + ln.eps)], 1)
            a = ln(a)
        out[f'act{k}'] = h = a
    out['heads'] = head(h)
    out['heads'].backward(d_heads.to(device, dtype))
    for k, (lin, act, ln) in enumerate(groups):
        out[f'dz{k}'], out[f'dbias{k}'] = zs[k].grad, lin.bias.grad
        if ln is not None:
            out[f'dgamma{k}'], out[f'dbeta{k}'] = ln.weight.grad, ln.bias.grad
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _kernel_run(groups, head, x, rms, d_heads, act, groups_req=0, train=True):
    from rl_games_amd import ops
    mods = [tuple(None if m is None else copy.deepcopy(m).to(DEV) for m in g) for g in groups]
    hd = copy.deepcopy(head).to(DEV)
    layers = [(lin.weight.data, lin.bias.data, act) for lin, _, _ in mods] + [(hd.weight.data, hd.bias.data, 'None')]
    norms = [None if ln is None else (ln.weight.data, ln.bias.data, ln.eps) for _, _, ln in mods] + [None]
    chain = ops.MlpChainLn(layers, norms, DEV)
    rows = x.shape[0]

    def nan(cols, dtype=torch.float32, r=rows + PAD):
        return torch.full((r, cols), float('nan'), dtype=dtype, device=DEV)
    widths = [lin.out_features for lin, _, _ in mods]
    xg, dh = x.to(DEV), torch.cat([d_heads, torch.zeros(PAD, d_heads.shape[1])]).to(DEV)
    rg = None if rms is None else tuple(t.to(DEV) for t in rms)
    heads, xn = nan(hd.out_features), nan(x.shape[1])
    acts = [nan(w) for w in widths]
    pre = [None if n is None else nan(w) for n, w in zip(norms, widths)]
    stats = [None if n is None else nan(2) for n in norms[:-1]]
    rv = lambda ts: [None if t is None else t[:rows] for t in ts]            # noqa: E731
    if not train:
        chain.forward(xg, heads[:rows], rms=rg, groups=groups_req)
        return {'heads': heads}
    chain.forward(xg, heads[:rows], act_out=rv(acts), pre_out=rv(pre), stats=rv(stats), rms=rg,
                  xn_out=None if rms is None else xn[:rows], groups=groups_req)
    nblk = chain.num_blocks(rows, 1, groups_req)
    dz = [nan(w) for w in widths]
    parts = [[None if (n is None and kind) else nan(w, torch.float64, nblk + 1) for n, w in zip(norms, widths)]
             for kind in (0, 1, 1)]
    chain.backward(dh[:rows], rv(acts), rv(pre), rv(stats), rv(dz), *[[None if p is None else p[:nblk].view(-1) for p in ps]
                                                                      for ps in parts], groups=groups_req)
    out = {'heads': heads, 'xn': xn if rms is not None else xg}
    for k, w in enumerate(widths):
        out[f'act{k}'], out[f'dz{k}'] = acts[k], dz[k]
        if pre[k] is not None:
            out[f'pre{k}'], out[f'stats{k}'] = pre[k], stats[k]
        for name, ps in zip(('dbias', 'dgamma', 'dbeta'), parts):
            if ps[k] is not None:
                assert torch.isnan(ps[k][nblk:]).all() and not torch.isnan(ps[k][:nblk]).any(), name
                out[f'{name}{k}'] = torch.empty(w, device=DEV)
                ops.colsum_finalize(ps[k][:nblk].view(-1), nblk, w, out[f'{name}{k}'])
    torch.cuda.synchronize()
    return out


def _inputs(widths, rows, rms_kind, dead):
    g = torch.Generator().manual_seed(rows * 7 + widths[0])
    x = torch.randn(rows, widths[0], generator=g) * 2.0 + 0.5
    rms = None
    if rms_kind is not None:
        rms = (torch.randn(widths[0], generator=g).double() * 0.5, torch.rand(widths[0], generator=g).double() + 0.5)
        if rms_kind == 'zero_var':
            rms[1][widths[0] // 2] = 0.0
    if dead:
        x = x.abs() + 1.0
        x[min(5, rows - 1)] = 0.0
    return x, rms, torch.randn(rows, widths[2], generator=g)


CASES = ([(w, r, 'relu', False, 'rms', False, 0) for w in (W_TINY, W_MID, W_WIDE, W_SMAC) for r in (1, 16, 17, 77, 200)]
         + [(W_MID, 77, a, False, 'rms', False, 0) for a in ('elu', 'tanh')]
         + [(W_MID, 77, 'relu', False, 'rms', False, g) for g in (1, 2, 4)]
         + [(W_SMAC, 77, 'relu', False, 'rms', False, 2), (W_WIDE, 77, 'relu', False, 'rms', False, 4)]   # several k-batches and blocks a wave at G > 1
         + [(W_MID, 77, 'relu', True, 'rms', False, 0), (W_WIDE, 200, 'relu', True, 'rms', False, 0),
            (W_MID, 77, 'relu', False, None, False, 0), (W_MID, 77, 'relu', False, 'zero_var', False, 0),
            (W_MID, 77, 'relu', False, None, True, 0)])


@pytest.mark.parametrize('widths,rows,act,first_only,rms_kind,dead,groups', CASES)
def test_chain_ln_matches_fp64_modules(widths, rows, act, first_only, rms_kind, dead, groups):
    mods, head = _modules(widths, act, first_only, dead)
    x, rms, d_heads = _inputs(widths, rows, rms_kind, dead)
    ref = _torch_run(mods, head, x, rms, d_heads, torch.float64, 'cpu')
    t32 = _torch_run(mods, head, x, rms, d_heads, torch.float32, DEV)
    got = _kernel_run(mods, head, x, rms, d_heads, act, groups)
    assert set(got) == set(ref)
    if dead:                                                        # variance 0: rstd = 1 / sqrt(eps), y = beta
        r = min(5, rows - 1)
        assert torch.equal(got['pre0'][r], torch.zeros_like(got['pre0'][r]))
        assert torch.equal(got['act0'][r].cpu(), mods[0][2].bias.data)
        assert all(torch.isfinite(got[f'dz{k}'][r]).all() for k in range(len(mods)))
    worst = {}
    for name, want in ref.items():
        have = got[name]
        if have.dim() == 2 and have.shape[0] == rows + PAD:
            assert torch.isnan(have[rows:]).all(), f'{name}: rows behind the launch were written'
            have = have[:rows]
        have = have.double().cpu()
        err, err32 = (have - want).abs().max().item(), (t32[name] - want).abs().max().item()
        bound = max(4.0 * err32, 1e-5 * want.abs().max().item())
        worst[name] = round(err / bound, 3) if bound > 0 else float(err > 0)
        assert err <= bound, (name, err, err32, want.abs().max().item())
    print('error / bound', widths, rows, act, worst)


def test_chain_ln_bit_properties():
    """Plain equalities: the inference form's heads are the training form's, two runs agree bit for bit, and row 5
    computed alone has the bits it has inside the 77-row launch - forward and backward."""
    mods, head = _modules(W_MID, 'relu', False, False)
    x, rms, d_heads = _inputs(W_MID, 77, 'rms', False)
    a = _kernel_run(mods, head, x, rms, d_heads, 'relu')
    b = _kernel_run(mods, head, x, rms, d_heads, 'relu')
    for k in a:
        assert torch.equal(a[k].nan_to_num(7.0), b[k].nan_to_num(7.0)), k
    inf = _kernel_run(mods, head, x, rms, d_heads, 'relu', train=False)
    assert torch.equal(inf['heads'][:77], a['heads'][:77]) and torch.isnan(inf['heads'][77:]).all()
    one = _kernel_run(mods, head, x[5:6], rms, d_heads[5:6], 'relu')
    for k in ('heads', 'act0', 'act1', 'pre0', 'pre1', 'stats0', 'stats1', 'dz0', 'dz1'):
        assert torch.equal(one[k][0], a[k][5]), k


def test_chain_ln_envelope_and_unsupported_fields():
    from rl_games_amd import _lib, ops
    lib = _lib.load()
    assert ctypes.sizeof(_lib.ChainLn) == 64

    def groups(hidden, rows=77, direction=2):
        n = len(hidden) + 1
        ins, outs = (ctypes.c_int * n)(33, *hidden), (ctypes.c_int * n)(*hidden, 6)
        return lib.rlg_mlp_chain_ln_groups(n, ins, outs, rows, direction)
    assert groups([64, 36]) == 1 and groups([64, 36], 100000) == 4
    assert groups([512, 256], 100000) == 2 and groups([512, 256], 100000, 1) == 2      # the SMAC widths: G < 4
    assert groups([18]) == 0 and groups([64, 18], direction=1) == 0
    assert groups([16384]) == 0 and groups([4] * 8) == 0
    mods, head = _modules(W_TINY, 'relu', False, False)
    lin, _, ln = (m.to(DEV) for m in mods[0])
    hd = head.to(DEV)
    chain = ops.MlpChainLn([(lin.weight.data, lin.bias.data, 'relu'), (hd.weight.data, hd.bias.data, 'None')],
                           [(ln.weight.data, ln.bias.data, ln.eps), None], DEV)
    x, heads, buf = torch.zeros(4, 9, device=DEV), torch.zeros(4, 3, device=DEV), torch.zeros(64, device=DEV)
    launch, stream = _lib.ChainLaunch(4, 0), ops._stream(x)
    ref = ctypes.byref
    for field in ('rms_batch_or_null', 'weight_form_or_null', 'pack_backward_planes_or_null'):
        fwd = chain._forward_args(x, [None, heads], None, 1e-5, None, None)
        setattr(fwd, field, buf.data_ptr())
        assert lib.rlg_mlp_chain_ln_forward(ref(chain._net), ref(fwd), ref(chain._ln_args(None, None)), ref(launch), stream) == 801
    acts, dz = [torch.zeros(4, 20, device=DEV)], [torch.zeros(4, 20, device=DEV)]
    loss = _lib.PpoLossDesc()
    for field, value in (('ppo_loss_or_null', ctypes.addressof(loss)), ('weight_form_or_null', buf.data_ptr()),
                         ('maxima_or_null', buf.data_ptr())):
        bwd = chain._backward_args(heads, acts, dz, None, None)
        setattr(bwd, field, value)
        lnd = chain._ln_args(acts, [torch.zeros(4, 2, device=DEV)])
        assert lib.rlg_mlp_chain_ln_backward(ref(chain._net), ref(bwd), ref(lnd), ref(launch), stream) == 801
