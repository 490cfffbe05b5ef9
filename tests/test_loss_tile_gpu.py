"""The PPO loss tile (csrc/ppo_loss_tile.hpp) in every launch that runs it, at every option and at the widths where its two
forms change, against the fp64 oracle and against the stand-alone loss kernel.

Only the loss is under test: what a launch makes of d heads (dZ, bias sums) has its own tests (test_mlp_chain_gpu.py).  The
reference is oracle.ppo_oracle.distribution_loss_and_grads in fp64 on the fp32 mu / values the launch itself consumed
(the heads are copied to the host; for the one-launch steps they are what the launch's own forward half wrote), so it does
not depend on the product scheme of the network in front of the tile.

Hosts (HOSTS below), the instantiation ppo_loss_tile<rows, threads> each pins, and what selects it.  "asserted": a
predicate of the library checked before / behind the launch; "shape rule": nothing the library exposes tells the two
apart, the case is built so that the rule in the code takes it.

  standalone16      <16,256>  ops.ppo_loss_fused, mb <= 8192; asserted: ops.ppo_loss_blocks(mb) == ceil(mb / 16)
  standalone64      <64,256>  ops.ppo_loss_fused, mb > 8192;  asserted: ops.ppo_loss_blocks(mb) == ceil(mb / 64)
  exact_g1_pipe     <16,512>  mlp_chain_bwd_pipe_kernel: backward(split_products=False); asserted: _route == 'exact',
                              groups == 1; shape rule: chain_rows16_status == 0 (hidden widths 64, 32: multiples of 4,
                              16-byte aligned H / dZ rows) takes the pipelined kernel, always 8 waves
  exact_g1_unit     <16,512>  mlp_chain_bwd_kernel<1, 8>: as above; shape rule: a hidden width of 30 (not a multiple of 4)
                              fails chain_rows16_status -> unit-structured kernel; 4 workgroups <= kChainWideBlocks = 384
                              -> 8 waves
  exact_g1_unit_4w  <16,256>  mlp_chain_bwd_kernel<1, 4>: as exact_g1_unit with 386 workgroups > kChainWideBlocks -> 4 waves
  exact_g2          <32,256>  mlp_chain_bwd_kernel<2, 4>: backward(groups=2, split_products=False); asserted: groups == 2
  exact_g4          <64,256>  mlp_chain_bwd_kernel<4, 4>: backward(groups=4, split_products=False); asserted: groups == 4
  split_handoff     <64,512>  mlp_chain_bwd_bx_kernel: backward(groups=4); asserted: split_products(rows, 1, 4), and behind the
                              launch gradient_maxima(rows) with 64 rows per entry (only that kernel leaves them); shape
                              rule: d heads laid out value first (d_values == d_out, d_mu == d_out + 1) and A <= 32 ->
                              d heads handed to the prologue in LDS
  split_nohandoff   <64,512>  as above with the heads laid out mu first, value last: d_mu == d_out -> no hand-off, the
                              prologue re-reads the d heads the tile stored to global memory (at A > 32 both split hosts
                              take this branch: the tile form has no hand-off)
  lean_bwd          <16,512>  mlp_chain_bwd_lean_kernel (plain tile): backward(); asserted: lean_used(rows, 1), and behind
                              the launch gradient_maxima(rows) with 16 rows per entry (only the lean kernels leave them)
  step_pipe         <16,512>  mlp_chain_step_pipe_kernel (quad_load before the forward, quad_run behind it): MlpChain.step
                              with the lean kernels off; asserted: _route == 'exact' both ways, step(...) is True
  step_lean         <16,512>  mlp_chain_step_lean_kernel (preloaded quad form): asserted: lean_used both ways, step(...) is
                              True

Rows per host: `ragged` = three full tiles + 5 rows (the 4-wave and the 64-row stand-alone hosts: the smallest count
their shape rule admits + a tile + 5), `full` = exactly one tile, `one_*` = one row.  The stand-alone 64-row kernel and the
4-wave kernel cannot run one tile: their `full` is a whole number of tiles, their `one_*` a last tile of one row.  A single
row lies in one region of the clip range only, so it runs three times: ratio below, inside and above [1 - e, 1 + e].

Every host meets every option set at A = 21 and every width of WIDTHS under `bound`; the hosts whose tile form has
remainder loops (rows x A > 8 x threads: <64,256> from A = 33, <64,512> from A = 65) also run A = 65 under `bound` and
`masked`, and A = 66 under `bound`: at A = 65 the 64 elements <64,512> leaves to its remainder loop are columns 1 .. 64
of the tile's last row, none of them behind a wrap of advance() to column 0, and with an odd A (LDS row stride A | 1 = A)
element (r, A) is element (r + 1, 0) - a wrap that comes one step late goes unseen there; at A = 66 the loop holds
128 elements, one of them reached by a wrap to column 0, in rows of stride 67.  The one-launch steps decline A > 32:
asserted False, nothing written.

Criteria.  Per-row outputs (d mu, d value, the mu / sigma write-back) bit-equal to the stand-alone kernel's on the same
inputs - for the 64-row stand-alone kernel itself: to the 16-row kernel run on chunks of at most 8,192 rows with the
minibatch's denominator passed as mask sum (an all-ones mask multiplies by 1.0: the same bits).  Against the fp64 oracle:
the criteria of test_ops_gpu.py::test_ppo_loss_forward_backward_kl, unchanged (gradients: max error <= 8 x the fp32
oracle's own + floors, <= 5e-5 of the fp32 oracle for >= 99.5 % of the entries, 2e-3 for all; scalars: rtol 1e-5, floor
2e-7 - or, for the means over few rows here, 8 x the fp32 oracle's own error: _check_scalars).  Raw fp64 partials summed on the host, host under test against the stand-alone kernel: the two sum the same fp32
terms in another order, |diff| <= 2 rows 2^-53 sum|term| with sum|term| from the fp64 oracle's per-row terms.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from oracle import ppo_oracle as O
from oracle.seeded_inputs import loss_inputs
from test_mlp_chain_gpu import _net

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
V = 1
NAN = float('nan')
RTOL = 1e-5
E_CLIP, CRITIC_COEF, ENTROPY_COEF = 0.2, 2.0, 0.01
IN_DIM = 12
PAD = 64                    # rows allocated behind the minibatch in every per-row output: one whole tile of the largest kind
NAN_ROW = 23                # the row of `nan_row`: inside a tile of every size (row 7 of 16, 23 of 32 and of 64)
WIDTHS = (1, 2, 3, 4, 5, 21, 32, 33, 40)
OPTIONS = ('bound', 'smooth_reg', 'noclip_nobound', 'masked', 'ppo_false', 'no_write_back', 'all_masked', 'nan_row')
ONE_ROW = {'one_below': 0.7, 'one_inside': 1.05, 'one_above': 1.3}          # the ratio of a one-row case's (last) row

Host = namedtuple('Host', 'tile ragged full one')
HOSTS = {
    'standalone16': Host(16, 16 * 3 + 5, 16, 1),
    'standalone64': Host(64, 8192 + 64 + 5, 8192 + 64, 8192 + 64 + 1),
    'exact_g1_pipe': Host(16, 16 * 3 + 5, 16, 1),
    'exact_g1_unit': Host(16, 16 * 3 + 5, 16, 1),
    'exact_g1_unit_4w': Host(16, 16 * 384 + 16 + 5, 16 * 385, 16 * 385 + 1),
    'exact_g2': Host(32, 32 * 3 + 5, 32, 1),
    'exact_g4': Host(64, 64 * 3 + 5, 64, 1),
    'split_handoff': Host(64, 64 * 3 + 5, 64, 1),
    'split_nohandoff': Host(64, 64 * 3 + 5, 64, 1),
    'lean_bwd': Host(16, 16 * 3 + 5, 16, 1),
    'step_pipe': Host(16, 16 * 3 + 5, 16, 1),
    'step_lean': Host(16, 16 * 3 + 5, 16, 1),
}
REMAINDER_LOOP_HOSTS = ('standalone64', 'exact_g4', 'split_handoff', 'split_nohandoff')
STEP_HOSTS = ('step_pipe', 'step_lean')


def _cases():
    out = []
    for host in HOSTS:
        out += [(host, 'ragged', 21, opt) for opt in OPTIONS]
        out += [(host, 'ragged', A, 'bound') for A in WIDTHS if A != 21]
        out += [(host, kind, 21, 'bound') for kind in ('full',) + tuple(ONE_ROW)]
        if host in REMAINDER_LOOP_HOSTS:
            out += [(host, 'ragged', 65, 'bound'), (host, 'ragged', 65, 'masked'), (host, 'ragged', 66, 'bound')]
    return out


def _rows(host, kind):
    h = HOSTS[host]
    return {'ragged': h.ragged, 'full': h.full}.get(kind, h.one)


# ----------------------------------------------------------------------------- inputs and oracle (host side)

def _hp(opt):
    hp = {'e_clip': E_CLIP, 'critic_coef': CRITIC_COEF, 'entropy_coef': ENTROPY_COEF, 'bounds_loss_coef': 1e-4,
          'clip_value': True, 'use_smooth_clamp': False, 'bound_loss_type': 'bound'}
    if opt == 'smooth_reg':
        hp.update(use_smooth_clamp=True, bound_loss_type='regularisation', bounds_loss_coef=0.01)
    elif opt == 'noclip_nobound':
        hp.update(clip_value=False, bounds_loss_coef=None)
    elif opt == 'ppo_false':
        hp.update(ppo=False)
    return hp


def _inputs(rows, A, opt, kind, heads=None):
    """The seeded inputs of a case (oracle.seeded_inputs.loss_inputs; heads [rows, V + A] value first: a network's outputs
    to place them around) and its options.  nan_row: the inputs of `bound`; the NaN is planted by the caller."""
    mu, logstd, values, batch = loss_inputs(rows, A, seed=1000 * A + rows,
                                            mu=None if heads is None else heads[:, V:],
                                            values=None if heads is None else heads[:, :V])
    if kind in ONE_ROW:
        with torch.no_grad():
            nlp = O.neglogp(batch['actions'][-1:].double(), mu[-1:].double(), torch.exp(logstd.double()), logstd.double())
        batch['old_logp_actions'][-1] = float(nlp + math.log(ONE_ROW[kind]))
    mask = None
    if opt == 'masked':
        mask = (torch.rand(rows, generator=torch.Generator().manual_seed(7)) < 0.8).float()
        mask[-1], mask[-2] = 0.0, 1.0              # the ragged last tile (5 rows) holds both kinds
    elif opt == 'all_masked':
        mask = torch.zeros(rows)
    return SimpleNamespace(mu=mu, logstd=logstd, values=values, batch=batch, mask=mask, hp=_hp(opt),
                           write_back=opt != 'no_write_back', rows=rows, A=A, opt=opt, kind=kind)


def _with_nan(inp):
    inp.mu = inp.mu.clone()
    inp.mu[NAN_ROW, inp.A // 2] = NAN
    return inp


def _oracle(inp, mu=None, values=None):
    """(fp32 oracle, fp64 oracle) on the fp32 mu [rows, A] / values [rows, 1] given (default: the case's own)."""
    mu = inp.mu if mu is None else mu
    values = inp.values if values is None else values
    ref = O.distribution_loss_and_grads(mu, inp.logstd, values, inp.batch, inp.hp, inp.mask)
    to64 = lambda t: t.double() if torch.is_floating_point(t) else t
    truth = O.distribution_loss_and_grads(to64(mu), to64(inp.logstd), to64(values), {k: to64(v) for k, v in inp.batch.items()},
                                          inp.hp, None if inp.mask is None else inp.mask.double())
    return ref, truth


@functools.lru_cache(maxsize=None)
def _shared(rows, A, opt, kind):
    """Inputs and both oracles of a case whose mu / values are inputs (every host but the one-launch steps): computed
    once, shared by the hosts that run the same row count, never modified."""
    inp = _inputs(rows, A, opt, kind)
    if opt == 'nan_row':
        _with_nan(inp)
    return (inp,) + _oracle(inp)


def _check_inputs(inp, truth, tile):
    """On the fp64 oracle's quantities: a case of the clipped surrogate has rows below, inside and above [1 - e, 1 + e] (a
    one-row case: its row in the region it names), a `bound` case rows with an active bound loss, a masked case masked and
    unmasked rows in its last, ragged tile."""
    rows = inp.rows
    finite = torch.isfinite(truth['neglogp'].reshape(rows))
    if inp.hp.get('ppo', True) and not inp.hp['use_smooth_clamp']:
        ratio = torch.exp(inp.batch['old_logp_actions'].double() - truth['neglogp'].reshape(rows))
        below, above = ratio < 1.0 - E_CLIP, ratio > 1.0 + E_CLIP
        inside = finite & ~below & ~above
        if inp.kind in ONE_ROW:
            want = {'one_below': below, 'one_inside': inside, 'one_above': above}[inp.kind]
            assert want[-1], (inp.kind, ratio[-1].item())
        if rows >= 16:
            assert below.any() and inside.any() and above.any(), (rows, inp.A, below.sum(), inside.sum(), above.sum())
    if inp.hp['bounds_loss_coef'] is not None and rows >= 16:
        assert (truth['rows']['b'][finite] > 0).any()
    if inp.opt == 'masked':
        last = inp.mask[(rows - 1) // tile * tile:]
        assert 1 < last.numel() < tile and (last == 0).any() and (last == 1).any()


# ----------------------------------------------------------------------------- launches

def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    """Bit-equal, any NaN equal to any NaN (which operand's payload a product keeps is the compiler's choice)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(_bits(torch.where(torch.isnan(a), 0.0, a)), _bits(torch.where(torch.isnan(b), 0.0, b)))


def _padded(t, rows):
    """[rows + PAD, ...] on the device: t, then NaN rows."""
    out = torch.full((rows + PAD,) + tuple(t.shape[1:]), NAN, device=DEV)
    out[:rows] = t.to(DEV)
    return out


def _device_batch(inp):
    d = lambda t: t.contiguous().to(DEV)
    b = inp.batch
    dev = SimpleNamespace(logstd=d(inp.logstd), actions=d(b['actions']), old_neglogp=d(b['old_logp_actions']),
                          adv=d(b['advantages']), old_values=d(b['old_values'].reshape(-1)), returns=d(b['returns'].reshape(-1)),
                          mask=None if inp.mask is None else d(inp.mask))
    dev.mask_sum = None if dev.mask is None else dev.mask.sum().reshape(1)
    return dev


def _loss_call(inp, dev, mu, values, old_mu, old_sigma, d_mu, d_values, partials, lo=0, hi=None, mask=None, mask_sum=None):
    """(args, kwargs) of ops.ppo_loss_fused / ops.ppo_loss_desc for rows lo .. hi of the case."""
    from rl_games_amd import ops
    hp = inp.hp
    s = slice(lo, hi)
    coef_b = hp['bounds_loss_coef'] if hp['bounds_loss_coef'] is not None else 0.0
    kind = 0 if hp['bounds_loss_coef'] is None else ops.BOUND_KINDS[hp['bound_loss_type']]
    smooth = ops.SURROGATE_NONE if not hp.get('ppo', True) else hp['use_smooth_clamp']
    if mask is None and dev.mask is not None:
        mask, mask_sum = dev.mask[s], dev.mask_sum
    args = (mu[s], dev.logstd, values[s], dev.actions[s], dev.old_neglogp[s], dev.adv[s], dev.old_values[s], dev.returns[s],
            old_mu[s], old_sigma[s], d_mu[s], d_values[s], partials, hp['e_clip'], hp['critic_coef'], coef_b)
    return args, dict(clip_value=hp['clip_value'], smooth=smooth, bound_kind=kind, write_back=inp.write_back, mask=mask,
                      mask_sum=mask_sum)


def _outputs(inp, layout='value_first'):
    """NaN-filled outputs with PAD rows behind the minibatch: d heads (and the views d mu / d value of the layout),
    old mu / old sigma (the case's, to be overwritten)."""
    rows, A = inp.rows, inp.A
    d_heads = torch.full((rows + PAD, V + A), NAN, device=DEV)
    d_mu, d_val = (d_heads[:, V:], d_heads[:, 0]) if layout == 'value_first' else (d_heads[:, :A], d_heads[:, A])
    return SimpleNamespace(d_heads=d_heads, d_mu=d_mu, d_values=d_val, old_mu=_padded(inp.batch['mu'], rows),
                           old_sigma=_padded(inp.batch['sigma'], rows))


def _partials(nb, A):
    from rl_games_amd import ops
    return torch.full((nb + 2, ops.ppo_loss_partials_per_block(A)), NAN, dtype=torch.float64, device=DEV)


def _standalone(inp, dev, mu, values, chunked):
    """The stand-alone kernel on device views mu [rows, A] / values [rows].  chunked: launches of at most 8,192 rows (the
    16-row tile) with the whole minibatch's denominator as the mask sum - an all-ones mask where the case has none."""
    from rl_games_amd import ops
    rows, A = inp.rows, inp.A
    out = _outputs(inp)
    if not chunked:
        out.nb = ops.ppo_loss_blocks(rows)
        out.partials = _partials(out.nb, A)
        args, kw = _loss_call(inp, dev, mu, values, out.old_mu[:rows], out.old_sigma[:rows], out.d_mu[:rows], out.d_values[:rows],
                              out.partials)
        ops.ppo_loss_fused(*args, **kw)
        return out
    mask = dev.mask if dev.mask is not None else torch.ones(rows, device=DEV)
    mask_sum = dev.mask_sum if dev.mask is not None else torch.full((1,), float(rows), device=DEV)
    bounds = list(range(0, rows, 8192)) + [rows]
    out.nb = sum(ops.ppo_loss_blocks(hi - lo) for lo, hi in zip(bounds, bounds[1:]))
    out.partials = _partials(out.nb, A)
    at = 0
    for lo, hi in zip(bounds, bounds[1:]):
        assert ops.ppo_loss_blocks(hi - lo) == -(-(hi - lo) // 16)
        args, kw = _loss_call(inp, dev, mu[:rows], values[:rows], out.old_mu[:rows], out.old_sigma[:rows], out.d_mu[:rows],
                              out.d_values[:rows], out.partials[at:], lo, hi, mask[lo:hi], mask_sum)
        ops.ppo_loss_fused(*args, **kw)
        at += ops.ppo_loss_blocks(hi - lo)
    return out


def _run_standalone(host, inp):
    from rl_games_amd import ops
    rows = inp.rows
    assert ops.ppo_loss_blocks(rows) == -(-rows // HOSTS[host].tile)       # the 16- / 64-row tile of this minibatch
    dev = _device_batch(inp)
    mu, values = inp.mu.to(DEV), inp.values.reshape(-1).to(DEV)
    out = _standalone(inp, dev, mu, values, chunked=False)
    out.dzs = []
    # the 16-row kernel has no other launch of itself to compare with: its rows are every other host's reference
    out.alone = _standalone(inp, dev, mu, values, chunked=True) if host == 'standalone64' else out
    out.mu, out.values = inp.mu, inp.values
    return out


def _chain(host, A):
    from rl_games_amd import ops
    hidden = [64, 30] if 'unit' in host else [64, 32]
    layers, g = _net(IN_DIM, hidden, V + A, 'elu', seed=7 + A)
    chain = ops.MlpChain(layers, DEV)
    if host == 'step_pipe':
        chain._lean = False
    return chain, hidden, g


def _run_backward(host, inp):
    """A backward launch with the loss descriptor: the heads are the case's mu / values (the launch reads them through the
    descriptor only), H of the hidden layers comes from a forward of the same network.
    The kernel is asserted through MlpChain's own predicates (_route, groups, split_products, lean_used; behind the launch
    the gradient maxima only the split / lean kernels leave) as far as they go.  No predicate tells the pipelined G = 1
    kernel from the unit-structured one (chain_rows16_status decides: a hidden width of 30 fails it), 8 waves from 4
    (kChainWideBlocks = 384 workgroups decides: asserted on num_blocks), or the split kernel's LDS hand-off of d heads
    from its re-read (the layout of d heads decides): those hosts are selected by the shape rule in the code."""
    from rl_games_amd import ops
    rows, A = inp.rows, inp.A
    chain, hidden, g = _chain(host, A)
    exact = host.startswith('exact')
    groups = {'exact_g2': 2, 'exact_g4': 4, 'split_handoff': 4, 'split_nohandoff': 4}.get(host, 0)
    split = None if not exact else False
    G = HOSTS[host].tile // 16
    # ---- the host that will run
    assert chain.groups(rows, 1, groups) == G
    route = chain._route(rows, 1, groups, split)
    assert route == ('exact' if exact else 'split' if host.startswith('split') else 'lean')
    if host.startswith('split'):
        assert chain.split_products(rows, 1, groups) and not chain.lean_used(rows, 1, groups)
    if host == 'lean_bwd':
        assert chain.lean_used(rows, 1) and not chain.split_products(rows, 1)
    if host == 'exact_g1_unit_4w':
        assert chain.num_blocks(rows, 1, groups) > 384
    elif G == 1:
        assert chain.num_blocks(rows, 1, groups) <= 384
    x = torch.randn(rows, IN_DIM, generator=g).to(DEV)
    acts = [torch.empty(rows, u, device=DEV) for u in hidden]
    chain.forward(x, torch.empty(rows, V + A, device=DEV), act_out=acts, split_products=split)
    layout = 'value_last' if host == 'split_nohandoff' else 'value_first'
    cat = [inp.values, inp.mu] if layout == 'value_first' else [inp.mu, inp.values]
    heads = torch.cat(cat, dim=1).to(DEV)
    mu, values = (heads[:, V:], heads[:, 0]) if layout == 'value_first' else (heads[:, :A], heads[:, A])
    dev = _device_batch(inp)
    out = _outputs(inp, layout)
    out.nb = chain.num_blocks(rows, 1, groups)
    assert out.nb == -(-rows // HOSTS[host].tile)
    out.partials = _partials(out.nb, A)
    out.dzs = [torch.full((rows + PAD, u), NAN, device=DEV) for u in hidden]
    parts = [torch.empty(out.nb * u, dtype=torch.float64, device=DEV) for u in hidden]
    args, kw = _loss_call(inp, dev, mu, values, out.old_mu[:rows], out.old_sigma[:rows], out.d_mu[:rows], out.d_values[:rows],
                          out.partials)
    chain.backward(out.d_heads[:rows], acts, [t[:rows] for t in out.dzs], parts, groups=groups, ppo_loss=ops.ppo_loss_desc(*args, **kw),
                   split_products=split)
    torch.cuda.synchronize()
    # ---- the host that ran: only the split / lean kernels leave gradient maxima (64 / 16 rows per entry)
    if host.startswith('split'):
        assert chain.gradient_maxima(rows) is not None and chain.maxima_rows_per_entry == 64
    elif host == 'lean_bwd':
        assert chain.gradient_maxima(rows) is not None and chain.maxima_rows_per_entry == 16
    else:
        assert chain.gradient_maxima(rows) is None
    out.alone = _standalone(inp, dev, mu, values, chunked=False)
    out.mu, out.values = inp.mu, inp.values
    return out


def _run_step(host, rows, A, opt, kind):
    """A one-launch step: mu / values are the network's own outputs.  The case's inputs are placed around the heads of a
    forward of the same observations; the reference is evaluated on the heads the step itself wrote.  nan_row: the NaN is
    planted in the row's observations (its value is then NaN as well).  Returns None when the step declined."""
    from rl_games_amd import ops
    chain, hidden, g = _chain(host, A)
    lean = host == 'step_lean'
    for kind_of_launch in (2, 1):
        assert chain.lean_used(rows, kind_of_launch) == lean and not chain.split_products(rows, kind_of_launch)
        assert chain._route(rows, kind_of_launch) == ('lean' if lean else 'exact')
    # (observations of twice the unit scale: mu of a standard deviation of 1.1 - 1.3, like loss_inputs' 1.2, a third of
    #  it beyond the soft bound of 1.1)
    x = (2 * torch.randn(rows, IN_DIM, generator=g)).to(DEV)
    heads0 = torch.empty(rows, V + A, device=DEV)
    chain.forward(x, heads0, act_out=[torch.empty(rows, u, device=DEV) for u in hidden])
    inp = _inputs(rows, A, opt, kind, heads=heads0.cpu())
    if opt == 'nan_row':
        x[NAN_ROW, 0] = NAN
    dev = _device_batch(inp)
    out = _outputs(inp)
    out.inp = inp
    heads = torch.full((rows, V + A), NAN, device=DEV)
    acts = [torch.full((rows, u), NAN, device=DEV) for u in hidden]
    out.nb = chain.num_blocks(rows, 1)
    out.partials = _partials(out.nb, A)
    out.dzs = [torch.full((rows + PAD, u), NAN, device=DEV) for u in hidden]
    parts = [torch.empty(out.nb * u, dtype=torch.float64, device=DEV) for u in hidden]
    args, kw = _loss_call(inp, dev, heads[:, V:], heads[:, 0], out.old_mu[:rows], out.old_sigma[:rows], out.d_mu[:rows],
                          out.d_values[:rows], out.partials)
    ran = chain.step(x, heads, acts, out.d_heads[:rows], [t[:rows] for t in out.dzs], parts, ops.ppo_loss_desc(*args, **kw))
    torch.cuda.synchronize()
    if not ran:
        written = [heads, out.d_heads, out.partials] + acts + out.dzs
        assert all(torch.isnan(t).all() for t in written)
        assert _same_bits(out.old_mu[:rows], inp.batch['mu']) and _same_bits(out.old_sigma[:rows], inp.batch['sigma'])
        return None
    out.alone = _standalone(inp, dev, heads[:, V:], heads[:, 0], chunked=False)
    h = heads.cpu()
    out.mu, out.values = h[:, V:].contiguous(), h[:, :V].contiguous()
    return out


def _run(host, rows, A, opt, kind):
    """-> (inputs, fp32 oracle, fp64 oracle, outputs) of a case; outputs None: a one-launch step that declined."""
    if host in STEP_HOSTS:
        out = _run_step(host, rows, A, opt, kind)
        if out is None:
            return None, None, None, None
        return (out.inp,) + _oracle(out.inp, out.mu, out.values) + (out,)
    inp, ref, truth = _shared(rows, A, opt, kind)
    out = _run_standalone(host, inp) if host.startswith('standalone') else _run_backward(host, inp)
    return inp, ref, truth, out


# ----------------------------------------------------------------------------- checks

def _finalize(inp, out):
    from rl_games_amd import ops
    hp, A = inp.hp, inp.A
    coef_b = hp['bounds_loss_coef'] if hp['bounds_loss_coef'] is not None else 0.0
    fin = SimpleNamespace(scalars=torch.zeros(8, device=DEV), d_logstd=torch.zeros(A, device=DEV), kl=torch.zeros(1, device=DEV),
                          d_mu_bias=torch.zeros(A, device=DEV), d_value_bias=torch.zeros(1, device=DEV))
    ops.ppo_loss_finalize(out.partials[:out.nb], out.nb, A, inp.rows, inp.mask is not None, hp['critic_coef'], hp['entropy_coef'],
                          coef_b, fin.scalars, fin.d_logstd, fin.kl, fin.d_mu_bias, fin.d_value_bias)
    return fin


def _term_sums(inp, truth, mu, values):
    """sum |term| of the kLossScalars + 2 A sums a tile's partial row holds, from the fp64 oracle."""
    rows, A = inp.rows, inp.A
    m = torch.ones(rows, dtype=torch.float64) if inp.mask is None else inp.mask.double()
    r = truth['rows']
    z = (inp.batch['actions'].double() - mu.double()) / torch.exp(inp.logstd.double())
    d_ls = truth['d_neglogp'].reshape(rows, 1) * (1.0 - z * z)
    scal = [(r[k] * m).abs().sum() for k in ('a', 'c', 'entropy', 'b', 'kl')] + [m.sum(), truth['d_values'].abs().sum()]
    return torch.cat([torch.stack(scal), d_ls.abs().sum(0), truth['d_mu'].abs().sum(0)])


def _check_padding(inp, out):
    rows = inp.rows
    bad = []
    for name in ('d_heads', 'old_mu', 'old_sigma'):
        if not torch.isnan(getattr(out, name)[rows:]).all():
            bad.append(f'{name}: rows behind the minibatch written')
    for k, t in enumerate(out.dzs):
        if not torch.isnan(t[rows:]).all():
            bad.append(f'dZ {k}: rows behind the minibatch written')
    if not torch.isnan(out.partials[out.nb:]).all():
        bad.append('partials: rows behind the last tile written')
    return bad


def _check_rows_equal_standalone(inp, out):
    rows = inp.rows
    bad = []
    for name in ('d_mu', 'd_values', 'old_mu', 'old_sigma'):
        if not _same_bits(getattr(out, name)[:rows], getattr(out.alone, name)[:rows]):
            bad.append(f'{name}: bits differ from the stand-alone kernel')
    return bad


def _check_write_back(inp, ref, out):
    rows = inp.rows
    if not inp.write_back:
        same = _same_bits(out.old_mu[:rows], inp.batch['mu']) and _same_bits(out.old_sigma[:rows], inp.batch['sigma'])
        return [] if same else ['write_back off: old mu / old sigma changed']
    bad = []
    if not _same_bits(out.old_mu[:rows], out.mu):
        bad.append('old mu is not a copy of mu')
    # sigma = exp(logstd): device expf and the host's exp may differ in the last bit
    if not torch.allclose(out.old_sigma[:rows].cpu(), ref['sigma'], rtol=3e-7, atol=0):
        bad.append('old sigma')
    return bad


def _check_gradients(inp, ref, truth, out, fin, figures):
    """test_ppo_loss_forward_backward_kl's criterion: as close to the fp64 truth as the fp32 oracle is (max error within 8x
    of the oracle's own, + its floors), element-wise within 5e-5 of the fp32 oracle for >= 99.5 % of the entries, 2e-3 for
    all."""
    rows = inp.rows
    bad = []
    scale = 1.0 / rows
    for got, key in ((out.d_mu[:rows].cpu(), 'd_mu'), (out.d_values[:rows].cpu().reshape(-1, 1), 'd_values'),
                     (fin.d_logstd.cpu(), 'd_logstd')):
        r32, r64 = ref[key], truth[key]
        atol = 1e-6 * r32.abs().max().item()
        outliers = ((got - r32).abs() > 5e-5 * r32.abs() + atol).float().mean().item()
        err_kernel = (got.double() - r64).abs().max().item()
        err_oracle = (r32.double() - r64).abs().max().item()
        bound = 8 * err_oracle + 1e-9 * scale + 1e-6 * r64.abs().max().item()
        figures.append(f'{key}: outliers {outliers:.4f} err {err_kernel:.3e} oracle {err_oracle:.3e} bound {bound:.3e}')
        if not torch.allclose(got, r32, rtol=2e-3, atol=atol):
            bad.append(f'{key}: not within 2e-3 of the fp32 oracle')
        if key != 'd_logstd' and outliers > 5e-3:
            bad.append(f'{key}: {outliers:.4f} of the entries beyond 5e-5')
        if not err_kernel <= bound:
            bad.append(f'{key}: error {err_kernel:.3e} > {bound:.3e}')
    return bad


SCALARS = ('a_loss', 'c_loss', 'entropy', 'b_loss', 'kl', 'loss')


def _check_scalars(ref, truth, fin, figures):
    """test_ppo_loss_forward_backward_kl's criterion: rtol 1e-5, floor 2e-7 against the fp64 truth; non-finite where the
    oracle is.  That floor was set for minibatches of 257 rows and more.  A mean over the 53 rows of a 16-row host's ragged
    case averages fewer rounding errors, and at A = 40 every term carries more of them (neglogp ~ 90, half an ulp of it
    4e-6 in the exponent of the ratio): there a_loss = -0.01190 is a sum of terms of both signs and of magnitude 1, the
    fp32 oracle itself is 2.5e-7 from the fp64 value (measured on the CPU on these inputs: rows 53, A 40, `bound`) and the
    kernel 4.4e-7, against rtol |a_loss| + floor = 3.2e-7.  Hence the same margin as for the gradients: a scalar may also
    be within 8 x the fp32 oracle's own error of the truth."""
    s = fin.scalars.cpu()
    bad = []
    for k, name in enumerate(SCALARS):
        t64, got = truth[name].item(), s[k].item()
        if not math.isfinite(t64):
            if math.isfinite(got):
                bad.append(f'{name}: {got} where the oracle has {t64}')
            continue
        own_err = abs(ref[name].item() - t64)
        figures.append(f'{name}: {got:.9g} truth {t64:.9g} err {abs(got - t64):.2e} oracle {own_err:.2e}')
        if not abs(got - t64) <= max(RTOL * abs(t64) + 2e-7, 8 * own_err):
            bad.append(f'{name}: {got} against {t64}')
        if not abs(got - ref[name].item()) <= RTOL * abs(t64) + 2e-7 + 2 * own_err:
            bad.append(f'{name}: {got} against the fp32 oracle {ref[name].item()}')
    if _bits(fin.kl)[0] != _bits(fin.scalars)[4]:
        bad.append('kl slot')
    return bad


def _check_partial_sums(inp, truth, out, figures):
    """The raw fp64 partial rows summed on the host: host under test against the stand-alone kernel, the same fp32 terms in
    another order.  Either sum is within (rows - 1) 2^-53 sum|term| of the exact one."""
    mine = out.partials[:out.nb].cpu().sum(0)
    alone = out.alone.partials[:out.alone.nb].cpu().sum(0)
    bound = 2.0 * inp.rows * 2.0 ** -53 * _term_sums(inp, truth, out.mu, out.values)
    diff = (mine - alone).abs()
    both_nan = torch.isnan(mine) & torch.isnan(alone)
    ok = (diff <= bound) | both_nan
    finite = torch.isfinite(diff) & torch.isfinite(bound) & (bound > 0)
    worst = (diff[finite] / bound[finite]).max().item() if finite.any() else 0.0
    figures.append(f'partial sums: worst |diff| / bound {worst:.3f}')
    return [] if ok.all() else [f'partial sums: columns {torch.nonzero(~ok).reshape(-1).tolist()} differ beyond fp64 reassociation']


@pytest.mark.parametrize('host,kind,A,opt', _cases(), ids=lambda v: str(v))
def test_loss_tile(host, kind, A, opt):
    """One case of the matrix in the module's docstring, under test_ops_gpu.py::test_ppo_loss_forward_backward_kl's bounds.
    One addition, for means over few rows: a scalar may be within 8 x the fp32 oracle's own error of the fp64 value where
    that is more than rtol 1e-5 + 2e-7.  Measured (fp32 oracle against fp64 on the CPU, kernel on the GPU) on the only
    inputs that need it, 53 rows, A = 40, `bound`: a_loss = -0.0118955, fp32 oracle off by 2.5e-7, kernel by 4.4e-7,
    rtol + floor 3.2e-7, 8 x oracle 2.0e-6 (_check_scalars)."""
    rows = _rows(host, kind)
    inp, ref, truth, out = _run(host, rows, A, opt, kind)
    if host in STEP_HOSTS and A > 32:
        assert out is None                      # declined, nothing written (_run_step)
        return
    assert out is not None
    figures = []
    bad = _check_padding(inp, out) + _check_rows_equal_standalone(inp, out)
    fin = _finalize(inp, out)
    if opt != 'nan_row':
        _check_inputs(inp, truth, HOSTS[host].tile)
        bad += _check_write_back(inp, ref, out)
        bad += _check_gradients(inp, ref, truth, out, fin, figures)
        bad += _check_scalars(ref, truth, fin, figures)
        bad += _check_partial_sums(inp, truth, out, figures)
        for t in (out.d_heads[:rows], out.old_mu[:rows], out.old_sigma[:rows], fin.scalars, fin.d_logstd, fin.d_mu_bias,
                  fin.d_value_bias, out.partials[:out.nb]) + tuple(t[:rows] for t in out.dzs):
            if not torch.isfinite(t).all():
                bad.append('non-finite output')
        if opt == 'all_masked':
            zero = (out.d_heads[:rows], fin.scalars, fin.d_logstd, fin.d_mu_bias, fin.d_value_bias, out.partials[:out.nb])
            if not all((t == 0).all() for t in zero):
                bad.append('all rows masked: a gradient or a scalar is not exactly 0')
    else:
        _, _, _, clean = _run(host, rows, A, 'bound', kind)
        others = torch.arange(rows) != NAN_ROW
        # the row: non-finite wherever the oracle's is; every other row: the bits of the run without the NaN
        for name, key in (('d_mu', 'd_mu'), ('d_values', 'd_values')):
            got, want = getattr(out, name)[:rows].cpu().reshape(rows, -1), ref[key].reshape(rows, -1)
            if (torch.isfinite(got) & ~torch.isfinite(want)).any():
                bad.append(f'{name}: finite where the oracle is not')
            if not _same_bits(got[others], getattr(clean, name)[:rows].cpu().reshape(rows, -1)[others]):
                bad.append(f'{name}: the NaN changed another row')
        if torch.isfinite(out.d_mu[NAN_ROW]).any():
            bad.append('d_mu: finite entries in the NaN row')
        bad += _check_scalars(ref, truth, fin, figures)
        if (torch.isfinite(fin.d_logstd.cpu()) & ~torch.isfinite(ref['d_logstd'])).any():
            bad.append('d_logstd: finite where the oracle is not')
        bad += _check_partial_sums(inp, truth, out, figures)
        for k, (t, c) in enumerate(zip(out.dzs, clean.dzs)):              # chain hosts: the NaN reaches only its row of dZ
            if not _same_bits(t[:rows][others.to(DEV)], c[:rows][others.to(DEV)]) or not torch.isfinite(t[:rows][others.to(DEV)]).all():
                bad.append(f'dZ {k}: the NaN left its row')
            if torch.isfinite(t[NAN_ROW]).all():
                bad.append(f'dZ {k}: the NaN row is finite')
    print(f'{host} {kind} A={A} {opt} rows={rows}: ' + '; '.join(figures))
    assert not bad, bad
