"""GPU: the range guard of the split-fp16 products - rlg_range_scan, the guarded optimiser launches, exact products per
chain (ops.MlpChain(products='exact')) and per weight-gradient launch, and the agents' `split_range` / `chain_products`.

No test here provokes a device fault: a NaN or an Inf in an array is data.
"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from test_mlp_chain_gpu import _bit_equal, _close, _net

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from rl_games_amd import ops
    return ops


# ----------------------------------------------------------------------------- rlg_range_scan

def _expected(arrays):
    """(tag of the first array in order with a non-finite value, smallest such flat index) by torch; (0, 0): clean."""
    for t, tag in arrays:
        bad = ~torch.isfinite(t.reshape(-1))
        if bad.any():
            return tag, int(torch.nonzero(bad)[0].item())
    return 0, 0


def _view(n, aligned, gen):
    """n finite floats at a 16-byte aligned address, or one float behind one."""
    base = torch.randn(n + 1, generator=gen).to(DEV)
    assert base.data_ptr() % 16 == 0
    return base[:n] if aligned else base[1:]


@pytest.mark.parametrize('n', [1, 3, 63, 64, 65, 4097])
def test_scan_finds_every_non_finite_value_at_the_first_last_and_a_middle_index(n):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    for aligned in (True, False):
        t = _view(n, aligned, gen)
        assert (t.data_ptr() % 16 == 0) == aligned
        rec = ops.guard_record(DEV)
        ops.range_scan([(t, 7)], rec)
        assert rec.tolist() == [0, 0, 0, 0]                          # clean input leaves a cleared record cleared
        for pos in sorted({0, n // 2, n - 1}):
            for bad in (float('nan'), float('inf'), float('-inf')):
                keep = t[pos].clone()
                t[pos] = bad
                rec = ops.guard_record(DEV)
                ops.range_scan([(t, 7)], rec)
                assert ops.read_guard(rec) == _expected([(t, 7)]) == (7, pos), (n, aligned, pos, bad)
                t[pos] = keep


def test_scan_reports_the_first_array_in_argument_order_and_its_smallest_index():
    """Several arrays, several hits each, many workgroups (300,001 elements: 74 of them), every alignment: the record
    does not depend on which workgroup finds what first - the same record from 5 launches."""
    ops = _ops()
    gen = torch.Generator().manual_seed(1)
    a, b, c, d = (_view(n, al, gen) for n, al in ((4097, True), (300001, False), (65, False), (100000, True)))
    arrays = [(a, 5), (b, 9), (c, 2), (d, 11)]
    c[3] = float('nan')
    d[:] = float('inf')                                             # every lane of every workgroup has a hit
    for idx in (299999, 150002, 77777, 300000):
        b[idx] = float('-inf')
    want = _expected(arrays)
    assert want == (9, 77777)
    for _ in range(5):
        rec = ops.guard_record(DEV)
        ops.range_scan(arrays, rec)
        assert ops.read_guard(rec) == want
    # the earlier array wins whatever its index; an array of zero elements is skipped
    a[4096] = float('nan')
    rec = ops.guard_record(DEV)
    ops.range_scan([(a[:0], 3)] + arrays, rec)
    assert ops.read_guard(rec) == (5, 4096)
    # all of an array non-finite: index 0
    rec = ops.guard_record(DEV)
    ops.range_scan([(d, 11), (b, 9)], rec)
    assert ops.read_guard(rec) == (11, 0)
    # eight arrays are one launch, a ninth is refused
    eight = [(_view(5, True, gen), k + 1) for k in range(8)]
    eight[7][0][4] = float('nan')
    rec = ops.guard_record(DEV)
    ops.range_scan(eight, rec)
    assert ops.read_guard(rec) == (8, 4)
    with pytest.raises(ValueError):
        ops.range_scan(eight + [(a, 9)], rec)


def test_a_set_record_is_sticky_bit_for_bit():
    ops = _ops()
    gen = torch.Generator().manual_seed(2)
    t, u = _view(4097, True, gen), _view(65, False, gen)
    clean = _view(300, True, gen)
    t[1000] = float('nan')
    rec = ops.guard_record(DEV)
    ops.range_scan([(t, 4)], rec)
    assert ops.read_guard(rec) == (4, 1000)
    first = rec.clone()
    ops.range_scan([(clean, 1)], rec)                                # a later clean launch
    assert torch.equal(rec, first)
    u[0] = float('inf')
    t[5] = float('nan')
    ops.range_scan([(u, 1), (t, 4)], rec)                            # later launches with other - "better" - hits
    ops.range_scan([(t, 4)], rec)
    assert torch.equal(rec, first)
    # a record that an optimiser launch set (two words, the scan's own words clear) is kept as well
    rec = torch.tensor([ops.GUARD_TAG_ADAM, 12, 0, 0], dtype=torch.int32, device=DEV)
    ops.range_scan([(u, 1), (t, 4)], rec)
    assert rec.tolist() == [ops.GUARD_TAG_ADAM, 12, 0, 0]
    # cleared, the record takes the next hit
    rec.zero_()
    ops.range_scan([(u, 1), (t, 4)], rec)
    assert ops.read_guard(rec) == (1, 0)


def test_scan_is_capturable():
    ops = _ops()
    gen = torch.Generator().manual_seed(3)
    t = _view(4097, False, gen)
    rec = ops.guard_record(DEV)
    ops.range_scan([(t, 3)], rec)                                    # (eager once: nothing is allocated under capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.range_scan([(t, 3)], rec)
    g.replay()
    assert rec.tolist() == [0, 0, 0, 0]
    t[77] = float('nan')
    g.replay()
    assert ops.read_guard(rec) == (3, 77)


# ----------------------------------------------------------------------------- guarded Adam, both kernels

LR = 3e-4
STEP = 3


class _Adam:
    """One optimiser state for adam_step_kernel ('step': a three-tensor arena of 64 x 12 + 33 + 6 = 807 parameters - no
    multiple of 4, three tail elements) or adam_pack_kernel ('pack': a [12 -> 64 -> 32] chain whose planes the launch
    writes), at step count STEP."""

    def __init__(self, kind):
        ops = _ops()
        self.kind = kind
        g = torch.Generator().manual_seed(17)
        if kind == 'pack':
            layers, g = _net(12, [64], 32, 'elu', seed=17)
            n = sum(w.numel() + b.numel() for w, b, _ in layers)
            self.p = torch.empty(0, device=DEV, dtype=torch.float32).set_(layers[0][0].untyped_storage(), 0, (n,))
            assert self.p.data_ptr() == layers[0][0].data_ptr()
            self.chain = ops.MlpChain(layers, DEV, weights_version=lambda: 0)
            self.target = self.chain.adam_pack_target()             # (packs the whole buffer once)
        else:
            n = 64 * 12 + 33 + 6
            self.p = (0.1 * torch.randn(n, generator=g)).to(DEV)
            self.tensors = [self.p[:768].view(64, 12), self.p[768:801], self.p[801:]]
            self.chain = self.target = None
        self.n = n
        self.m = (0.01 * torch.randn(n, generator=g)).to(DEV)
        self.v = (0.001 * torch.rand(n, generator=g)).to(DEV)
        self.grads = (0.1 * torch.randn(n, generator=g)).to(DEV)
        self.lr_slots = torch.tensor([7.0, 7.0], dtype=torch.float64, device=DEV)
        self.lr_slots[(STEP - 1) & 1] = LR
        self.counter = torch.tensor([STEP], dtype=torch.int64, device=DEV)
        self.stats = torch.full((4,), -1.0, device=DEV)
        self.kl = torch.tensor([0.001], device=DEV)

    KEYS = ('p', 'g', 'm', 'v', 'lr_slots', 'stats', 'planes')

    def snapshot(self, g):
        torch.cuda.synchronize()
        planes = self.chain._plane_buffer().clone() if self.chain is not None else torch.zeros(1, device=DEV)
        return dict(p=self.p.clone(), g=g.clone(), m=self.m.clone(), v=self.v.clone(), lr_slots=self.lr_slots.clone(),
                    stats=self.stats.clone(), planes=planes)

    def restore(self, snap):
        self.p.copy_(snap['p'])
        self.m.copy_(snap['m'])
        self.v.copy_(snap['v'])
        self.lr_slots.copy_(snap['lr_slots'])
        self.stats.copy_(snap['stats'])
        if self.chain is not None:
            self.chain._plane_buffer().copy_(snap['planes'])

    def step(self, grads, guard=None, skip=None):
        """One launch on a copy of `grads`; returns the state behind it."""
        ops = _ops()
        g = grads.clone()
        norm = torch.zeros(ops.grad_norm_blocks(self.n), dtype=torch.float64, device=DEV)
        ops.grad_sumsq(g, 1.0, norm, None)
        kw = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule_kind=1, kl=self.kl, kl_scale=1.0,
                  kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5, stats_out=self.stats,
                  skip_flag=None if skip is None else skip.data_ptr(), pack=self.target)
        args = (self.p, g, self.m, self.v, norm, 1.0, 0.5, self.lr_slots, self.counter)
        if guard is None:
            ops.adam_step(*args, **kw)
        else:
            ops.adam_step_guarded(guard, *args, **kw)
        return self.snapshot(g)


def _same(a, b, keys=_Adam.KEYS):
    return [k for k in keys if not _bit_equal(a[k], b[k])]


@pytest.mark.parametrize('kind', ['step', 'pack'])
def test_guarded_adam_equals_the_unguarded_launch_on_finite_gradients_and_skips_like_skip_flag_otherwise(kind):
    """Every buffer that test_skip_flag_leaves_everything_but_the_statistics_and_carries_the_learning_rate names -
    parameters, clipped gradients, both moments, the learning-rate slots, the statistics row - plus the planes of the
    pack form.  An infinite gradient trips the guard as well: the unguarded launch clips with coefficient 0 there and
    spoils only the infinite elements; a guarded run asked for nothing computed from an overflow to be applied, and drops
    the step - that difference is deliberate."""
    ops = _ops()
    a = _Adam(kind)
    start = a.snapshot(a.grads)
    rec = ops.guard_record(DEV)

    # finite gradients: the same bits as the unguarded entry, the record stays clear
    plain = a.step(a.grads)
    a.restore(start)
    guarded = a.step(a.grads, guard=rec)
    assert not _same(plain, guarded) and rec.tolist() == [0, 0, 0, 0]
    assert not torch.equal(plain['p'], start['p']) and plain['lr_slots'].tolist() != [LR, LR]

    # one NaN gradient: skipped exactly as a set skip flag skips - and recorded
    bad = a.grads.clone()
    bad[5] = float('nan')
    a.restore(start)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    flagged = a.step(bad, skip=flag)
    a.restore(start)
    tripped = a.step(bad, guard=rec)
    assert not _same(flagged, tripped)
    assert not _same(tripped, dict(start, g=bad), ('p', 'g', 'm', 'v', 'planes'))
    assert tripped['lr_slots'].tolist() == [LR, LR]                  # carried over (step 3 reads slot 0, writes slot 1)
    st = tripped['stats'].cpu().numpy()
    assert np.isnan(st[0]) and st[2] == np.float32(LR) and st[3] == np.float32(LR)
    assert rec.tolist() == [ops.GUARD_TAG_ADAM, STEP, 0, 0]
    assert ops.read_guard(rec) == (ops.GUARD_TAG_ADAM, STEP)

    # the record is set: a following launch with finite gradients is still skipped, the record stays
    after = a.step(a.grads, guard=rec)
    assert not _same(after, dict(tripped, g=a.grads), ('p', 'g', 'm', 'v', 'lr_slots', 'planes'))
    assert rec.tolist() == [ops.GUARD_TAG_ADAM, STEP, 0, 0]

    # cleared: the next step is the unguarded step from that state
    rec.zero_()
    a.restore(start)
    again = a.step(a.grads, guard=rec)
    assert not _same(plain, again) and rec.tolist() == [0, 0, 0, 0]

    # one +Inf gradient trips too (deliberately: see above)
    inf = a.grads.clone()
    inf[a.n - 1] = float('inf')
    a.restore(start)
    unguarded = a.step(inf)
    assert torch.isfinite(unguarded['p'][:-1]).all() and not torch.isfinite(unguarded['p'][-1])
    a.restore(start)
    tripped = a.step(inf, guard=rec)
    assert not _same(tripped, dict(start, g=inf), ('p', 'g', 'm', 'v', 'planes'))
    assert rec.tolist() == [ops.GUARD_TAG_ADAM, STEP, 0, 0]


def test_flat_adam_uses_the_guarded_launch_when_armed_also_without_truncation():
    """FlatAdam.guard: the same step as unguarded on finite gradients - with and without a clip threshold (the guard
    is handed the norm under a threshold that never clips) - and no step at all on a NaN gradient."""
    ops = _ops()
    from rl_games_amd.flat_optim import FlatAdam

    def make():
        torch.manual_seed(3)
        ps = [nn.Parameter(torch.randn(64, 12, device=DEV)), nn.Parameter(torch.randn(33, device=DEV)),
              nn.Parameter(torch.randn(6, device=DEV))]
        return FlatAdam(ps, LR)
    for max_norm in (None, 0.5):
        plain, armed = make(), make()
        armed.guard = ops.guard_record(DEV)
        g = torch.randn(plain.numel, generator=torch.Generator().manual_seed(4)).to(DEV)
        for o in (plain, armed):
            o.grads.copy_(g)
            o.step(max_norm=max_norm)
        for k in ('flat_params', 'exp_avg', 'exp_avg_sq', 'lr_slots'):
            assert torch.equal(getattr(plain, k), getattr(armed, k)), (max_norm, k)
        assert _bit_equal(plain.grads, armed.grads)
        before = armed.flat_params.clone()
        armed.grads.copy_(g)
        armed.grads[700] = float('nan')
        armed.step(max_norm=max_norm)
        assert torch.equal(armed.flat_params, before) and ops.read_guard(armed.guard) == (ops.GUARD_TAG_ADAM, 2)


# ----------------------------------------------------------------------------- MlpChain(products='exact')

def _chain_run(chain, layers, x, rows, split):
    """Training forward, inference forward and backward; everything the launches write."""
    heads = torch.full((rows, 9), float('nan'), device=DEV)
    infer = torch.full((rows, 9), float('nan'), device=DEV)
    acts = [torch.full((rows, 256), float('nan'), device=DEV), torch.full((rows, 128), float('nan'), device=DEV)]
    kw = {} if split is None else dict(split_products=split)
    chain.forward(x, heads, act_out=acts, **kw)
    chain.forward(x, infer, **kw)
    d = (1e-4 * torch.randn(rows, 9, generator=torch.Generator().manual_seed(rows))).to(DEV)
    dzs = [torch.full((rows, 256), float('nan'), device=DEV), torch.full((rows, 128), float('nan'), device=DEV)]
    nb = chain.num_blocks(rows, 1)
    parts = [torch.full((nb * 256,), float('nan'), dtype=torch.float64, device=DEV),
             torch.full((nb * 128,), float('nan'), dtype=torch.float64, device=DEV)]
    chain.backward(d, acts, dzs, parts, **kw)
    torch.cuda.synchronize()
    return [heads, infer] + acts + dzs + parts


@pytest.mark.parametrize('rows', [16, 4096, 8192, 16384])
def test_exact_chain_equals_split_products_false_and_has_no_range_limit(rows):
    """The net of test_split_fp16_range_limits_end_in_non_finite_values_never_in_wrong_ones.  16 and 4,096 rows run the
    lean 16-row kernels on an 'auto' chain, 8,192 the split training pair, 16,384 the split inference forward too."""
    ops = _ops()
    layers, g = _net(60, [256, 128], 9, 'elu', seed=32)
    x = torch.randn(rows, 60, generator=g).to(DEV)
    auto, exact = ops.MlpChain(layers, DEV), ops.MlpChain(layers, DEV, products='exact')
    assert exact.products == 'exact' and auto.products == 'auto'
    for kind in (0, 1, 2):
        assert auto.lean_used(rows, kind) or auto.split_products(rows, kind)
        assert not exact.lean_used(rows, kind) and not exact.split_products(rows, kind)
    want = _chain_run(auto, layers, x, rows, False)
    got = _chain_run(exact, layers, x, rows, None)
    for k, (a, b) in enumerate(zip(want, got)):
        assert torch.isfinite(b).all() and torch.equal(a, b), k
    assert exact.gradient_maxima(rows) is None and exact._planes is None and exact._frags is None
    # the attribute switches an existing chain over, and back
    auto.products = 'exact'
    for k, (a, b) in enumerate(zip(want, _chain_run(auto, layers, x, rows, None))):
        assert torch.equal(a, b), k
    auto.products = 'auto'
    # a row whose first-layer activations pass 4,094
    big = x.clone()
    big[5] *= 3e4
    ex = _chain_run(exact, layers, big, rows, None)
    au = _chain_run(auto, layers, big, rows, None)
    assert ex[2][5].abs().max() > 4094
    assert all(torch.isfinite(t).all() for t in ex)
    assert not torch.isfinite(au[0][5]).all() and not torch.isfinite(au[1][5]).all()
    # a weight of 2,000
    heavy = [(w.clone(), b.clone(), a) for w, b, a in layers]
    heavy[1][0][3, 7] = 2000.0
    ex = _chain_run(ops.MlpChain(heavy, DEV, products='exact'), heavy, x, rows, None)
    au = _chain_run(ops.MlpChain(heavy, DEV), heavy, x, rows, None)
    assert all(torch.isfinite(t).all() for t in ex)
    assert not torch.isfinite(au[3][:, 3]).any() and not torch.isfinite(au[0]).all()


def test_exact_one_launch_step_equals_forward_and_backward():
    """MlpChain.step under products='exact' takes the exact-product form of the one-launch step (never the lean one) and
    gives the bits of the exact forward + backward pair."""
    ops = _ops()
    rows, A = 128, 8
    layers, g = _net(60, [256, 128], 1 + A, 'elu', seed=33)
    x = torch.randn(rows, 60, generator=g).to(DEV)
    chain = ops.MlpChain(layers, DEV, products='exact')

    def buffers():
        return dict(heads=torch.empty(rows, 1 + A, device=DEV),
                    acts=[torch.empty(rows, 256, device=DEV), torch.empty(rows, 128, device=DEV)],
                    d_heads=torch.zeros(rows, 1 + A, device=DEV),
                    dzs=[torch.empty(rows, 256, device=DEV), torch.empty(rows, 128, device=DEV)],
                    parts=[torch.empty(chain.num_blocks(rows, 1) * w, dtype=torch.float64, device=DEV) for w in (256, 128)],
                    lossp=torch.zeros(max(ops.ppo_loss_blocks(rows), (rows + 15) // 16), ops.ppo_loss_partials_per_block(A),
                                      dtype=torch.float64, device=DEV))
    logstd = torch.zeros(A, device=DEV)
    actions = torch.randn(rows, A, generator=g).to(DEV)
    old_nlp = (torch.randn(rows, generator=g).abs() + 8).to(DEV)
    adv, old_v, ret = (torch.randn(rows, generator=g).to(DEV) for _ in range(3))
    old_mu, old_sigma = torch.randn(rows, A, generator=g).to(DEV), torch.ones(rows, A, device=DEV)

    def desc(b):
        return ops.ppo_loss_desc(b['heads'][:, 1:], logstd, b['heads'][:, 0], actions, old_nlp, adv, old_v, ret, old_mu,
                                 old_sigma, b['d_heads'][:, 1:], b['d_heads'][:, 0], b['lossp'], 0.2, 2.0, 1e-4)
    one, two = buffers(), buffers()
    d1, d2 = desc(one), desc(two)
    if not chain.step(x, one['heads'], one['acts'], one['d_heads'], one['dzs'], one['parts'], d1):
        pytest.fail('the exact one-launch step declined a 128-row minibatch')
    chain.forward(x, two['heads'], act_out=two['acts'])
    chain.backward(two['d_heads'], two['acts'], two['dzs'], two['parts'], ppo_loss=d2)
    torch.cuda.synchronize()
    assert chain.gradient_maxima(rows) is None and chain._frags is None
    assert torch.equal(one['heads'], two['heads']) and torch.equal(one['d_heads'], two['d_heads'])
    for k in ('acts', 'dzs'):
        for a, b in zip(one[k], two[k]):
            assert torch.isfinite(a).all() and torch.equal(a, b), k


# ----------------------------------------------------------------------------- weight gradients, form per launch

def test_weight_gradient_form_is_chosen_per_launch():
    """dz [4,096, 64], x [4,096, 60] with |x| up to 1e4.  The exact form is finite and within the bound the exact-product
    weight-gradient tests use (test_mlp_chain_gpu._close against fp64 and the library's fp32 product); the fp16 form
    splits x under the hidden activations' fixed scale 16 - 1e4 x 16 is past fp16 - and is non-finite; the library's
    choice without maxima is the bf16 form, bit for bit."""
    ops = _ops()
    rows = 4096
    g = torch.Generator().manual_seed(8)
    dz = (1e-3 * torch.randn(rows, 64, generator=g)).to(DEV)
    x = torch.randn(rows, 60, generator=g)
    x = (x * (1e4 / x.abs().max())).to(DEV)
    assert x.abs().max().item() == pytest.approx(1e4, rel=1e-6)
    t64, lib32 = dz.double().t() @ x.double(), dz.t() @ x
    plan = ops.MlpDwPlan([(64, 60)], rows, DEV)

    def run(**kw):
        grad = torch.full((64, 60), float('nan'), device=DEV)
        plan.launch([(dz, x, grad)], **kw)
        torch.cuda.synchronize()
        return grad
    exact = run(form='exact')
    assert torch.isfinite(exact).all()
    _close(exact, t64, lib32)
    entries = torch.zeros(8, 1024, device=DEV)
    entries[0, :rows // 64] = dz.abs().view(rows // 64, -1).max(dim=1).values
    maxima = (entries, [0], [ops.SPLIT_SCALE_HIDDEN], 64)
    assert not torch.isfinite(run(maxima=maxima, form='fp16')).all()
    assert not torch.isfinite(run(maxima=maxima)).all()              # (the library's choice with maxima: the fp16 form)
    assert torch.equal(run(maxima=maxima, form='exact'), exact)     # exact whatever maxima the step carries
    bf = run(form='bf16')
    _close(bf, t64, lib32)
    assert torch.equal(run(), bf) and torch.equal(run(form='auto'), bf)
    with pytest.raises(ValueError):
        run(form='fp32')
    with pytest.raises(Exception):
        run(form='fp16')                                             # no maxima: hipErrorInvalidValue, nothing launched


# ----------------------------------------------------------------------------- agents

def _linears(agent):
    return [m for m in agent.model.a2c_network.actor_mlp if isinstance(m, nn.Linear)]


def _poison(agent):
    """A trunk weight of 2,000 (limit of the fp16 planes: 1,023), written the way a user would - p.copy_().  It multiplies
    a unit pinned to 1e-3 (zero weights, bias 1e-3), so that on exact products the network is an ordinary one: 2,000 x
    1e-3 = 2; on fp16 planes the weight's plane is Inf and everything behind it is not finite."""
    first, second = _linears(agent)[:2]
    with torch.no_grad():
        w1, b1, w2 = first.weight.clone(), first.bias.clone(), second.weight.clone()
        w1[7, :] = 0.0
        b1[7] = 1e-3
        w2[3, 7] = 2000.0
        first.weight.copy_(w1)
        first.bias.copy_(b1)
        second.weight.copy_(w2)


def _state(agent):
    o = agent.optimizer
    out = [o.flat_params.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()]
    vm = getattr(agent, 'value_mean_std', None)
    if vm is not None:
        out += [vm.running_mean.clone(), vm.running_var.clone(), vm.count.clone()]
    cv = agent.central_value_net
    if cv is not None:
        out += [cv.optimizer.flat_params.clone(), cv.optimizer.exp_avg.clone(), cv.optimizer.exp_avg_sq.clone()]
    return out


def _unchanged(agent, before):
    return all(_bit_equal(a, b) for a, b in zip(_state(agent), before))


def _agent(cls=None, params=None, **over):
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    if params is None:
        params = configs.tiny(num_actors=64, horizon=8, minibatch_size=128, normalize_input=False)
    params = copy.deepcopy(params)
    params['config'].update(over)
    torch.manual_seed(5)
    agent = (cls or A2CAgent)('guard', params)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    return agent


def _epoch(agent):
    agent.update_epoch()
    return agent.train_epoch()


class _Spy:
    """Records the names of the library entries that are called."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def test_warn_is_todays_behaviour_and_todays_launches(monkeypatch):
    """Default policy: the guard is not armed - no scan launch, the unguarded optimiser entries, the library's own choice
    of weight-gradient form - and the poisoned epoch ends in non-finite parameters, with one warning."""
    from rl_games_amd import _lib
    agent = _agent()
    assert agent.split_range == 'warn' and agent.chain_products == 'auto' and agent._guard is None
    assert agent.optimizer.guard is None
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    _epoch(agent)
    assert torch.isfinite(agent.optimizer.flat_params).all()
    _poison(agent)
    with pytest.warns(RuntimeWarning, match='chain_products'):
        _epoch(agent)
    assert not torch.isfinite(agent.optimizer.flat_params).all()
    called = set(spy.names)
    assert not {'rlg_range_scan', 'rlg_adam_step_guarded', 'rlg_adam_pack_guarded', 'rlg_mlp_dw_launch_form'} & called
    assert {'rlg_adam_step', 'rlg_adam_step_pack'} & called and 'rlg_mlp_dw_launch' in called


def test_raise_on_a_rollout_trip_leaves_parameters_moments_and_value_statistics_alone(monkeypatch):
    from rl_games_amd import SplitRangeError, _lib, range_guard
    agent = _agent(split_range='raise')
    assert agent._guard is not None and agent.optimizer.guard is agent._guard
    _epoch(agent)
    _poison(agent)
    before = _state(agent)
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    with pytest.raises(SplitRangeError) as e:
        _epoch(agent)
    assert e.value.phase == 'rollout' and e.value.tag in (range_guard.TAG_VALUES, range_guard.TAG_NEGLOGPS)
    for word in ('rollout', '1023', '4094', f'flat index {e.value.index}'):
        assert word in str(e.value), word
    assert _unchanged(agent, before)
    assert spy.names.count('rlg_range_scan') == 1 and 'rlg_prepare_finalize' not in spy.names


@pytest.mark.parametrize('policy', ['raise', 'exact'])
def test_an_overflow_in_the_bootstrap_values_alone_is_a_rollout_trip(policy, capsys):
    """Only the observation BEHIND the last step of the rollout is large, in one env: every stored value, neglogp and mu
    is clean, but the bootstrap values - one more launch on the fp16 planes, kept in no buffer - are not, and they reach
    value_mean_std through the returns.  The scan runs behind that launch and covers the returns: a rollout trip, the
    offending index in env 5's rows, parameters, moments and value_mean_std bit-unchanged."""
    from rl_games_amd import SplitRangeError, range_guard
    agent = _agent(split_range=policy)
    _epoch(agent)
    H = agent.horizon_length
    step, calls = agent.env_step, []

    def env_step(*args, **kw):
        out = step(*args, **kw)
        calls.append(1)
        if len(calls) == H:
            out[0]['obs'][5] *= 1e5                      # raw observations (normalize_input: False), N(1, 3^2) x 1e5
        return out
    agent.env_step = env_step
    before = _state(agent)
    if policy == 'raise':
        with pytest.raises(SplitRangeError) as e:
            _epoch(agent)
        assert e.value.phase == 'rollout' and e.value.tag == range_guard.TAG_RETURNS
        assert e.value.index // H == 5 and 'returns' in str(e.value)
    else:
        capsys.readouterr()
        _epoch(agent)
        assert agent.chain_products == 'exact' and 'returns' in capsys.readouterr().out
    assert len(calls) == H and _unchanged(agent, before)
    st = agent.experience_buffer.storage
    assert all(torch.isfinite(st[k]).all() for k in ('values', 'neglogpacs', 'mus'))
    if policy == 'exact':
        # the large observation opens the next rollout: exact products take it
        agent.env_step = step
        out = _epoch(agent)
        assert all(torch.isfinite(x) for x in out[4] + out[5])
        assert all(torch.isfinite(t).all() for t in _state(agent))


def test_raise_on_an_update_trip_leaves_the_state_of_the_step_before():
    from rl_games_amd import SplitRangeError, range_guard
    agent = _agent(split_range='raise')
    _epoch(agent)
    steps = agent.optimizer.step_count
    seen = {}

    def after_steps():                                    # between prepare_dataset and the update
        _poison(agent)
        seen['state'] = _state(agent)
    agent.algo_observer.after_steps = after_steps
    with pytest.raises(SplitRangeError) as e:
        _epoch(agent)
    assert e.value.phase == 'update' and e.value.tag == range_guard.TAG_ADAM
    assert e.value.index == steps + 1                     # the first step of the epoch tripped: k = 0
    assert f'optimiser step {steps + 1}' in str(e.value)
    assert _unchanged(agent, seen['state'])


def test_exact_policy_drops_the_epoch_switches_to_exact_products_and_trains_on(capsys):
    agent = _agent(split_range='exact')
    for _ in range(2):
        out = _epoch(agent)                               # the second one on captured graphs
    assert all(torch.isfinite(x) for x in out[4] + out[5])
    sig_auto = agent._update_graphs.signature
    assert sig_auto is not None and (agent._update_graphs.epoch is not None or agent._update_graphs.minibatch)
    _poison(agent)
    before = _state(agent)
    capsys.readouterr()
    out = _epoch(agent)                                   # trips in the rollout: returns, nothing applied
    assert _unchanged(agent, before)
    assert agent.chain_products == 'exact' and agent._guard.tolist() == [0, 0, 0, 0]
    assert all(f.chain.products == 'exact' for f in agent._form_chains)
    assert agent._engine.weight_grads.form == 'exact' and agent._lean_chain() is None and agent._adam_pack_chain() is None
    params = agent.optimizer.flat_params.clone()
    for _ in range(2):
        out = _epoch(agent)
        assert all(torch.isfinite(x) for x in out[4] + out[5] + out[8])
    printed = capsys.readouterr().out
    assert printed.count('range guard tripped') == 1 and 'exact fp32 products' in printed
    assert torch.isfinite(agent.optimizer.flat_params).all() and not torch.equal(agent.optimizer.flat_params, params)
    # the update graphs were captured again, under another signature
    assert agent._update_graphs.signature != sig_auto
    assert agent._update_graphs.signature[-2:] == ('exact', True) and sig_auto[-2:] == ('auto', True)
    assert agent._update_graphs.epoch is not None or agent._update_graphs.minibatch


def test_exact_policy_on_an_update_trip_and_non_finite_inputs_on_exact_products():
    from rl_games_amd import SplitRangeError
    agent = _agent(split_range='exact')
    _epoch(agent)
    seen = {}

    def after_steps():
        if not seen:
            _poison(agent)
            seen['state'] = _state(agent)
    agent.algo_observer.after_steps = after_steps
    _epoch(agent)                                         # every step of this update is skipped on the device
    assert _unchanged(agent, seen['state']) and agent.chain_products == 'exact'
    out = _epoch(agent)
    assert all(torch.isfinite(x) for x in out[4] + out[5]) and not _unchanged(agent, seen['state'])
    # exact products and a non-finite parameter: the inputs are not finite - the step is skipped, recorded, and raised
    with torch.no_grad():
        w = _linears(agent)[0].weight
        bad = w.clone()
        bad[0, 0] = float('nan')
        w.copy_(bad)
    with pytest.raises(SplitRangeError, match='inputs'):
        _epoch(agent)


def test_chain_products_exact_from_the_start_matches_the_oracle():
    """One epoch on a recorded rollout against the CPU oracle, with the comparison and the tolerances of
    tests/test_agent_gpu.py::test_odd_shapes_match_oracle_epoch."""
    from oracle.ppo_epoch_oracle import OracleAgent
    from rl_games_amd import configs
    from rl_games_amd.synthetic_env import SyntheticTensorEnv
    N, H, obs_dim, act_dim = 64, 8, 12, 3
    params = configs.tiny(num_actors=N, horizon=H, obs_dim=obs_dim, act_dim=act_dim, minibatch_size=128, seq_length=1)
    agent = _agent(params=params, chain_products='exact')
    assert agent.chain_products == 'exact' and agent._guard is None
    assert all(f.chain.products == 'exact' for f in agent._form_chains) and agent._engine.weight_grads.form == 'exact'
    agent.set_eval()
    with torch.no_grad():
        batch = agent.play_steps()
    oracle = OracleAgent(copy.deepcopy(params), SyntheticTensorEnv(N, obs_dim, act_dim, device='cpu', seed=1))
    oracle.model.load_full_state_dict({k: v.detach().cpu().clone() for k, v in agent.model.state_dict().items()})
    ref = oracle.update({k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)})
    agent.set_train()
    agent.prepare_dataset(batch)
    vd = agent.dataset.values_dict
    assert torch.allclose(vd['advantages'].cpu(), oracle.dataset['advantages'], rtol=1e-5, atol=1e-6)
    k = 0
    for _ in range(agent.mini_epochs_num):
        for i in range(len(agent.dataset)):
            res = agent.train_actor_critic(agent.dataset[i])
            for got, key in ((res[0], 'a_loss'), (res[1], 'c_loss'), (res[2], 'entropy'), (res[3], 'kl'),
                             (res[8], 'b_loss')):
                print(k, key, got.item(), ref[k][key].item())
                assert np.isclose(got.item(), ref[k][key].item(), rtol=1e-5, atol=2e-6), (k, key, got.item(), ref[k][key].item())
            k += 1
    assert agent.optimizer.last_and_next_lr()[1] == oracle.lr
    final, want = agent.model.state_dict(), oracle.model.full_state_dict()
    steps = agent.mini_epochs_num * len(agent.dataset)
    for name, v in want.items():
        if v.is_floating_point():
            got = final[name].cpu().to(v.dtype)
            bad = ~torch.isclose(got, v, rtol=2e-3, atol=1e-5)
            assert bad.sum().item() <= max(2, 0.05 * v.numel()), (name, bad.sum().item(), v.numel())
            assert (got - v).abs().max().item() <= 2.1 * steps * max(oracle.lr, 3e-4), name
    assert agent._engine.chain._frags is None and agent._engine.chain._planes is None


def test_discrete_agent_raises_on_a_rollout_trip():
    """The smallest masked configuration of tests/test_discrete_gpu.py: multi-discrete heads behind separate trunks."""
    from rl_games_amd import SplitRangeError, configs
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    params = configs.cartpole_discrete(num_actors=16, use_action_masks=True)
    params['network']['space'] = {'multi_discrete': None}
    params['model']['name'] = 'multi_discrete_a2c'
    params['config']['env_config'].update(discrete_actions=[3, 5, 2], action_masks=True, autoreset_mode='same_step')
    agent = _agent(DiscreteA2CAgent, params, split_range='raise')
    assert agent._chains is not None and agent._guard is not None
    _epoch(agent)
    _poison(agent)
    before = _state(agent)
    with pytest.raises(SplitRangeError) as e:
        _epoch(agent)
    assert e.value.phase == 'rollout' and _unchanged(agent, before)
    # and the other policy: the discrete agent trains on, on exact products
    agent = _agent(DiscreteA2CAgent, params, split_range='exact')
    _epoch(agent)
    _poison(agent)
    _epoch(agent)
    assert agent.chain_products == 'exact' and all(c.chain.products == 'exact' and c.weight_grads.form == 'exact'
                                                   for c in agent._chains)
    out = _epoch(agent)
    assert all(torch.isfinite(x).all() for x in out[4] + out[5])


def test_central_value_agent_raises_on_a_rollout_trip():
    from rl_games_amd import SplitRangeError, configs, range_guard
    params = configs.tiny(num_actors=64, horizon=8, minibatch_size=128, normalize_input=False)
    params['config']['central_value_config'] = {
        'minibatch_size': 128, 'mini_epochs': 2, 'learning_rate': 5e-4, 'clip_value': True,
        'normalize_input': True, 'truncate_grads': True, 'grad_norm': 1.0,
        'network': {'name': 'actor_critic', 'central_value': True,
                    'mlp': {'units': [32, 16], 'activation': 'elu', 'initializer': {'name': 'default'}}}}
    params['config']['env_config']['state_dim'] = 9
    agent = _agent(params=params, split_range='raise')
    cv = agent.central_value_net
    assert cv.optimizer.guard is agent._guard and cv._engine is not None
    _epoch(agent)
    # a weight of 2,000 in the critic's trunk spoils the values - the critic's, the first array of the scan - and one in
    # the actor's the neglogps, the second
    second = [m for m in cv.model.a2c_network.actor_mlp if isinstance(m, nn.Linear)][1]
    with torch.no_grad():
        w = second.weight.clone()
        w[3, 7] = 2000.0
        second.weight.copy_(w)
    _poison(agent)
    before = _state(agent)
    with pytest.raises(SplitRangeError) as e:
        _epoch(agent)
    assert e.value.phase == 'rollout' and e.value.tag in (range_guard.TAG_CRITIC_VALUES, range_guard.TAG_NEGLOGPS)
    assert range_guard.TAG_NAMES[e.value.tag] in str(e.value) and _unchanged(agent, before)
    # chain_products reaches the critic's chain and its weight gradients
    agent = _agent(params=params, chain_products='exact')
    cv = agent.central_value_net
    assert cv.chain_products == 'exact' and cv._engine.chain.products == 'exact' and cv._engine.weight_grads.form == 'exact'
    out = _epoch(agent)
    assert all(torch.isfinite(x) for x in out[4] + out[5])


def test_two_armed_ranks_give_a_collective_verdict_and_stay_in_sync():
    """2 ranks on this box's single GPU (RLG_TEST_SINGLE_GPU=1: gloo collectives), the guard armed: every epoch ends in
    two collective verdicts (behind the rollout, behind the update, in front of the ranks' parameter check) and the
    guarded optimiser launches run behind the in-graph all-reduce; 4 epochs later parameters, statistics and learning
    rate are bit-identical on both ranks (tools/two_rank_check.py, as test_two_rank_training_keeps_ranks_in_sync runs it)."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RLG_TEST_SINGLE_GPU='1', RLG_TWO_RANK_CONFIG='{"split_range": "exact"}')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(root, 'tools', 'two_rank_check.py'), 'mlp']
    res = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert 'TWO_RANK_CHECK mlp in_sync' in res.stdout
