"""GPU: grad_sumsq_kernel + adam_step_kernel (csrc/optim.hip) and FlatAdam against an fp64 Adam step.

Reference = oracle.ppo_oracle.adam_step_fp64 (clip_grad_norm_ + torch's single-tensor Adam in fp64; shown to be just that
by tests/test_optim_cpu.py), applied to the fp32 state read back from the device in front of every step, so errors do not
accumulate.  Every element must satisfy |got - ref| <= K * 2^-24 * scale with the reference's own per-element scales and
the K_* of tests/test_optim_cpu.py (twice the error of the same op chain evaluated in numpy fp32 on these very inputs).
No floor is added: a scale is exactly 0 only where every term of the element is 0 (a zero gradient on zero moments),
and there the result is exact - such elements are compared with ==.  Bit equality is used between the project's own
forms only.  The pack form (adam_pack_kernel) has its tests next to its helper in tests/test_mlp_chain_gpu.py.
"""
import math

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from oracle import seeded_inputs as S
from test_optim_cpu import K_G, K_M, K_NORM, K_P, K_V, U, case_kwargs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = dict(p=K_P, g=K_G, m=K_M, v=K_V)
SCHEDULE = dict(kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulps(a, b):
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (x if x >= 0 else -(x & 0x7fffffff) for x in (ia, ib))
    return abs(ia - ib)


class Arena:
    """The four arenas of one optimiser plus its device scalars; `start` = steps already taken."""

    def __init__(self, p, m, v, start=0, lr=S.ADAM_LR, other_slot=0.0):
        self.p, self.m, self.v = _dev(p), _dev(m), _dev(v)
        self.g = torch.zeros_like(self.p)
        self.n = self.p.numel()
        self.counter = torch.tensor([start], dtype=torch.int64, device=DEV)
        slots = [other_slot, other_slot]
        slots[start & 1] = lr                                   # step s (1-based) reads slot (s - 1) & 1
        self.lr_slots = torch.tensor(slots, dtype=torch.float64, device=DEV)
        self.stats = torch.full((4,), -1.0, device=DEV)
        self.partials = torch.full((ops().grad_norm_blocks(self.n),), float('nan'), dtype=torch.float64, device=DEV)

    def clone(self):
        c = Arena.__new__(Arena)
        for k, x in vars(self).items():
            setattr(c, k, x.clone() if torch.is_tensor(x) else x)
        return c

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in 'pgmv'}

    def step(self, g, max_norm, grad_scale=1.0, partials=None, **kw):
        """grad_sumsq (advances the counter) + adam_step; `partials`: a norm-partials tensor given instead of the
        gradient's own."""
        self.g.copy_(_dev(g) if not torch.is_tensor(g) else g)
        ops().grad_sumsq(self.g, grad_scale, self.partials, self.counter)
        if partials is None:
            partials = self.partials if max_norm is not None else None
        ops().adam_step(self.p, self.g, self.m, self.v, partials, grad_scale, 0.0 if max_norm is None else max_norm,
                        self.lr_slots, self.counter, stats_out=self.stats, **kw)


def ops():
    from rl_games_amd import ops as _ops
    return _ops


def _check_elements(got, ref, what=''):
    for key in 'pgmv':
        r, x = ref[key], got[key].astype(np.float64)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(x), fin), (what, key, 'non-finite elements differ')
        scale = ref['scale'][key][fin]
        err = np.abs(x[fin] - r[fin])
        ratio = err[scale > 0] / (U * scale[scale > 0])
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f'{what} {key}: worst error {worst:.2f} x 2^-24 scale (bound {K[key]})')
        assert (err[scale == 0] == 0).all(), (what, key)
        assert worst <= K[key], (what, key, worst)


def _check_norm_and_clip(stats, ref, max_norm, what=''):
    norm32, clip32 = np.float32(stats[0]), np.float32(stats[1])
    if max_norm is None:
        assert norm32 == 0 and clip32 == 1
        return
    err = abs(float(norm32) - ref['norm']) / (U * ref['norm'])
    print(f'{what} norm: error {err:.2f} x 2^-24 norm (bound {K_NORM})')
    assert err <= K_NORM, (what, err)
    want = min(np.float32(max_norm) / (norm32 + np.float32(1e-6)), np.float32(1.0))
    assert _ulps(clip32, want) <= 2, (what, clip32, want)


# ----------------------------------------------------------------------------- a. grad_sumsq

@pytest.mark.parametrize('grad_scale', [1.0, 0.25, 1.0 / 3.0])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 2047, 2048, 2049, 524293])
def test_grad_sumsq_partials_counter_and_count(n, grad_scale):
    """524,293 elements are 257 blocks of 2,048: the cap of 256 sends block 0 on a second grid-stride trip."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen).numpy()
    blocks = ops().grad_norm_blocks(n)
    assert blocks == min(max((n + 2047) // 2048, 1), 256)
    want = math.fsum(((g * np.float32(grad_scale)).astype(np.float64) ** 2).tolist())   # fp32 products, exact squares
    dg = _dev(g)
    partials = torch.full((blocks + 3,), float('nan'), dtype=torch.float64, device=DEV)
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    ops().grad_sumsq(dg, grad_scale, partials[:blocks], counter)
    assert counter.item() == 42
    got = partials.cpu()
    assert torch.isnan(got[blocks:]).all() and torch.isfinite(got[:blocks]).all()       # exactly `blocks` partials
    assert abs(math.fsum(got[:blocks].tolist()) - want) <= n * 2.0 ** -52 * want
    again = torch.zeros(blocks, dtype=torch.float64, device=DEV)
    ops().grad_sumsq(dg, grad_scale, again, None)
    assert counter.item() == 42                                                          # untouched without a counter
    assert _same_bits(again, partials[:blocks]) and _same_bits(dg, _dev(g))


# ----------------------------------------------------------------------------- b. adam_step, option matrix

@pytest.mark.parametrize('case', S.ADAM_CASES, ids=S.adam_case_id)
def test_adam_step_option_matrix_against_fp64(case):
    n, _, _, gs, _, _, start = case
    inp = S.adam_inputs(case)
    kw = case_kwargs(case)
    a = Arena(inp['p'], inp['m'], inp['v'], start)
    lr = S.ADAM_LR
    for k, kl in enumerate(S.ADAM_KLS):
        before = a.state()
        step = start + k + 1
        a.step(inp['grads'][k], inp['max_norm'], gs, betas=kw['betas'], eps=kw['eps'], weight_decay=kw['weight_decay'],
               schedule_kind=1, kl=torch.tensor([kl], device=DEV), **SCHEDULE)
        ref = O.adam_step_fp64(before['p'], inp['grads'][k], before['m'], before['v'], step, lr, max_norm=inp['max_norm'],
                               **kw)
        what = f'{S.adam_case_id(case)} step {step}'
        _check_elements(a.state(), ref, what)
        stats = a.stats.cpu().numpy()
        _check_norm_and_clip(stats, ref, inp['max_norm'], what)
        assert a.counter.item() == step
        nxt = O.adaptive_lr(lr, float(np.float32(kl)))
        assert stats[2] == np.float32(lr) and stats[3] == np.float32(nxt)
        assert a.lr_slots[step & 1].item() == nxt and a.lr_slots[(step - 1) & 1].item() == lr
        lr = nxt


# ----------------------------------------------------------------------------- c. exact properties

def _case(n, trunc):
    return next(c for c in S.ADAM_CASES if c[0] == n and c[1] == trunc)


def test_inactive_truncation_at_scale_one_leaves_the_gradients_bit_unchanged():
    case = _case(1027, 'inactive')
    inp = S.adam_inputs(case)
    a = Arena(inp['p'], inp['m'], inp['v'])
    a.step(inp['grads'][0], 4 * inp['max_norm'], 1.0, weight_decay=1e-2)       # (the case's own grad_scale is 0.25)
    assert a.stats[1].item() == 1.0 and a.stats[0].item() > 0
    assert _same_bits(a.g, _dev(inp['grads'][0]))
    assert not _same_bits(a.p, _dev(inp['p']))


def test_skip_flag_leaves_everything_but_the_statistics_and_carries_the_learning_rate():
    case = _case(1027, 'inactive')
    inp = S.adam_inputs(case)
    kw = dict(weight_decay=1e-2, schedule_kind=1, kl=torch.tensor([1.0], device=DEV), **SCHEDULE)
    flag = torch.tensor([0, 7], dtype=torch.int32, device=DEV)
    res = {}
    for mode, skip in (('none', None), ('zero', flag[0:1].data_ptr()), ('set', flag[1:2].data_ptr())):
        a = Arena(inp['p'], inp['m'], inp['v'], start=1, other_slot=0.125)
        a.step(inp['grads'][0], 0.5, 1.0, skip_flag=skip, **kw)
        torch.cuda.synchronize()
        res[mode] = a
    a = res['set']
    for got, want in ((a.p, inp['p']), (a.g, inp['grads'][0]), (a.m, inp['m']), (a.v, inp['v'])):
        assert _same_bits(got, _dev(want))
    assert a.lr_slots.tolist() == [S.ADAM_LR, S.ADAM_LR]                        # (step 2 reads slot 1, writes slot 0)
    stats = a.stats.cpu().numpy()
    assert stats[0] > 0.5 and 0 < stats[1] < 1 and stats[2] == np.float32(S.ADAM_LR) and stats[3] == np.float32(S.ADAM_LR)
    # a flag word of 0 is no flag
    for key in ('p', 'g', 'm', 'v', 'lr_slots', 'stats'):
        assert _same_bits(getattr(res['zero'], key), getattr(res['none'], key)), key
    assert res['none'].lr_slots.tolist() == [O.adaptive_lr(S.ADAM_LR, 1.0), S.ADAM_LR]
    assert not _same_bits(res['none'].p, a.p)
    assert _same_bits(res['none'].stats[:3], a.stats[:3])


def test_two_launches_on_the_same_inputs_give_the_same_bits():
    case = _case(123921, 'active')
    inp = S.adam_inputs(case)
    kw = case_kwargs(case)
    gs = kw.pop('grad_scale')
    first = Arena(inp['p'], inp['m'], inp['v'], case[6])
    second = first.clone()
    for a in (first, second):
        a.step(inp['grads'][0], inp['max_norm'], gs, **kw)
    for key in ('p', 'g', 'm', 'v', 'lr_slots', 'stats', 'partials'):
        assert _same_bits(getattr(first, key), getattr(second, key)), key


def test_elements_are_updated_independently_of_their_position():
    """A pattern of period 7 over 1,027 elements: the same quadruple passes through every lane of the 4-wide vector
    threads of both blocks and through the three one-element tail threads."""
    gen = torch.Generator().manual_seed(7)
    n, reps = 1027, 1027 // 7 + 1
    p, g, m = (np.tile((torch.randn(7, generator=gen) * s).numpy(), reps)[:n] for s in (0.1, 0.5, 0.01))
    v = np.tile((torch.rand(7, generator=gen) * 1e-3).numpy(), reps)[:n]
    a = Arena(p, m, v, start=4)
    a.step(g, 0.5, 1.0 / 3.0, weight_decay=1e-2, betas=(0.8, 0.99), eps=1e-5)
    assert 0 < a.stats[1].item() < 1
    for key, x in a.state().items():
        bits = x.view(np.int32)
        assert np.array_equal(bits, np.tile(bits[:7], reps)[:n]), key
    assert not np.array_equal(a.state()['p'], p)


@pytest.mark.parametrize('start', [0, 1])
def test_the_slot_that_is_not_read_may_hold_anything(start):
    case = _case(1025, 'active')
    inp = S.adam_inputs(case)
    a = Arena(inp['p'], inp['m'], inp['v'], start, other_slot=float('nan'))
    lr = S.ADAM_LR
    for k in range(3):
        step = start + k + 1
        a.lr_slots[step & 1] = float('nan')                                    # step reads slot (step - 1) & 1
        a.step(inp['grads'][k], inp['max_norm'], 1.0, schedule_kind=1, kl=torch.tensor([0.001], device=DEV), **SCHEDULE)
        st = a.state()
        assert all(np.isfinite(st[key]).all() for key in 'pgmv')
        assert torch.isfinite(a.stats).all()
        nxt = O.adaptive_lr(lr, float(np.float32(0.001)))
        assert a.lr_slots[step & 1].item() == nxt and a.lr_slots[(step - 1) & 1].item() == lr
        lr = nxt
    assert lr == S.ADAM_LR * 1.5 * 1.5 * 1.5


# ----------------------------------------------------------------------------- d. learning-rate rule

def test_learning_rate_rule_at_its_bounds_and_clamps():
    thr = 0.0078125                                   # 2 * thr and 0.5 * thr are exact in fp32
    sched = dict(kl_threshold=thr, min_lr=1e-6, max_lr=1e-2, lr_multiplier=1.5)
    f32 = np.float32
    up, down = (lambda x: float(np.nextafter(f32(x), f32(np.inf)))), (lambda x: float(np.nextafter(f32(x), f32(-np.inf))))
    rows = []                                         # (lr, kl, kl_scale)
    for bound in (2 * thr, 0.5 * thr):
        rows += [(3e-4, up(bound), 1.0), (3e-4, bound, 1.0), (3e-4, down(bound), 1.0)]
        rows += [(3e-4, 4 * up(bound), 0.25), (3e-4, 4 * bound, 0.25), (3e-4, 4 * down(bound), 0.25)]
    rows += [(1.2e-6, 1.0, 1.0), (1e-6, 1.0, 1.0), (8e-3, 0.0, 1.0), (1e-2, 0.0, 1.0), (3e-4, thr, 1.0)]
    seen = set()
    for lr, kl, kl_scale in rows:
        for kind in (1, 0):
            a = Arena(np.ones(5, f32), np.zeros(5, f32), np.zeros(5, f32), start=2, lr=lr, other_slot=-1.0)
            a.step(np.ones(5, f32), 1.0, 1.0, schedule_kind=kind, kl=torch.tensor([kl], device=DEV), kl_scale=kl_scale,
                   **sched)
            want = O.adaptive_lr(lr, float(f32(kl) * f32(kl_scale)), **sched) if kind == 1 else lr
            got = a.lr_slots.tolist()
            assert got[0] == lr and got[1] == want, (lr, kl, kl_scale, kind, got, want)     # step 3 reads 0, writes 1
            assert a.stats[3].item() == f32(want)
            if kind == 1:
                seen.add('down' if want < lr else 'up' if want > lr else 'keep')
                seen.add('min' if want == 1e-6 else 'max' if want == 1e-2 else '')
    assert seen >= {'down', 'up', 'keep', 'min', 'max'}
    # the bounds themselves belong to "keep": both inequalities are strict
    assert O.adaptive_lr(3e-4, 2 * thr, **sched) == 3e-4 == O.adaptive_lr(3e-4, 0.5 * thr, **sched)


# ----------------------------------------------------------------------------- e. norm-partials reduction

NORM_PARTIAL_COUNTS = [1, 255, 256, 257, 768, 769, 1023, 1024, 1025, 1793, 2311, 4100]


def norm_partials_case(count):
    """(device tensor [count + 64]: `count` positive fp64 partials, NaN behind them; the norm they give, as fp32)"""
    gen = torch.Generator().manual_seed(count)
    vals = torch.rand(count, generator=gen, dtype=torch.float64) * 1e-3 + 1e-9
    buf = torch.full((count + 64,), float('nan'), dtype=torch.float64)
    buf[:count] = vals
    return buf.to(DEV), np.float32(math.sqrt(math.fsum(vals.tolist())))


@pytest.mark.parametrize('count', NORM_PARTIAL_COUNTS)
def test_norm_partials_of_another_launch_are_all_summed_once(count):
    """The 4-way unrolled loop starts at 769 partials; the finalise launch leaves about 2,300."""
    case = _case(1027, 'inactive')
    inp = S.adam_inputs(case)
    buf, want = norm_partials_case(count)
    a = Arena(inp['p'], inp['m'], inp['v'])
    a.step(inp['grads'][0], 0.25, 1.0, partials=buf[:count])
    stats = a.stats.cpu().numpy()
    assert _ulps(stats[0], want) <= 1, (stats[0], want)
    assert _ulps(stats[1], min(np.float32(0.25) / (np.float32(stats[0]) + np.float32(1e-6)), np.float32(1.0))) <= 2
    st = a.state()
    assert all(np.isfinite(st[key]).all() for key in 'pgmv') and np.isfinite(stats).all()


# ----------------------------------------------------------------------------- f. non-finite gradients

def _nonfinite_run(bad, truncate):
    case = S.ADAM_NONFINITE_CASE
    inp = S.adam_inputs(case)
    g = inp['grads'][0].copy()
    g[S.ADAM_NONFINITE_INDEX] = bad
    kw = case_kwargs(case)
    max_norm = inp['max_norm'] if truncate else None
    a = Arena(inp['p'], inp['m'], inp['v'], case[6])
    a.step(g, max_norm, kw['grad_scale'], betas=kw['betas'], eps=kw['eps'], weight_decay=kw['weight_decay'])
    ref = O.adam_step_fp64(inp['p'], g, inp['m'], inp['v'], case[6] + 1, S.ADAM_LR, max_norm=max_norm, **kw)
    tp, tm, tv, _ = O.clip_and_adam_reference(*([torch.from_numpy(x)] for x in (inp['p'], g, inp['m'], inp['v'])),
                                              case[6], S.ADAM_LR, max_norm if truncate else 1.0, truncate,
                                              betas=kw['betas'], eps=kw['eps'], weight_decay=kw['weight_decay'])
    return a, ref, dict(p=tp[0].numpy(), m=tm[0].numpy(), v=tv[0].numpy())


def test_one_infinite_gradient_spoils_one_element():
    a, ref, torch_ref = _nonfinite_run(np.inf, True)
    st = a.state()
    only = np.zeros(a.n, bool)
    only[S.ADAM_NONFINITE_INDEX] = True
    for key in 'pgmv':
        assert np.array_equal(~np.isfinite(st[key]), only), key
        assert np.array_equal(~np.isfinite(ref[key]), only), key
    for key in 'pmv':
        assert np.array_equal(~np.isfinite(torch_ref[key]), only), key
    _check_elements(st, ref, 'inf gradient')
    assert math.isinf(a.stats[0].item()) and a.stats[1].item() == 0.0


def test_one_nan_gradient_spoils_everything_under_truncation_like_clip_grad_norm():
    """torch.clamp(max=1.0) propagates a NaN norm into the coefficient (fminf alone would answer 1)."""
    a, ref, torch_ref = _nonfinite_run(np.nan, True)
    st = a.state()
    for key in 'pgmv':
        assert np.isnan(st[key]).all() and np.isnan(ref[key]).all(), key
    for key in 'pmv':
        assert np.isnan(torch_ref[key]).all(), key
    assert math.isnan(a.stats[0].item()) and math.isnan(a.stats[1].item())


def test_one_nan_gradient_spoils_one_element_without_truncation():
    a, ref, torch_ref = _nonfinite_run(np.nan, False)
    st = a.state()
    only = np.zeros(a.n, bool)
    only[S.ADAM_NONFINITE_INDEX] = True
    for key in 'pgmv':
        assert np.array_equal(np.isnan(st[key]), only) and np.array_equal(~np.isfinite(ref[key]), only), key
    for key in 'pmv':
        assert np.array_equal(np.isnan(torch_ref[key]), only), key
    _check_elements(st, ref, 'nan gradient, no truncation')


def test_zero_gradients_on_zero_moments_change_nothing():
    n = 1027
    p = S.adam_inputs(_case(1027, 'inactive'))['p']
    z = np.zeros(n, np.float32)
    a = Arena(p, z, z)
    a.step(z, 1.0, 1.0)
    st = a.state()
    assert np.array_equal(st['p'].view(np.int32), p.view(np.int32))
    assert all((st[key] == 0).all() for key in 'gmv')
    assert a.stats[0].item() == 0.0 and a.stats[1].item() == 1.0


# ----------------------------------------------------------------------------- h. FlatAdam

def _flat_adam(values, lr):
    from rl_games_amd.flat_optim import FlatAdam
    _, _, wd, _, betas, eps, _ = S.ADAM_FLAT_CASE
    params, off = [], 0
    for shape in S.ADAM_FLAT_SHAPES:
        k = int(np.prod(shape))
        params.append(torch.nn.Parameter(_dev(values[off:off + k]).view(shape).clone()))
        off += k
    return FlatAdam(params, lr, betas=betas, eps=eps, weight_decay=wd)


def test_flat_adam_state_dict_round_trip_and_torch_adam_continue_the_same_run():
    """Three steps; state_dict() into a fresh FlatAdam: a fourth step on both gives the same bits and the same learning
    rate.  The same state_dict loaded into torch.optim.Adam on an fp64 CPU copy of the parameters (load_state_dict casts
    the moments to the parameters' type): its fourth step on the device's clipped gradients is the fp64 reference of the
    device's - torch's fp32 step is not one (tests/test_optim_cpu.py) - to the tolerance of the option matrix."""
    case = S.ADAM_FLAT_CASE
    inp = S.adam_inputs(case, S.ADAM_FLAT_STEPS, zero_moments=True)
    max_norm = inp['max_norm']
    opt = _flat_adam(inp['p'], S.ADAM_LR)
    assert opt.numel == case[0]
    lr = S.ADAM_LR
    for k in range(3):
        opt.grads.copy_(_dev(inp['grads'][k]))
        opt.kl_slot.fill_(S.ADAM_FLAT_KL)
        opt.step(1.0, max_norm, SCHEDULE)
        lr = O.adaptive_lr(lr, float(np.float32(S.ADAM_FLAT_KL)))
    sd = opt.state_dict()
    assert sd['param_groups'][0]['lr'] == lr != S.ADAM_LR
    before = {k: x.cpu().numpy().copy() for k, x in (('p', opt.flat_params), ('m', opt.exp_avg), ('v', opt.exp_avg_sq))}
    fresh = _flat_adam(before['p'], 1.0)                       # (an lr that the state_dict must replace)
    fresh.load_state_dict(sd)
    cpu_params = [torch.nn.Parameter(p.detach().cpu().double()) for p in opt.params]
    topt = torch.optim.Adam(cpu_params, 1.0)
    topt.load_state_dict(sd)
    for o in (opt, fresh):
        o.grads.copy_(_dev(inp['grads'][3]))
        o.kl_slot.fill_(S.ADAM_FLAT_KL)
        o.step(1.0, max_norm, SCHEDULE)
    for key in ('flat_params', 'grads', 'exp_avg', 'exp_avg_sq', 'stats', 'step_counter'):
        assert _same_bits(getattr(opt, key), getattr(fresh, key)), key
    assert opt.current_lr() == fresh.current_lr() == O.adaptive_lr(lr, float(np.float32(S.ADAM_FLAT_KL)))
    assert opt.last_and_next_lr() == fresh.last_and_next_lr()
    # torch.optim.Adam, fp64, on the clipped gradients the device left
    for p, (off, cnt) in zip(cpu_params, opt.offsets):
        p.grad = opt.grads[off:off + cnt].view(p.shape).cpu().double()
    topt.step()
    got = {'p': opt.flat_params.cpu().numpy(), 'g': opt.grads.cpu().numpy(), 'm': opt.exp_avg.cpu().numpy(),
           'v': opt.exp_avg_sq.cpu().numpy()}
    ref = O.adam_step_fp64(before['p'], inp['grads'][3], before['m'], before['v'], 4, lr, max_norm=max_norm,
                           **case_kwargs(case))
    _check_elements(got, ref, 'FlatAdam step 4 against adam_step_fp64')
    _check_norm_and_clip(opt.stats.cpu().numpy(), ref, max_norm, 'FlatAdam step 4')
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).numpy()
    tref = dict(ref, p=flat(cpu_params), m=flat([topt.state[p]['exp_avg'] for p in cpu_params]),
                v=flat([topt.state[p]['exp_avg_sq'] for p in cpu_params]), g=got['g'].astype(np.float64))
    _check_elements(got, tref, 'FlatAdam step 4 against torch.optim.Adam in fp64')
