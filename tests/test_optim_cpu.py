"""CPU: the fp64 reference of the optimiser step and the tolerance the device tests hold the kernels to.

tests/test_optim_gpu.py compares adam_step_kernel / adam_pack_kernel with oracle.ppo_oracle.adam_step_fp64, element by
element, to K * 2^-24 * scale (the scales are the reference's own: see its docstring).  Two things are settled here,
without a GPU:

 * adam_step_fp64 IS the reference's algorithm: it agrees with clip_grad_norm_ + torch.optim.Adam on fp64 parameters to
   1e-12.  (torch's fp32 Adam is no yardstick for single elements: it accumulates the norm in fp32 and its moments pass
   near zero, where a few roundings are 1e5 ulps.)
 * the K_* constants: the error of the kernels' own op chain evaluated in numpy fp32 (adam_step_f32_emulation, one rounding
   per operation) against adam_step_fp64, on every input set the device tests use (oracle.seeded_inputs), in units of
   2^-24 * scale.  K = twice the worst measured ratio, rounded up: the device's double pow / sqrt and its fp32 divide may
   each round one step differently from numpy's.  The test below holds the emulation to K / 2, so inputs and constants
   cannot drift apart.
"""
import math

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from oracle import seeded_inputs as S

U = 2.0 ** -24

# worst ratios measured over S.ADAM_CASES (3 steps each), S.ADAM_NONFINITE_CASE (inf with, NaN without truncation) and the
# fourth step of S.ADAM_FLAT_CASE:
#   p 4.16   g 0.76   m 1.26   v 3.93   norm 0.79
K_P, K_G, K_M, K_V, K_NORM = 9, 2, 3, 8, 2
K = dict(p=K_P, g=K_G, m=K_M, v=K_V, norm=K_NORM)


def case_kwargs(case):
    _, _, wd, gs, betas, eps, _ = case
    return dict(grad_scale=gs, betas=betas, eps=eps, weight_decay=wd)


def error_ratios(got, ref):
    """Worst |got - ref| / (2^-24 * scale) per quantity over the elements where the reference is finite; the non-finite
    elements must be the same ones."""
    out = {}
    for key in 'pgmv':
        r, x = ref[key], np.asarray(got[key], dtype=np.float64)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(x), fin), key
        scale = ref['scale'][key][fin]
        err = np.abs(x[fin] - r[fin])
        assert (err[scale == 0] == 0).all(), key           # (scale 0: every term of the element is 0 - the result is exact)
        out[key] = float((err[scale > 0] / (U * scale[scale > 0])).max()) if (scale > 0).any() else 0.0
    out['norm'] = abs(float(got['norm']) - ref['norm']) / (U * ref['norm']) if ref['norm'] > 0 and math.isfinite(ref['norm']) else 0.0
    return out


def calibration_sets():
    """(id, case, inputs, steps, first compared step) of every input set of the device tests.  The FlatAdam round trip
    compares its fourth step only; the three before it build the state.  (Its first step starts from zero moments with
    weight decay: where g_c and wd * p cancel, v' = w2 * (g_c + wd * p)^2 has no other term to be measured against and
    the ratio of that step is unbounded - 46 here - for the emulation as for any fp32 evaluation.)"""
    sets = [(S.adam_case_id(c), c, S.adam_inputs(c), S.ADAM_STEPS, 0) for c in S.ADAM_CASES]
    nf = S.adam_inputs(S.ADAM_NONFINITE_CASE)
    nf['grads'][0][S.ADAM_NONFINITE_INDEX] = np.inf
    sets.append(('inf gradient', S.ADAM_NONFINITE_CASE, nf, 1, 0))
    nan = S.adam_inputs(S.ADAM_NONFINITE_CASE)
    nan['grads'][0][S.ADAM_NONFINITE_INDEX] = np.nan
    sets.append(('nan gradient, no truncation', S.ADAM_NONFINITE_CASE, dict(nan, max_norm=None), 1, 0))
    sets.append(('flat', S.ADAM_FLAT_CASE, S.adam_inputs(S.ADAM_FLAT_CASE, S.ADAM_FLAT_STEPS, zero_moments=True),
                 S.ADAM_FLAT_STEPS, S.ADAM_FLAT_STEPS - 1))
    return sets


def measure():
    worst = dict(p=0.0, g=0.0, m=0.0, v=0.0, norm=0.0)
    for _, case, inp, steps, first in calibration_sets():
        p, m, v = inp['p'], inp['m'], inp['v']
        lr = S.ADAM_LR
        kls = [S.ADAM_FLAT_KL] * steps if case is S.ADAM_FLAT_CASE else S.ADAM_KLS
        for k in range(steps):
            args = (p, inp['grads'][k], m, v, case[6] + k + 1, lr)
            ref = O.adam_step_fp64(*args, max_norm=inp['max_norm'], **case_kwargs(case))
            emu = O.adam_step_f32_emulation(*args, max_norm=inp['max_norm'], **case_kwargs(case))
            for key, r in error_ratios(emu, ref).items():
                if k >= first:
                    worst[key] = max(worst[key], r)
            p, m, v = emu['p'], emu['m'], emu['v']              # (carry the fp32 state, like the device)
            lr = O.adaptive_lr(lr, float(np.float32(kls[k])))
    return worst


def test_tolerance_constants_cover_the_fp32_op_chain_twice():
    worst = measure()
    print({k: round(x, 2) for k, x in worst.items()})
    for key, x in worst.items():
        assert x <= K[key] / 2, (key, x, K[key])
        assert K[key] == math.ceil(2 * x), (key, x, K[key])              # (twice the measured value, rounded up)


@pytest.mark.parametrize('max_norm', [None, 0.5])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.8, 0.99)])
def test_adam_step_fp64_is_clip_grad_norm_and_torch_adam_in_fp64(max_norm, wd, betas):
    """Four steps.  Each starts from fp32 state (the previous result rounded, what the device tests hand to the
    reference) promoted to fp64 parameters and moments of a torch.optim.Adam at that step count."""
    gen = torch.Generator().manual_seed(3)
    n = 257
    p = (torch.randn(n, generator=gen) * 0.1).numpy()
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    clipped_steps = 0
    for step in range(1, 5):
        g = (torch.randn(n, generator=gen) * (3.0 if step == 1 else 0.01)).numpy()
        tp = torch.nn.Parameter(torch.from_numpy(p).double())
        tp.grad = torch.from_numpy(g).double()
        norm = torch.nn.utils.clip_grad_norm_([tp], max_norm).item() if max_norm is not None else 0.0
        clipped = tp.grad.clone().numpy()
        opt = torch.optim.Adam([tp], 3e-4, betas=betas, eps=1e-8, weight_decay=wd)
        opt.state[tp] = {'step': torch.tensor(float(step - 1)), 'exp_avg': torch.from_numpy(m).double(),
                         'exp_avg_sq': torch.from_numpy(v).double()}
        opt.step()
        ref = O.adam_step_fp64(p, g, m, v, step, 3e-4, 1.0, max_norm, betas, 1e-8, wd)
        st = opt.state[tp]
        for got, want in ((tp.detach().numpy(), ref['p']), (clipped, ref['g']), (st['exp_avg'].numpy(), ref['m']),
                          (st['exp_avg_sq'].numpy(), ref['v'])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert abs(norm - ref['norm']) <= 1e-12 * max(ref['norm'], 1e-300)
        clipped_steps += ref['clip'] < 1.0
        p, m, v = (ref[k].astype(np.float32) for k in 'pmv')
    assert max_norm is None or 0 < clipped_steps < 4             # with and without an active clip


def test_nan_and_inf_gradients_like_clip_grad_norm():
    """One NaN gradient among six turns everything into NaN when truncation is on (torch.clamp propagates NaN), one inf
    gradient exactly one element; without truncation only the element itself."""
    base = dict(step=1, lr=3e-4, grad_scale=1.0)
    p = np.linspace(-1, 1, 6).astype(np.float32)
    z = np.zeros(6, np.float32)
    for bad, max_norm, want in ((np.nan, 1.0, 6), (np.inf, 1.0, 1), (np.nan, None, 1), (np.inf, None, 1)):
        g = np.full(6, 0.5, np.float32)
        g[2] = bad
        ref = O.adam_step_fp64(p, g, z, z, max_norm=max_norm, **base)
        emu = O.adam_step_f32_emulation(p, g, z, z, max_norm=max_norm, **base)
        tp, _, _, _ = O.clip_and_adam_reference([torch.from_numpy(p)], [torch.from_numpy(g)], [torch.zeros(6)],
                                                [torch.zeros(6)], 0, 3e-4, 1.0, max_norm is not None)
        for x in (ref['p'], emu['p'], tp[0].numpy()):
            assert int((~np.isfinite(x)).sum()) == want, (bad, max_norm, x)
