"""GPU: the players' kernels (csrc/play.hip) against the rollout heads they must agree with bit for bit, torch.argmax
on the CPU, and the statements of the player's host loop.  Seeded inputs; every output sits between guard rows of a
sentinel that must survive the launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -777.0
GUARD = 3


def _gen(seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return g


class _Guarded:
    """A [rows, cols] output (cols 0: [rows]) between GUARD rows of the sentinel on either side."""

    def __init__(self, rows, cols, dtype):
        shape = (rows + 2 * GUARD,) + ((cols,) if cols else ())
        self.buf = torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
        self.out = self.buf[GUARD:GUARD + rows]

    def check(self):
        assert (self.buf[:GUARD] == SENTINEL).all() and (self.buf[-GUARD:] == SENTINEL).all(), 'wrote outside its rows'
        return self.out


def _heads(rows, A, view, seed):
    """[rows, 1 + A] heads, contiguous or the leading columns of a [rows, 1 + A + 5] buffer."""
    full = torch.randn(rows, 1 + A + (5 if view else 0), generator=_gen(seed)).to(DEV)
    return full[:, :1 + A]


# ----------------------------------------------------------------------------- continuous head

def _rollout_head(heads, logstd, noise, bounds):
    """actions_out / env_actions_out of rlg_rollout_policy_head on the same inputs."""
    from rl_games_amd import ops
    rows, A = noise.shape
    storage = {k: torch.empty(rows, 1, A, device=DEV) for k in ('actions', 'mus', 'sigmas')}
    storage.update({k: torch.empty(rows, 1, device=DEV) for k in ('neglogpacs', 'values')})
    actions, values, env = torch.empty(rows, A, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, A, device=DEV)
    ops.rollout_policy_head(heads.contiguous(), logstd, noise, None, 1e-5, actions, values, storage, 1, 0,
                            env_actions=None if bounds is None else (env,) + bounds)
    return actions if bounds is None else env


def _bounds(A, seed):
    lo = -1.0 - torch.rand(A, generator=_gen(seed))
    hi = 0.5 + 2.0 * torch.rand(A, generator=_gen(seed + 1))
    return lo.to(DEV), hi.to(DEV)


@pytest.mark.parametrize('view', [False, True])
@pytest.mark.parametrize('A', [1, 3, 8])
@pytest.mark.parametrize('rows', [1, 63, 64, 65, 257])
def test_continuous_head_is_the_rollout_heads_action(rows, A, view):
    from rl_games_amd import ops
    from rl_games_amd.agent import rescale_actions
    heads = _heads(rows, A, view, 11 * rows + A)
    heads[0, 1] = 3.0                                    # something for the clamp to do
    logstd = (0.3 * torch.randn(A, generator=_gen(5))).to(DEV)
    noise = torch.randn(rows, A, generator=_gen(rows + 7 * A)).to(DEV)
    for bounds in (None, _bounds(A, 3)):
        out = _Guarded(rows, A, torch.float32)
        ops.play_policy_head(heads[:, 1:], logstd, noise, out.out, bounds)
        assert torch.equal(out.check(), _rollout_head(heads, logstd, noise, bounds)), 'stochastic'
        # deterministic: the means, whatever logstd holds
        out = _Guarded(rows, A, torch.float32)
        ops.play_policy_head(heads[:, 1:], torch.full_like(logstd, float('inf')), None, out.out, bounds)
        mu = heads[:, 1:1 + A]
        want = mu if bounds is None else rescale_actions(bounds[0], bounds[1], torch.clamp(mu, -1.0, 1.0))
        assert torch.equal(out.check(), want), 'deterministic'


def test_continuous_head_nan_inf_and_degenerate_bounds():
    from rl_games_amd import ops
    rows, A = 65, 3
    heads = _heads(rows, A, True, 2)
    heads[3, 1], heads[4, 2], heads[5, 3], heads[64, 3] = float('nan'), float('inf'), float('-inf'), float('nan')
    lo, hi = _bounds(A, 9)
    out = _Guarded(rows, A, torch.float32)
    ops.play_policy_head(heads[:, 1:], None, None, out.out, (lo, hi))
    got = out.check()
    assert torch.isnan(got[3, 0]) and torch.isnan(got[64, 2])
    d, m = (hi - lo) / 2.0, (hi + lo) / 2.0
    assert got[4, 1] == (1.0 * d + m)[1] and got[5, 2] == (-1.0 * d + m)[2]
    assert torch.isnan(got).sum() == 2
    # lo == hi: every finite action is the bound itself, NaN stays NaN
    same = torch.tensor([0.25, -2.0, 0.0], device=DEV)
    out = _Guarded(rows, A, torch.float32)
    ops.play_policy_head(heads[:, 1:], None, None, out.out, (same, same.clone()))
    got = out.check()
    finite = ~torch.isnan(heads[:, 1:1 + A])
    assert torch.equal(got[finite], same.expand(rows, A)[finite]) and torch.isnan(got[~finite]).all()
    # unclipped: the values pass through
    out = _Guarded(rows, A, torch.float32)
    ops.play_policy_head(heads[:, 1:], None, None, out.out, None)
    assert torch.equal(torch.nan_to_num(out.check(), 7.0), torch.nan_to_num(heads[:, 1:1 + A], 7.0))


# ----------------------------------------------------------------------------- categorical head

BRANCHES = [[3], [3, 4], [130], [2] * 16]


def _exp_noise(rows, sizes, seed):
    return torch.empty(rows * sum(sizes)).exponential_(generator=_gen(seed)).to(DEV)


def _rollout_categorical(logits, sizes, noise, masks):
    from rl_games_amd import ops
    rows, B = logits.shape[0], len(sizes)
    storage = {'actions': torch.empty(rows, 1, B, dtype=torch.int64, device=DEV),
               'neglogpacs': torch.empty(rows, 1, device=DEV), 'values': torch.empty(rows, 1, device=DEV)}
    actions = torch.empty(rows, B, dtype=torch.int64, device=DEV)
    ops.rollout_categorical_head(logits, torch.zeros(rows, 1, device=DEV), sizes, noise, masks, None, 1e-5, actions,
                                 torch.empty(rows, device=DEV), storage, 1, 0)
    return actions


def _masks(rows, sizes, seed, pad=0):
    S = sum(sizes)
    full = torch.rand(rows, S + pad, generator=_gen(seed)) > 0.4
    at = 0
    for n in sizes:                                       # at least one allowed action per branch
        full[torch.arange(rows), at + torch.randint(0, n, (rows,), generator=_gen(seed + at + 1))] = True
        at += n
    return full.to(DEV)[:, :S]


@pytest.mark.parametrize('sizes', BRANCHES, ids=str)
@pytest.mark.parametrize('rows', [1, 65, 257])
def test_categorical_sample_is_the_rollout_heads(rows, sizes):
    from rl_games_amd import ops
    S, B = sum(sizes), len(sizes)
    logits = (2.0 * torch.randn(rows, 1 + S + 2, generator=_gen(rows + S))).to(DEV)[:, 1:1 + S]     # strided
    noise = _exp_noise(rows, sizes, 3 * rows + S)
    for masks in (None, _masks(rows, sizes, 17, pad=3)):                                            # strided masks
        out = _Guarded(rows, B, torch.int64)
        ops.play_categorical_head(logits, sizes, noise, masks, out.out)
        got = out.check()
        assert torch.equal(got, _rollout_categorical(logits, sizes, noise, masks))
        if masks is not None:
            at = 0
            for b, n in enumerate(sizes):
                assert masks.gather(1, (at + got[:, b]).view(-1, 1)).all(), 'a masked action was sampled'
                at += n


def _crafted(sizes, rows, seed):
    """(logits, masks) on the CPU whose first rows hold the arg-max's edge cases in EVERY branch: ties, NaN in the
    first / middle / last place and twice, an all-masked row, a row whose only allowed action is the last, a NaN under
    the mask, and - wide branches - ties across the 64-lane boundary."""
    S = sum(sizes)
    logits = 2.0 * torch.randn(rows, S, generator=_gen(seed))
    masks = torch.rand(rows, S, generator=_gen(seed + 1)) > 0.3
    nan = float('nan')
    at = 0
    for n in sizes:
        x, m = logits[:, at:at + n], masks[:, at:at + n]
        m[:14] = True
        x[0] = 0.5                                            # every column ties
        x[1, n - 1] = x[1, 0] = 9.0                           # first and last tie for the maximum
        x[2, 0], x[3, n // 2], x[4, n - 1] = nan, nan, nan
        x[5, n - 1] = x[5, n // 2] = nan                      # two NaN: the first one wins
        x[6, 0] = 50.0                                        # NaN behind the maximum still wins
        x[6, n - 1] = nan
        m[7] = False                                          # all masked: every logit is -1e8, action 0
        m[8] = False
        m[8, n - 1] = True                                    # only the last action is allowed
        x[9, 0] = nan                                         # a NaN under the mask is -1e8, not NaN
        m[9, 0] = False
        if n > 64:
            x[10, 5] = x[10, 69] = 20.0                       # one lane, two of its columns
            x[11, 63] = x[11, 64] = 20.0                      # the last lane and the first of the next round
            x[12, 64] = x[12, 3] = 20.0
            x[13, 129] = 20.0
            x[13, 64] = nan                                   # NaN in a later round beats an earlier maximum
        at += n
    return logits, masks


@pytest.mark.parametrize('sizes', BRANCHES, ids=str)
def test_categorical_argmax_is_torch_argmax_on_the_cpu(sizes):
    from rl_games_amd import ops
    rows, S, B = 67, sum(sizes), len(sizes)
    logits, masks = _crafted(sizes, rows, 23 + S)
    for use_masks in (True, False):
        x = torch.where(masks, logits, torch.tensor(-1e8)) if use_masks else logits
        want, at = [], 0
        for n in sizes:
            want.append(torch.argmax(x[:, at:at + n], dim=-1))
            at += n
        want = torch.stack(want, dim=-1)
        if use_masks:
            assert (want[7] == 0).all() and (want[8] == torch.tensor(sizes) - 1).all()
        for pad in (0, 5):                                    # contiguous and strided logits / masks
            lg = torch.cat([logits, torch.zeros(rows, pad)], dim=1).to(DEV)[:, :S]
            mk = torch.cat([masks, torch.ones(rows, pad, dtype=torch.bool)], dim=1).to(DEV)[:, :S] if use_masks else None
            out = _Guarded(rows, B, torch.int64)
            ops.play_categorical_head(lg, sizes, None, mk, out.out)
            assert torch.equal(out.check().cpu(), want), (use_masks, pad)


# ----------------------------------------------------------------------------- post-step and fold

def _episode_run(rows, ld, steps, p_done, seed, slots_per_fold, games_limit=10 ** 9, quiet_step=None):
    """`steps` steps of rlg_play_post_step into `steps` slots, folded `slots_per_fold` at a time; cur_r / cur_n against
    the statements of the player's loop after every step.  -> (totals [3] fp64 on the CPU, games, the CPU's evaluation)."""
    from rl_games_amd import ops
    g = _gen(seed)
    blocks = ops.play_post_step_blocks(rows)
    partials = torch.full((steps, blocks, 3), float('nan'), dtype=torch.float64, device=DEV)
    totals, games = ops.play_totals(DEV)
    cur_r, cur_n = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    ref_r, ref_n = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    sum_r, sum_n, count, open_ = 0.0, 0.0, 0, True
    for s in range(steps):
        rewards = torch.randn(rows, ld, generator=g).to(DEV)
        dones = torch.rand(rows, generator=g) < (0.0 if s == quiet_step else p_done)
        dones = dones.to(DEV)
        ops.play_post_step(rewards, dones, cur_r, cur_n, partials[s])
        ref_r += rewards[:, 0]                                # (the player's loop)
        ref_n += 1
        if open_:
            # the host loop: add the step, then stop once games >= games_num; fp32 episode sums, fp64 totals
            sum_r += ref_r[dones].cpu().double().sum().item()
            sum_n += ref_n[dones].cpu().double().sum().item()
            count += int(dones.sum().item())
            open_ = count < games_limit
        ref_r[dones] = 0
        ref_n[dones] = 0
        assert torch.equal(cur_r, ref_r) and torch.equal(cur_n, ref_n), s
    for at in range(0, steps, slots_per_fold):
        ops.play_fold(partials[at:at + slots_per_fold], min(slots_per_fold, steps - at), games_limit, totals)
    return totals.cpu(), int(games.item()), (sum_r, sum_n, count)


@pytest.mark.parametrize('ld', [1, 2])
@pytest.mark.parametrize('rows', [1, 64, 65, 1000])
def test_post_step_and_fold_against_the_host_loop(rows, ld):
    steps = 40
    runs = {k: _episode_run(rows, ld, steps, 0.2, 100 + rows, k, quiet_step=7) for k in (1, 7, 40)}
    totals, games, (sum_r, sum_n, count) = runs[40]
    assert games == count and totals[1].item() == sum_n
    assert abs(totals[0].item() - sum_r) <= 1e-12 * abs(sum_r)
    for k in (1, 7):                                          # however the slots are spread over calls: the same bits
        assert torch.equal(runs[k][0].view(torch.int64), totals.view(torch.int64)) and runs[k][1] == games
    again = _episode_run(rows, ld, steps, 0.2, 100 + rows, 7, quiet_step=7)
    assert torch.equal(again[0].view(torch.int64), runs[7][0].view(torch.int64))


@pytest.mark.parametrize('per_fold', [1, 7, 40])
def test_fold_stops_behind_the_slot_that_reaches_the_limit(per_fold):
    from rl_games_amd import ops
    rows, limit = 65, 100
    totals, games, (sum_r, sum_n, count) = _episode_run(rows, 1, 40, 0.2, 5, per_fold, games_limit=limit)
    # the crossing slot counts whole (13 finished rows a step on average: the limit falls inside a slot), later ones not
    assert limit <= count == games < limit + rows and totals[1].item() == sum_n
    assert abs(totals[0].item() - sum_r) <= 1e-12 * abs(sum_r)
    # a further fold changes nothing
    dev_totals = totals.to(DEV)
    before = dev_totals.clone()
    ops.play_fold(torch.ones(3, ops.play_post_step_blocks(rows), 3, dtype=torch.float64, device=DEV), 3, limit, dev_totals)
    assert torch.equal(dev_totals.view(torch.int64), before.view(torch.int64))
