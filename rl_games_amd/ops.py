"""Thin, typed wrappers over the C ABI (include/rlg_hip.h): one Python function per entry
point, taking torch CUDA tensors, launching on torch's current stream.  No arithmetic
happens here - shapes/dtypes are checked and raw pointers are handed to librlg_hip.so.
"""
import ctypes
import math

import numpy as np
import os

import torch

from . import _lib, range_guard, weight_forms

F32 = torch.float32
F64 = torch.float64
U8 = torch.uint8


def _need(t, dtype, name, contiguous=True):
    if t is None:
        raise ValueError(f'{name} is None')
    _lib.require_gpu(t, name)
    if t.dtype != dtype:
        raise ValueError(f'{name}: expected {dtype}, got {t.dtype}')
    if contiguous and not t.is_contiguous():
        raise ValueError(f'{name}: expected a contiguous tensor, got strides {t.stride()}')
    return t.data_ptr()


def _opt(t, dtype, name):
    return None if t is None else _need(t, dtype, name)


def _stream(t):
    return _lib.stream_handle(t.device)


# ------------------------------------------------------------------ rollout buffer

def rollout_store_step(pairs, num_envs, horizon, step):
    """pairs: list of (src [N, ...] contiguous, dst env-major storage [N, H, ...] contiguous).
    Equivalent to `dst_view[step, :] = src` for every pair (experience.py:433-456)."""
    lib = _lib.load()
    n = len(pairs)
    srcs = (ctypes.c_void_p * n)()
    dsts = (ctypes.c_void_p * n)()
    rows = (ctypes.c_int * n)()
    for k, (src, dst) in enumerate(pairs):
        _lib.require_gpu(src, 'rollout_store_step src')
        if not src.is_contiguous() or not dst.is_contiguous():
            raise ValueError('rollout_store_step needs contiguous src and env-major dst')
        if src.dtype != dst.dtype:
            raise ValueError(f'dtype mismatch {src.dtype} vs {dst.dtype}')
        row_bytes = (src.numel() // num_envs) * src.element_size()
        if src.shape[0] != num_envs or dst.numel() * dst.element_size() != num_envs * horizon * row_bytes:
            raise ValueError(f'shape mismatch: src {tuple(src.shape)} dst {tuple(dst.shape)}')
        srcs[k] = src.data_ptr()
        dsts[k] = dst.data_ptr()
        rows[k] = row_bytes
    _lib.check(lib.rlg_rollout_store_step(n, srcs, dsts, rows, num_envs, horizon, step,
                                          _stream(pairs[0][0])), 'rlg_rollout_store_step')


def post_step_num_blocks(num_envs):
    return _lib.load().rlg_rollout_post_step_num_blocks(int(num_envs))


def rollout_post_step(rewards, dones, time_outs, values, live_rows, rewards_buf, cur_rewards,
                      cur_shaped, cur_lengths, ep_partials, shaper, bootstrap, gamma, horizon, step,
                      num_agents=1):
    """shaper = (shift, scale, min_val, max_val[, log_val])."""
    lib = _lib.load()
    N, V = rewards.shape
    shift, scale, rmin, rmax = shaper[:4]
    clamp = 0 if (rmin == -np.inf and rmax == np.inf) else 1
    if len(shaper) > 4 and shaper[4]:
        clamp |= 2
    kind, to_ptr = 0, None
    if time_outs is not None:
        if time_outs.dtype == F32:
            kind, to_ptr = 2, _need(time_outs, F32, 'time_outs')
        elif time_outs.dtype in (U8, torch.bool):
            kind, to_ptr = 1, (time_outs.view(U8) if time_outs.dtype == torch.bool else time_outs).data_ptr()
            _lib.require_gpu(time_outs, 'time_outs')
        else:
            raise ValueError(f'time_outs dtype {time_outs.dtype} unsupported')
    desc = _lib.PostStepDesc(
        rewards=_need(rewards, F32, 'rewards'), dones=_need(dones, U8, 'dones'), time_outs=to_ptr, time_outs_kind=kind,
        values=_need(values, F32, 'values'), live_rows=_opt(live_rows, F32, 'live_rows'),
        rewards_buf=_need(rewards_buf, F32, 'rewards_buf'), cur_rewards=_need(cur_rewards, F32, 'cur_rewards'),
        cur_shaped=_need(cur_shaped, F32, 'cur_shaped'), cur_lengths=_need(cur_lengths, F32, 'cur_lengths'),
        ep_partials=_need(ep_partials, F64, 'ep_partials'), shift=shift, scale=scale, rmin=max(rmin, -3.0e38),
        rmax=min(rmax, 3.0e38), clamp_rewards=clamp, bootstrap=1 if bootstrap else 0, gamma=gamma, N=N, H=horizon, V=V,
        step=step, num_agents=int(num_agents))
    _lib.check(lib.rlg_rollout_post_step(ctypes.addressof(desc), _stream(rewards)), 'rlg_rollout_post_step')


def episode_meters_update(ep_partials, horizon, num_blocks, value_size, max_size, mean_rewards,
                          mean_shaped, mean_lengths, current_sizes, finished_total):
    lib = _lib.load()
    _lib.check(lib.rlg_episode_meters_update(
        _need(ep_partials, F64, 'ep_partials'), horizon, num_blocks, value_size, max_size,
        _need(mean_rewards, F32, 'mean_rewards'), _need(mean_shaped, F32, 'mean_shaped'),
        _need(mean_lengths, F32, 'mean_lengths'), _need(current_sizes, torch.int32, 'current_sizes'),
        _need(finished_total, torch.int64, 'finished_total'), _stream(ep_partials)),
        'rlg_episode_meters_update')


def rollout_policy_head(heads, logstd, noise, value_stats, eps, actions_out, values_out, storage, horizon,
                        step, env_actions=None, value=None, value_repeat=1):
    """storage: ExperienceBuffer.storage (env-major fields).  value_stats = (mean, var) or None.
    env_actions = (out [N, A], low [A], high [A]): also rescale_actions(low, high, clamp(actions, -1, 1)).
    value: None (column 0 of the heads) or a [N / value_repeat, 1] view with any row stride (a central value network's
    output): row r of the step gets the value of row r // value_repeat."""
    lib = _lib.load()
    N, A = noise.shape
    desc = _lib.PolicyHeadDesc(
        heads=_need(heads, F32, 'heads'), ld=heads.stride(0), logstd=_need(logstd, F32, 'logstd'),
        noise=_need(noise, F32, 'noise'), eps=eps, actions_out=_need(actions_out, F32, 'actions_out'),
        values_out=_need(values_out, F32, 'values_out'), buf_actions=_need(storage['actions'], F32, 'actions'),
        buf_mus=_need(storage['mus'], F32, 'mus'), buf_sigmas=_need(storage['sigmas'], F32, 'sigmas'),
        buf_neglogp=_need(storage['neglogpacs'], F32, 'neglogpacs'), buf_values=_need(storage['values'], F32, 'values'),
        N=N, H=horizon, A=A, step=step)
    if value_stats is not None:
        desc.v_mean, desc.v_var = _need(value_stats[0], F64, 'value mean'), _need(value_stats[1], F64, 'value var')
    if value is None:
        if value_repeat != 1:
            raise ValueError('value_repeat needs a value tensor')
    else:
        desc.value, desc.ld_value = _value_column(value, N, value_repeat)
        desc.value_repeat = int(value_repeat)
    if env_actions is not None:
        desc.env_actions_out = _need(env_actions[0], F32, 'env actions')
        desc.act_low, desc.act_high = _need(env_actions[1], F32, 'actions low'), _need(env_actions[2], F32, 'actions high')
    _lib.check(lib.rlg_rollout_policy_head(ctypes.addressof(desc), _stream(heads)), 'rlg_rollout_policy_head')


CATEGORICAL_MAX_BRANCHES = 16


def _row_view(t, dtype, rows, cols, name):
    """[rows, cols] view with unit column stride and any row stride -> (address, row stride)."""
    _lib.require_gpu(t, name)
    if t.dtype != dtype:
        raise ValueError(f'{name}: expected {dtype}, got {t.dtype}')
    if t.dim() != 2 or tuple(t.shape) != (rows, cols) or (cols > 1 and t.stride(1) != 1) or t.stride(0) < cols:
        raise ValueError(f'{name}: expected a [{rows}, {cols}] view with unit column stride, got {tuple(t.shape)} '
                         f'strides {t.stride()}')
    return t.data_ptr(), t.stride(0)


def _value_column(value, N, value_repeat):
    """(address, row stride) of the value column that serves N rollout rows, value_repeat rows per value row."""
    if int(value_repeat) < 1 or N % int(value_repeat):
        raise ValueError(f'value_repeat {value_repeat} does not divide {N} rows')
    if value.dim() == 1:
        value = value.unsqueeze(1)
    return _row_view(value, F32, N // int(value_repeat), 1, 'value')


def _categorical_rows(logits, branch_sizes, noise, masks):
    """What both categorical heads are told about their rows, checked: (the sizes as a C int array, N, B, logits
    address and row stride, noise address or None, masks address or None and row stride)."""
    sizes = [int(s) for s in branch_sizes]
    N, S, B = logits.shape[0], sum(sizes), len(sizes)
    lg, ld_lg = _row_view(logits, F32, N, S, 'logits')
    if noise is not None:
        _need(noise, F32, 'noise')
        if noise.numel() < N * S:
            raise ValueError(f'noise: {noise.numel()} draws for {N} x {S}')
    mp, ld_m = None, 0
    if masks is not None:
        mp, ld_m = _row_view(masks.view(U8) if masks.dtype == torch.bool else masks, U8, N, S, 'masks')
    return (ctypes.c_int * B)(*sizes), N, B, lg, ld_lg, None if noise is None else noise.data_ptr(), mp, ld_m


def rollout_categorical_head(logits, value, branch_sizes, noise, masks, value_stats, eps, actions_out, values_out,
                             storage, horizon, step, value_repeat=1):
    """Categorical rollout head (csrc/rollout_categorical.hip).  logits [N, sum(sizes)] and value [N, 1] (views of the
    chain's heads, any row stride; value may also be [N]); noise: fp32 Exp(1) draws, >= N * sum(sizes), branch b's block [N, sizes[b]] at
    N * sum(sizes[:b]); masks: bool [N, sum(sizes)] view (the buffer slot of the step) or None; value_stats =
    (mean, var) or None; actions_out int64 [N] / [N, B]; values_out fp32 [N]; storage: ExperienceBuffer.storage
    (env-major 'actions', 'neglogpacs', 'values').  Slot `step` of those fields is written.  value_repeat > 1: value
    has N / value_repeat rows (a central value network's output), row r of the step gets the value of row
    r // value_repeat."""
    lib = _lib.load()
    if noise is None:
        raise ValueError('noise is None')
    arr, N, B, lg, ld_lg, qp, mp, ld_m = _categorical_rows(logits, branch_sizes, noise, masks)
    vp, ld_v = _value_column(value, N, value_repeat)
    if actions_out.numel() != N * B or values_out.numel() != N:
        raise ValueError('actions_out [N, B] / values_out [N] expected')
    fields = ((storage['actions'], torch.int64, N * horizon * B), (storage['neglogpacs'], F32, N * horizon),
              (storage['values'], F32, N * horizon))
    for t, dtype, numel in fields:
        if t.numel() != numel:
            raise ValueError(f'buffer field of {t.numel()} elements, expected {numel}')
    buf_actions, buf_neglogp, buf_values = [_need(t, dtype, 'buffer field') for t, dtype, _ in fields]
    desc = _lib.CategoricalHeadDesc(
        logits=lg, ld_logits=ld_lg, branch_sizes=ctypes.addressof(arr), num_branches=B, exp_noise=qp, masks_or_null=mp,
        ld_masks=ld_m, value=vp, ld_value=ld_v, value_repeat=int(value_repeat), eps=eps,
        actions_out=_need(actions_out, torch.int64, 'actions_out'), values_out=_need(values_out, F32, 'values_out'),
        buf_actions=buf_actions, buf_neglogp=buf_neglogp, buf_values=buf_values, num_envs=N, horizon=horizon, step=step)
    if value_stats is not None:
        desc.v_mean_or_null = _need(value_stats[0], F64, 'value mean')
        desc.v_var_or_null = _need(value_stats[1], F64, 'value var')
    _lib.check(lib.rlg_rollout_categorical_head(ctypes.addressof(desc), _stream(value)), 'rlg_rollout_categorical_head')


def rnn_zero_done_states(states, dones):
    lib = _lib.load()
    L, N, U = states.shape
    _lib.check(lib.rlg_rnn_zero_done_states(_need(states, F32, 'states'), _need(dones, U8, 'dones'),
                                            L, N, U, _stream(states)), 'rlg_rnn_zero_done_states')


# ------------------------------------------------------------------ players (csrc/play.hip)

def play_policy_head(mu, logstd, noise, actions_out, bounds=None):
    """mu: the [rows, A] mean columns of the heads (a view, any row stride); noise [rows, A] or None (deterministic: a =
    mu, logstd is not read); bounds = (low [A], high [A]) or None: clamp + rescale for the env.  actions_out [rows, A]."""
    rows, A = mu.shape
    mp, ld = _row_view(mu, F32, rows, A, 'mu')
    if tuple(actions_out.shape) != (rows, A) or (noise is not None and tuple(noise.shape) != (rows, A)):
        raise ValueError(f'noise / actions_out: [{rows}, {A}] expected')
    lo, hi = (None, None) if bounds is None else (_need(bounds[0], F32, 'actions low'), _need(bounds[1], F32, 'actions high'))
    _lib.check(_lib.load().rlg_play_policy_head(
        mp, ld, 0, _opt(logstd, F32, 'logstd'), _opt(noise, F32, 'noise'), lo, hi,
        _need(actions_out, F32, 'actions_out'), rows, A, _stream(mu)), 'rlg_play_policy_head')


def play_categorical_head(logits, branch_sizes, noise, masks, actions_out):
    """logits [N, sum(sizes)] (a view, any row stride); noise: the Exp(1) draws of rollout_categorical_head or None
    (arg-max); masks: bool / uint8 [N, sum(sizes)] view or None; actions_out int64 [N] / [N, B]."""
    arr, N, B, lg, ld_lg, qp, mp, ld_m = _categorical_rows(logits, branch_sizes, noise, masks)
    if actions_out.numel() != N * B:
        raise ValueError('actions_out [N, B] expected')
    _lib.check(_lib.load().rlg_play_categorical_head(
        lg, ld_lg, arr, B, qp, mp, ld_m, _need(actions_out, torch.int64, 'actions_out'), N, _stream(logits)),
        'rlg_play_categorical_head')


def play_post_step_blocks(rows):
    return _lib.load().rlg_play_post_step_num_blocks(int(rows))


def play_post_step(rewards, dones, cur_rewards, cur_lengths, partials_slot):
    """rewards: fp32 [rows] or column 0 of [rows, V]; dones: bool / uint8 [rows]; partials_slot: fp64 [blocks, 3]."""
    rows = cur_rewards.shape[0]
    if rewards.dim() == 1:
        rewards = rewards.unsqueeze(1)
    rp, ld = _row_view(rewards[:, :1], F32, rows, 1, 'rewards')
    if dones.numel() != rows or cur_lengths.numel() != rows or partials_slot.numel() != 3 * play_post_step_blocks(rows):
        raise ValueError('dones / cur_lengths [rows] and partials_slot [blocks, 3] expected')
    _lib.check(_lib.load().rlg_play_post_step(
        rp, ld, _need(dones.view(U8) if dones.dtype == torch.bool else dones, U8, 'dones'),
        _need(cur_rewards, F32, 'cur_rewards'), _need(cur_lengths, F32, 'cur_lengths'),
        _need(partials_slot, F64, 'partials_slot'), rows, _stream(cur_rewards)), 'rlg_play_post_step')


def play_totals(device):
    """(totals, games): 24 bytes as fp64 [3] - reward sum, length sum - and the same storage's third word as int64."""
    totals = torch.zeros(3, dtype=F64, device=device)
    return totals, totals.view(torch.int64)[2:]


def play_fold(partials, slots, games_limit, totals):
    """partials fp64 [>= slots, blocks, 3]: folds the first `slots` slots into totals while games < games_limit."""
    if partials.dim() != 3 or partials.shape[2] != 3 or partials.shape[0] < slots or totals.numel() != 3:
        raise ValueError('partials [slots, blocks, 3] and totals [3] expected')
    _lib.check(_lib.load().rlg_play_fold(
        _need(partials, F64, 'partials'), int(slots), partials.shape[1], min(int(games_limit), 2 ** 62),
        _need(totals, F64, 'totals'), _stream(partials)), 'rlg_play_fold')


# ------------------------------------------------------------------ running statistics

def column_moments_blocks(rows, cols):
    return _lib.load().rlg_column_moments_num_blocks(int(rows), int(cols))


def column_moments(x, mask=None, partials=None):
    """x [rows, C] fp32 -> partials [blocks, 2C+1] fp64."""
    lib = _lib.load()
    x2 = x.reshape(x.shape[0], -1)
    rows, C = x2.shape
    nb = column_moments_blocks(rows, C)
    if partials is None:
        partials = torch.empty((nb, 2 * C + 1), dtype=F64, device=x.device)
    _lib.check(lib.rlg_column_moments(_need(x2, F32, 'x'), _opt(mask, F32, 'mask'), rows, C,
                                      _need(partials, F64, 'partials'), nb, _stream(x)),
               'rlg_column_moments')
    return partials, nb


def column_moments_segments(x, rows_per_segment, table=None, scratch=None):
    """x [segments * rows_per_segment, C] fp32 contiguous -> table [segments, 2C+1] fp64 =
    {sum[C], sumsq[C], rows} per band of rows (the minibatches of an epoch); two launches.
    Returns (table, scratch) so that callers can keep both between epochs."""
    lib = _lib.load()
    x2 = x.reshape(x.shape[0], -1)
    total, C = x2.shape
    rps = int(rows_per_segment)
    if rps <= 0 or total % rps != 0:
        raise ValueError(f'{total} rows are not a whole number of {rps}-row segments')
    segs = total // rps
    nb = column_moments_blocks(rps, C)
    W = 2 * C + 1
    if table is None or table.numel() != segs * W or table.device != x.device:
        table = torch.empty((segs, W), dtype=F64, device=x.device)
    if scratch is None or scratch.numel() < segs * nb * W or scratch.device != x.device:
        scratch = torch.empty(segs * nb * W, dtype=F64, device=x.device)
    _lib.check(lib.rlg_column_moments_segments(_need(x2, F32, 'x'), rps, C, segs, _need(scratch, F64, 'scratch'),
                                               nb, _need(table, F64, 'table'), _stream(x)),
               'rlg_column_moments_segments')
    return table, scratch


_tickets = {}


def _ticket(device):
    """Zero-initialised arrival counter shared by all rms_update launches of a device (the
    launches are stream-ordered and the kernel resets it)."""
    key = str(device)
    if key not in _tickets:
        _tickets[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _tickets[key]


def rms_update(partials, num_blocks, cols, total_rows, mode, running_mean, running_var, count):
    lib = _lib.load()
    _lib.check(lib.rlg_rms_update(_need(partials, F64, 'partials'), num_blocks, cols, total_rows, mode,
                                  _need(running_mean, F64, 'running_mean'),
                                  _need(running_var, F64, 'running_var'),
                                  _need(count, torch.int64, 'count'),
                                  _ticket(partials.device).data_ptr(), _stream(partials)),
               'rlg_rms_update')


def rms_apply(x, running_mean, running_var, eps, mode=0, out=None):
    lib = _lib.load()
    x2 = x.reshape(x.shape[0], -1) if x.dim() > 1 else x.reshape(-1, 1)
    rows, C = x2.shape
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    _lib.check(lib.rlg_rms_apply(_need(x2, F32, 'x'), _need(out, F32, 'out'), rows, C,
                                 _need(running_mean, F64, 'running_mean'),
                                 _need(running_var, F64, 'running_var'), float(np.float32(eps)), mode,
                                 _stream(x)), 'rlg_rms_apply')
    return out


class StatsSyncKernels:
    """Device side of distributed.StatsSync: the normalisers' state tensors as the pointer tables of
    rlg_stats_sync_pack / rlg_stats_sync_apply (include/rlg_hip.h)."""

    PACK_DELTAS, PACK_SEED, PACK_STATE = 0, 1, 2
    APPLY_MERGE, APPLY_STATE = 0, 2

    MAX_SEGMENTS = 8      # kStatsMaxSegments of csrc/running_stats.hip

    def __init__(self, modules):
        import ctypes
        n = len(modules)
        if n > self.MAX_SEGMENTS:
            raise ValueError(f'StatsSyncKernels: {n} normalisers, one launch carries at most {self.MAX_SEGMENTS} '
                             '(build one StatsSync per group of normalisers)')
        self.device = modules[0].running_mean.device
        self._keep = [(m.running_mean, m.running_var, m.count) for m in modules]
        self.dims = [int(m.running_mean.numel()) for m in modules]
        self._means = (ctypes.c_void_p * n)(*[_need(m.running_mean, F64, 'running_mean') for m in modules])
        self._vars = (ctypes.c_void_p * n)(*[_need(m.running_var, F64, 'running_var') for m in modules])
        self._counts = (ctypes.c_void_p * n)(*[_need(m.count, torch.int64, 'count') for m in modules])
        self._dims = (ctypes.c_int * n)(*self.dims)
        self._n = n
        self._ctypes = ctypes
        self.flat_size = int(_lib.load().rlg_stats_sync_flat_size(n, ctypes.cast(self._dims, ctypes.c_void_p)))
        self._ptrs = [(m.running_mean.data_ptr(), m.running_var.data_ptr(), m.count.data_ptr()) for m in modules]

    def bound_to(self, modules):
        """True while the pointer tables still address these modules' state tensors."""
        return len(modules) == self._n and all(
            (m.running_mean.data_ptr(), m.running_var.data_ptr(), m.count.data_ptr()) == p
            for m, p in zip(modules, self._ptrs))

    def _tables(self, has_snapshot):
        c = self._ctypes
        flags = (c.c_int * self._n)(*[int(bool(h)) for h in has_snapshot])
        return (self._n, c.cast(self._means, c.c_void_p), c.cast(self._vars, c.c_void_p),
                c.cast(self._counts, c.c_void_p), c.cast(self._dims, c.c_void_p), c.cast(flags, c.c_void_p)), flags

    def pack(self, has_snapshot, snapshot, out, mode):
        args, keep = self._tables(has_snapshot)
        _lib.check(_lib.load().rlg_stats_sync_pack(*args, _need(snapshot, F64, 'snapshot'),
                                                   _need(out, F64, 'out'), mode, _stream(out)),
                   'rlg_stats_sync_pack')

    def apply(self, has_snapshot, snapshot, reduced, mode):
        args, keep = self._tables(has_snapshot)
        _lib.check(_lib.load().rlg_stats_sync_apply(*args, _need(snapshot, F64, 'snapshot'),
                                                    _need(reduced, F64, 'reduced'), mode, _stream(reduced)),
                   'rlg_stats_sync_apply')


PREP_NORM_VALUE = 1
PREP_NORM_ADV = 2
PREP_FREEZE_CRITIC = 4
PREP_EMA_ADV = 8


def prepare_stats_buffer(device):
    n = _lib.load().rlg_prepare_stats_bytes()
    return torch.zeros(n // 4, dtype=F32, device=device)


def prepare_finalize(gae_partials, batch, flags, value_stats, eps, ema, stats_out):
    """value_stats = (running_mean, running_var, count) or None; ema = dict(mean, sqrs, step,
    decay, max, eps) or None."""
    lib = _lib.load()
    rm = rv = cnt = None
    if value_stats is not None:
        rm, rv, cnt = value_stats
    em = es = est = None
    decay = factor = 0.0
    emax, eeps = 1e5, 0.0
    if ema is not None:
        em, es, est = ema['mean'], ema['sqrs'], ema['step']
        decay = float(np.float32(ema['decay']))
        factor = float(np.float32(1 - ema['decay']))
        emax, eeps = float(ema['max']), float(ema['eps'])
    _lib.check(lib.rlg_prepare_finalize(
        _need(gae_partials, F64, 'gae_partials'), gae_partials.shape[0], gae_partials.shape[1], batch, flags,
        _opt(rm, F64, 'value running_mean'), _opt(rv, F64, 'value running_var'),
        _opt(cnt, torch.int64, 'value count'), float(np.float32(eps)), _opt(em, F32, 'ema mean'),
        _opt(es, F32, 'ema sqrs'), _opt(est, torch.int32, 'ema step'), decay, factor,
        float(np.float32(emax)), float(np.float32(eeps)), _need(stats_out, F32, 'stats_out'),
        _stream(gae_partials)), 'rlg_prepare_finalize')


def triple_moments(advantages, values, returns, mask=None):
    """[blocks, 6 or 7] fp64 partial sums in the GAE-partials format."""
    lib = _lib.load()
    B = advantages.numel()
    nb = lib.rlg_triple_moments_num_blocks(B)
    part = torch.empty((nb, 7 if mask is not None else 6), dtype=F64, device=advantages.device)
    _lib.check(lib.rlg_triple_moments(_need(advantages, F32, 'advantages'), _need(values, F32, 'values'),
                                      _need(returns, F32, 'returns'), _opt(mask, F32, 'mask'), B,
                                      part.data_ptr(), nb, _stream(advantages)), 'rlg_triple_moments')
    return part


def prepare_apply(values, returns, advantages, flags, stats, out=None):
    """out = (values_out, returns_out, advantages_out) or None for in place."""
    lib = _lib.load()
    B = advantages.numel()
    vo, ro, ao = (values, returns, advantages) if out is None else out
    _lib.check(lib.rlg_prepare_apply(_need(values, F32, 'values'), _need(returns, F32, 'returns'),
                                     _need(advantages, F32, 'advantages'), _need(vo, F32, 'values_out'),
                                     _need(ro, F32, 'returns_out'), _need(ao, F32, 'advantages_out'),
                                     B, flags, _need(stats, F32, 'stats'), _stream(values)),
               'rlg_prepare_apply')


# ------------------------------------------------------------------ PPO loss

BOUND_KINDS = {None: 0, 'none': 0, 'bound': 1, 'regularisation': 2}


def sequence_mask(rnn_masks):
    """(mask [rows] fp32, sum(mask) [1]) - the `mask` / `mask_sum` arguments of the loss launches - of a recurrent
    minibatch's `rnn_masks`; (None, None) without one."""
    if rnn_masks is None:
        return None, None
    mask = rnn_masks.reshape(-1).float().contiguous()
    return mask, mask.sum().reshape(1)


def ppo_loss_blocks(minibatch):
    return _lib.load().rlg_ppo_loss_num_blocks(int(minibatch))


def ppo_loss_partials_per_block(actions):
    return _lib.load().rlg_ppo_loss_partials_per_block(int(actions))


def _rows_view(t, name):
    """(pointer, row stride) of a [rows, cols] / [rows] fp32 view whose inner stride is 1."""
    _lib.require_gpu(t, name)
    if t.dtype != F32:
        raise ValueError(f'{name}: expected fp32')
    if t.dim() == 2:
        if t.shape[1] != 1 and t.stride(1) != 1:
            raise ValueError(f'{name}: inner stride must be 1, got {t.stride()}')
        return t.data_ptr(), t.stride(0)
    if t.dim() == 1:
        return t.data_ptr(), t.stride(0)
    raise ValueError(f'{name}: expected 1-D or 2-D')


SURROGATE_CLIP, SURROGATE_SMOOTH, SURROGATE_NONE = 0, 1, 2


def _surrogate_kind(smooth):
    """The `smooth` argument of the loss launches: False / True (`use_smooth_clamp`) or one of SURROGATE_* -
    SURROGATE_NONE is `ppo: False`, the plain A2C actor loss neglogp * advantage (common_losses.py:59, 80)."""
    k = int(smooth)
    if k not in (SURROGATE_CLIP, SURROGATE_SMOOTH, SURROGATE_NONE):
        raise ValueError(f'surrogate kind {smooth!r}')
    return k


def ppo_loss_fused(mu, logstd, values, actions, old_neglogp, advantages, old_values, returns,
                   old_mu, old_sigma, d_mu, d_values, partials, e_clip, critic_coef, bounds_coef,
                   clip_value=True, smooth=False, bound_kind=1, write_back=True, mask=None,
                   mask_sum=None):
    """mu/d_mu [mb, A] and values/d_values [mb] may be strided row views (fused head buffer)."""
    lib = _lib.load()
    desc = ppo_loss_desc(mu, logstd, values, actions, old_neglogp, advantages, old_values, returns, old_mu, old_sigma,
                         d_mu, d_values, partials, e_clip, critic_coef, bounds_coef, clip_value, smooth, bound_kind,
                         write_back, mask, mask_sum)
    _lib.check(lib.rlg_ppo_loss_fused(ctypes.addressof(desc), _stream(mu)), 'rlg_ppo_loss_fused')


def ppo_loss_desc(mu, logstd, values, actions, old_neglogp, advantages, old_values, returns,
                  old_mu, old_sigma, d_mu, d_values, partials, e_clip, critic_coef, bounds_coef,
                  clip_value=True, smooth=False, bound_kind=1, write_back=True, mask=None, mask_sum=None):
    """The arguments of the loss as an rlg_ppo_loss_desc: what ppo_loss_fused launches, and for
    MlpChain.backward(ppo_loss=...) the loss the backward launch evaluates for each row tile in front of its own
    work.  There d_mu / d_values must be views of the d_heads tensor that backward then reads, and partials needs
    MlpChain.num_blocks(rows, 1) rows.  The descriptor keeps no tensor alive - the caller does (they are the step's
    static buffers)."""
    mb, A = mu.shape
    mu_p, ld_mu = _rows_view(mu, 'mu')
    val_p, ld_val = _rows_view(values, 'values')
    dmu_p, ld_dmu = _rows_view(d_mu, 'd_mu')
    dval_p, ld_dval = _rows_view(d_values, 'd_values')
    return _lib.PpoLossDesc(
        mu_p, _need(logstd, F32, 'logstd'), val_p, _need(actions, F32, 'actions'),
        _need(old_neglogp, F32, 'old_neglogp'), _need(advantages, F32, 'advantages'),
        _need(old_values, F32, 'old_values'), _need(returns, F32, 'returns'), _need(old_mu, F32, 'old_mu'),
        _need(old_sigma, F32, 'old_sigma'), _opt(mask, F32, 'mask'), _opt(mask_sum, F32, 'mask_sum'), dmu_p, dval_p,
        _need(partials, F64, 'partials'), mb, A, ld_mu, ld_val, ld_dmu, ld_dval,
        float(np.float32(e_clip)), float(np.float32(critic_coef)), float(np.float32(bounds_coef)),
        1 if clip_value else 0, _surrogate_kind(smooth), bound_kind, 1 if write_back else 0)


def value_loss(values, old_values, returns, d_values, partials, e_clip, clip_value=True, mask=None, mask_sum=None):
    """Central-value critic loss + its gradient; partials [ceil(mb/256), 7] for ppo_loss_finalize."""
    lib = _lib.load()
    mb = values.shape[0]
    _lib.check(lib.rlg_value_loss(_need(values, F32, 'values'), _need(old_values, F32, 'old_values'),
                                  _need(returns, F32, 'returns'), _opt(mask, F32, 'mask'),
                                  _opt(mask_sum, F32, 'mask_sum'), _need(d_values, F32, 'd_values'),
                                  _need(partials, F64, 'partials'), mb, float(np.float32(e_clip)),
                                  1 if clip_value else 0, _stream(values)), 'rlg_value_loss')


def ppo_loss_discrete_blocks(minibatch):
    return _lib.load().rlg_ppo_loss_discrete_num_blocks(int(minibatch))


def ppo_loss_discrete(logits, values, actions, old_neglogp, advantages, old_values, returns, d_logits,
                      d_values, partials, e_clip, critic_coef, entropy_coef, clip_value=True,
                      smooth=False, mask=None, mask_sum=None, branch_sizes=None, action_masks=None,
                      new_neglogp=None):
    """Categorical PPO loss + gradients.  branch_sizes: widths of the multi-discrete heads
    (default: one head of logits.shape[1]); actions [mb] or [mb, branches] int64; action_masks
    [mb, n] bool/uint8 or None; new_neglogp: fp32 [mb] that receives each row's neglogp, or None."""
    lib = _lib.load()
    mb, n = logits.shape
    _lib.require_gpu(logits, 'logits')
    if logits.dtype != F32 or logits.stride(1) != 1:
        raise ValueError('logits: fp32 with unit inner stride expected')
    sizes = [n] if branch_sizes is None else [int(s) for s in branch_sizes]
    if sum(sizes) != n:
        raise ValueError(f'branch sizes {sizes} do not add up to {n} logits')
    if actions.numel() != mb * len(sizes):
        raise ValueError(f'actions must hold {len(sizes)} indices per row')
    am = None
    if action_masks is not None:
        if action_masks.dtype == torch.bool:
            action_masks = action_masks.view(torch.uint8)
        if tuple(action_masks.shape) != (mb, n):
            raise ValueError('action_masks must be [minibatch, sum(branch sizes)]')
        am = _need(action_masks, torch.uint8, 'action_masks')
    # values / d_values / d_logits may be columns of wider rows (the fused chain's [value | logits] head matrix)
    for name, t, shape in (('values', values, (mb,)), ('d_values', d_values, (mb,)), ('d_logits', d_logits, (mb, n))):
        _lib.require_gpu(t, name)
        if t.dtype != F32 or tuple(t.shape) != shape or (t.dim() == 2 and t.stride(1) != 1):
            raise ValueError(f'{name}: fp32 {shape} with unit inner stride expected')
    arr = (ctypes.c_int * len(sizes))(*sizes)
    if new_neglogp is not None and tuple(new_neglogp.shape) != (mb,):
        raise ValueError('new_neglogp must be [minibatch]')
    desc = _lib.DiscreteLossDesc(
        logits=logits.data_ptr(), ld_logits=logits.stride(0), values=values.data_ptr(),
        ld_values=max(values.stride(0), 1), actions=_need(actions, torch.int64, 'actions'), action_masks_or_null=am,
        branch_sizes=ctypes.addressof(arr), num_branches=len(sizes), old_neglogp=_need(old_neglogp, F32, 'old_neglogp'),
        advantages=_need(advantages, F32, 'advantages'), old_values=_need(old_values, F32, 'old_values'),
        returns=_need(returns, F32, 'returns'), mask_or_null=_opt(mask, F32, 'mask'),
        mask_sum_or_null=_opt(mask_sum, F32, 'mask_sum'), d_logits=d_logits.data_ptr(), ld_d_logits=d_logits.stride(0),
        d_values=d_values.data_ptr(), ld_d_values=max(d_values.stride(0), 1), partials=_need(partials, F64, 'partials'),
        minibatch=mb, e_clip=e_clip, critic_coef=critic_coef, entropy_coef=entropy_coef,
        clip_value=1 if clip_value else 0, use_smooth_clamp=_surrogate_kind(smooth),
        new_neglogp_or_null=_opt(new_neglogp, F32, 'new_neglogp'))
    _lib.check(lib.rlg_ppo_loss_discrete_nlp(ctypes.addressof(desc), _stream(logits)), 'rlg_ppo_loss_discrete_nlp')


def ppo_diag_stats():
    """Doubles per row of the diagnostics table (rlg_ppo_diag)."""
    return _lib.load().rlg_ppo_diag_stats()


def ppo_diag_blocks(minibatch):
    return _lib.load().rlg_ppo_diag_num_blocks(int(minibatch))


def ppo_diag_log_bounds(e_clip):
    """fp32(log(1 - e)), fp32(log(1 + e)): the clip-fraction thresholds of torch_ext.policy_clip_fraction."""
    return float(np.float32(math.log(1.0 - e_clip))), float(np.float32(math.log(1.0 + e_clip)))


def ppo_diag(out, old_neglogp, e_clip, partials, ticket, mask=None, new_neglogp=None, mu=None, logstd=None,
             actions=None, neglogp_out=None):
    """Clip columns (rows, sum of the mask, masked clipped count) of one minibatch's diagnostics row `out` (fp64
    [ppo_diag_stats()]; columns 0..2 written, not accumulated; include/rlg_hip.h).  The new neglogp is `new_neglogp`
    [mb], or - None - recomputed from mu [mb, A] (row stride free), logstd [A] and actions [mb, A] with the continuous
    loss's arithmetic.  partials: fp64, >= ppo_diag_blocks(mb) * 3; ticket: int32 [1], zero, left at zero."""
    lib = _lib.load()
    mb = old_neglogp.numel()
    for name, t in (('mask', mask), ('new_neglogp', new_neglogp), ('neglogp_out', neglogp_out)):
        if t is not None and t.numel() != mb:
            raise ValueError(f'{name}: {mb} elements expected, got {t.numel()}')
    if out.numel() != lib.rlg_ppo_diag_stats() or partials.numel() < ppo_diag_blocks(mb) * 3:
        raise ValueError('ppo_diag: out / partials too small')
    mu_p = ls_p = act_p = None
    ld_mu = ld_act = A = 0
    if new_neglogp is None:
        if mu is None or logstd is None or actions is None:
            raise ValueError('ppo_diag: mu, logstd and actions are needed to recompute the neglogp')
        mu_p, ld_mu = _rows_view(mu, 'mu')
        act_p, ld_act = _rows_view(actions, 'actions')
        A = mu.shape[1]
        if tuple(actions.shape) != (mb, A) or logstd.numel() != A or tuple(mu.shape) != (mb, A):
            raise ValueError('ppo_diag: mu / actions [mb, A] and logstd [A] expected')
        ls_p = _need(logstd, F32, 'logstd')
    lo, hi = ppo_diag_log_bounds(e_clip)
    _lib.check(lib.rlg_ppo_diag(
        mu_p, ld_mu, ls_p, act_p, ld_act, _opt(new_neglogp, F32, 'new_neglogp'), _need(old_neglogp, F32, 'old_neglogp'),
        _opt(mask, F32, 'mask'), mb, A, lo, hi, _need(partials, F64, 'partials'), _need(ticket, torch.int32, 'ticket'),
        _need(out, F64, 'out'), _opt(neglogp_out, F32, 'neglogp_out'), _stream(old_neglogp)), 'rlg_ppo_diag')


def ppo_diag_moments_blocks(rows, cols=1):
    return _lib.load().rlg_ppo_diag_moments_num_blocks(int(rows), int(cols))


def ppo_diag_moments(table, values, returns, slices, rows, partials, tickets, mask=None):
    """Moment columns (3..9) of the diagnostics rows table[:slices] (fp64 [>= slices, ppo_diag_stats()], row-contiguous)
    for `slices` consecutive minibatch slices of `rows` rows: values / returns [slices * rows, cols] (or flat), mask
    [slices * rows] or None.  partials: fp64 >= slices * ppo_diag_moments_blocks(rows, cols) * 9; tickets: int32 [>= slices],
    zero, left at zero."""
    lib = _lib.load()
    n = int(slices) * int(rows)
    if values.numel() % n or values.numel() != returns.numel() or values.numel() < n:
        raise ValueError('ppo_diag_moments: values / returns must hold slices * rows rows of equal width')
    cols = values.numel() // n
    k = lib.rlg_ppo_diag_stats()
    if table.dim() != 2 or table.shape[0] < slices or table.shape[1] != k or table.stride(1) != 1:
        raise ValueError('ppo_diag_moments: table [>= slices, stats] expected')
    if mask is not None and mask.numel() != n:
        raise ValueError(f'ppo_diag_moments: mask of {n} rows expected')
    if partials.numel() < slices * ppo_diag_moments_blocks(rows, cols) * 9 or tickets.numel() < slices:
        raise ValueError('ppo_diag_moments: partials / tickets too small')
    _lib.require_gpu(table, 'table')
    _lib.check(lib.rlg_ppo_diag_moments(
        _need(values, F32, 'values'), _need(returns, F32, 'returns'), _opt(mask, F32, 'mask'), int(slices), int(rows),
        cols, _need(partials, F64, 'partials'), _need(tickets, torch.int32, 'tickets'), table.data_ptr(),
        table.stride(0), _stream(values)), 'rlg_ppo_diag_moments')


def ppo_loss_finalize(partials, num_blocks, actions_num, minibatch, masked, critic_coef,
                      entropy_coef, bounds_coef, scalars, d_logstd, kl_slot=None, d_mu_bias=None,
                      d_value_bias=None):
    ppo_loss_finalize_from(loss_finalize_desc(partials, num_blocks, actions_num, minibatch, masked, critic_coef,
                                              entropy_coef, bounds_coef, scalars, d_logstd, kl_slot, d_mu_bias,
                                              d_value_bias), partials.device)


def loss_finalize_desc(partials, num_blocks, actions_num, minibatch, masked, critic_coef, entropy_coef,
                       bounds_coef, scalars, d_logstd, kl_slot=None, d_mu_bias=None, d_value_bias=None):
    """The arguments of ppo_loss_finalize as an rlg_loss_finalize_desc: MlpDwPlan.launch(loss_finalize=...)
    folds the loss partials in its finalise launch; ppo_loss_finalize_from(desc) is the stand-alone launch."""
    return _lib.LossFinalizeDesc(
        _need(partials, F64, 'partials'), int(num_blocks), int(actions_num), int(minibatch), 1 if masked else 0,
        float(np.float32(critic_coef)), float(np.float32(entropy_coef)), float(np.float32(bounds_coef)),
        _need(scalars, F32, 'scalars'), _need(d_logstd, F32, 'd_logstd'), _opt(kl_slot, F32, 'kl_slot'),
        _opt(d_mu_bias, F32, 'd_mu_bias'), _opt(d_value_bias, F32, 'd_value_bias'))


def ppo_loss_finalize_from(desc, device):
    _lib.check(_lib.load().rlg_ppo_loss_finalize(ctypes.addressof(desc), _lib.stream_handle(device)),
               'rlg_ppo_loss_finalize')


# ------------------------------------------------------------------ manual MLP backward

ACT_KINDS = {'None': 0, None: 0, 'elu': 1, 'relu': 2, 'tanh': 3}


def act_bwd_blocks(rows, cols):
    return _lib.load().rlg_act_bwd_num_blocks(int(rows), int(cols))


def act_bwd_colsum(d_out, pre_act, d_pre, act_kind, partials, num_blocks):
    """d_pre = d_out * act'(pre_act) (d_pre may be d_out); partials[blocks, C] column sums."""
    lib = _lib.load()
    rows, C = d_out.shape
    _lib.check(lib.rlg_act_bwd_colsum(_need(d_out, F32, 'd_out'), _opt(pre_act, F32, 'pre_act'),
                                      _need(d_pre, F32, 'd_pre'), rows, C, d_out.stride(0), act_kind,
                                      _need(partials, F64, 'partials'), num_blocks, _stream(d_out)),
               'rlg_act_bwd_colsum')


def colsum_finalize(partials, num_blocks, cols, out, accumulate=False):
    lib = _lib.load()
    _lib.check(lib.rlg_colsum_finalize(_need(partials, F64, 'partials'), num_blocks, cols,
                                       _need(out, F32, 'out'), 1 if accumulate else 0,
                                       _stream(partials)), 'rlg_colsum_finalize')


# ------------------------------------------------------------------ optimiser

def grad_norm_blocks(n):
    return _lib.load().rlg_grad_norm_num_blocks(int(n))


def grad_sumsq(grads, grad_scale, partials, step_counter=None):
    """Also advances the device-resident Adam step counter when given."""
    lib = _lib.load()
    _lib.check(lib.rlg_grad_sumsq(_need(grads, F32, 'grads'), grads.numel(),
                                  float(np.float32(grad_scale)), _need(partials, F64, 'partials'),
                                  partials.numel(), _opt(step_counter, torch.int64, 'step_counter'),
                                  _stream(grads)), 'rlg_grad_sumsq')


def adam_step(params, grads, exp_avg, exp_avg_sq, norm_partials, grad_scale, max_norm, lr_slots,
              step_counter, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, schedule_kind=0,
              kl=None, kl_scale=1.0, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2,
              lr_multiplier=1.5, stats_out=None, skip_flag=None, pack=None):
    """skip_flag: device address (int) of the in-graph all-reduce's error word, or None.
    pack = MlpChain.adam_pack_target() (n, weights, in, out, planes address): the launch also leaves the chain's
    weight planes for the new weights (rlg_adam_step_pack, csrc/mlp_chain_bx.hip)."""
    _adam_launch(None, params, grads, exp_avg, exp_avg_sq, norm_partials, grad_scale, max_norm, lr_slots, step_counter,
                 betas, eps, weight_decay, schedule_kind, kl, kl_scale, kl_threshold, min_lr, max_lr, lr_multiplier,
                 stats_out, skip_flag, pack)


def adam_step_guarded(guard, params, grads, exp_avg, exp_avg_sq, norm_partials, grad_scale, max_norm, lr_slots,
                      step_counter, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, schedule_kind=0,
                      kl=None, kl_scale=1.0, kl_threshold=0.008, min_lr=1e-6, max_lr=1e-2,
                      lr_multiplier=1.5, stats_out=None, skip_flag=None, pack=None):
    """adam_step under the range-guard record `guard` (guard_record()): the launch is skipped as under skip_flag when the
    record is set or the total gradient norm is not finite, and a clear record then becomes (GUARD_TAG_ADAM, step) -
    rlg_adam_step_guarded / rlg_adam_pack_guarded."""
    if guard is None:
        raise ValueError('adam_step_guarded needs a guard record (ops.guard_record)')
    _adam_launch(guard, params, grads, exp_avg, exp_avg_sq, norm_partials, grad_scale, max_norm, lr_slots, step_counter,
                 betas, eps, weight_decay, schedule_kind, kl, kl_scale, kl_threshold, min_lr, max_lr, lr_multiplier,
                 stats_out, skip_flag, pack)


def _adam_launch(guard, params, grads, exp_avg, exp_avg_sq, norm_partials, grad_scale, max_norm, lr_slots, step_counter,
                 betas, eps, weight_decay, schedule_kind, kl, kl_scale, kl_threshold, min_lr, max_lr, lr_multiplier,
                 stats_out, skip_flag, pack):
    lib = _lib.load()
    desc = _lib.AdamDesc(
        _need(params, F32, 'params'), _need(grads, F32, 'grads'), _need(exp_avg, F32, 'exp_avg'),
        _need(exp_avg_sq, F32, 'exp_avg_sq'), params.numel(), _opt(norm_partials, F64, 'norm_partials'),
        0 if norm_partials is None else norm_partials.numel(), float(np.float32(grad_scale)),
        float(np.float32(max_norm)), _need(lr_slots, F64, 'lr_slots'),
        _need(step_counter, torch.int64, 'step_counter'),
        float(betas[0]), float(betas[1]), float(eps), float(weight_decay), schedule_kind,
        _opt(kl, F32, 'kl'), float(np.float32(kl_scale)), float(kl_threshold), float(min_lr),
        float(max_lr), float(lr_multiplier), _opt(stats_out, F32, 'stats_out'), skip_flag)
    args = (ctypes.addressof(desc),) if guard is None else (ctypes.addressof(desc), _guard_ptr(guard))
    names = ('rlg_adam_step', 'rlg_adam_step_pack') if guard is None else ('rlg_adam_step_guarded', 'rlg_adam_pack_guarded')
    if pack is not None:
        n, w, ins, outs, planes = pack
        _lib.check(getattr(lib, names[1])(*args, n, w, ins, outs, planes, _stream(params)), names[1])
    else:
        _lib.check(getattr(lib, names[0])(*args, _stream(params)), names[0])


# ------------------------------------------------------------------ range guard of the split-fp16 products

GUARD_TAG_ADAM = range_guard.TAG_ADAM            # RLG_GUARD_TAG_ADAM (include/rlg_hip.h)
GUARD_MAX_ARRAYS = 8


def guard_record(device):
    """A clear range-guard record: 4 int32 words - [0] tag (0 = clear), [1] index, [2:4] the scan's own."""
    return torch.zeros(4, dtype=torch.int32, device=device)


def _guard_ptr(record):
    _lib.require_gpu(record, 'guard record')
    if record.dtype != torch.int32 or record.numel() != 4 or not record.is_contiguous():
        raise ValueError('guard record: 4 contiguous int32 words expected (ops.guard_record)')
    return record.data_ptr()


def range_scan(arrays, record):
    """arrays: up to 8 (fp32 tensor, tag != 0) pairs, contiguous, any 4-byte alignment.  One launch; on a non-finite value
    record[0:2] = (tag of the first array in this order that holds one, smallest offending flat index in it) unless
    the record is already set (csrc/range_guard.hip).  No host read here: read_guard().
    Captured into a graph, the launch keeps the nonce of its capture: replayed over a record that an EARLIER REPLAY OF
    ITSELF set, it takes that record for its own and keeps the better of the two hits instead of leaving it.  Read and
    clear the record between replays (records set by other launches - other scans, optimiser steps - are safe)."""
    n = len(arrays)
    if n > GUARD_MAX_ARRAYS:
        raise ValueError(f'range_scan: {n} arrays, one launch takes at most {GUARD_MAX_ARRAYS}')
    P = ctypes.c_void_p * max(n, 1)
    ptrs = P(*[_need(t, F32, 'scanned array') for t, _ in arrays])
    counts = (ctypes.c_longlong * max(n, 1))(*[t.numel() for t, _ in arrays])
    tags = (ctypes.c_int * max(n, 1))(*[int(tag) for _, tag in arrays])
    _lib.check(_lib.load().rlg_range_scan(n, ptrs, counts, tags, _guard_ptr(record), _lib.stream_handle(record.device)),
               'rlg_range_scan')


def read_guard(record):
    """(tag, index) of the record - ONE device-to-host copy; tag 0: clear."""
    w = record[:2].tolist()
    return int(w[0]) & 0xffffffff, int(w[1]) & 0xffffffff


# ------------------------------------------------------------------ MLP forward / dX (MFMA, fused epilogues)

def mlp_rowgemm_supported(reduction_dim, leading_dim):
    return bool(_lib.load().rlg_mlp_rowgemm_supported(int(reduction_dim), int(leading_dim)))


def mlp_linear_act_forward(x, w, bias, out, pre_act=None, act_kind=0):
    """out = act(x @ w.T + bias); pre_act (optional) receives x @ w.T + bias.  csrc/mlp_rowgemm.hip."""
    lib = _lib.load()
    rows, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or out.shape != (rows, N) or x.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError('mlp_linear_act_forward: shape mismatch')
    if pre_act is not None and (pre_act.shape != out.shape or pre_act.stride() != out.stride()):
        raise ValueError('pre_act must have the layout of out')
    _lib.require_gpu(x, 'x')
    _lib.check(lib.rlg_mlp_linear_act_forward(
        x.data_ptr(), x.stride(0), _need(w, F32, 'w'), _opt(bias, F32, 'bias'),
        None if pre_act is None else pre_act.data_ptr(), out.data_ptr(), out.stride(0), rows, N, K,
        act_kind, _stream(x)), 'rlg_mlp_linear_act_forward')


def mlp_linear_act_backward(dz, w, z_prev, dz_prev, act_kind=0):
    """dz_prev = (dz @ w) * act'(z_prev)  (z_prev None: plain dz @ w).  csrc/mlp_rowgemm.hip."""
    lib = _lib.load()
    rows, No = dz.shape
    Mi = w.shape[1]
    if w.shape[0] != No or dz_prev.shape != (rows, Mi) or dz.stride(1) != 1 or dz_prev.stride(1) != 1:
        raise ValueError('mlp_linear_act_backward: shape mismatch')
    if z_prev is not None and (z_prev.shape != dz_prev.shape or z_prev.stride() != dz_prev.stride()):
        raise ValueError('z_prev must have the layout of dz_prev')
    _lib.require_gpu(dz, 'dz')
    _lib.check(lib.rlg_mlp_linear_act_backward(
        dz.data_ptr(), dz.stride(0), _need(w, F32, 'w'), None if z_prev is None else z_prev.data_ptr(),
        dz_prev.data_ptr(), dz_prev.stride(0), rows, No, Mi, act_kind, _stream(dz)),
        'rlg_mlp_linear_act_backward')


NARROW_MAX = 8


def narrow_dx(dz, w, dx):
    """dx [rows, in] = dz [rows, out] @ w [out, in] for out <= 8 (csrc/mlp_narrow.hip)."""
    rows, No = dz.shape
    if w.shape[0] != No or dx.shape != (rows, w.shape[1]) or dz.stride(1) != 1 or dx.stride(1) != 1:
        raise ValueError('narrow_dx: shape mismatch')
    _lib.require_gpu(dz, 'dz')
    _lib.check(_lib.load().rlg_narrow_dx(dz.data_ptr(), dz.stride(0), _need(w, F32, 'w'), dx.data_ptr(), dx.stride(0),
                                         rows, No, w.shape[1], _stream(dz)), 'rlg_narrow_dx')


_narrow_scratch = {}


def narrow_dw(dz, x, grad):
    """grad [out, in] = dz[rows, out].T @ x[rows, in] for in <= 8, out <= 256 (csrc/mlp_narrow.hip)."""
    rows, No = dz.shape
    Mi = x.shape[1]
    if x.shape[0] != rows or tuple(grad.shape) != (No, Mi) or dz.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError('narrow_dw: shape mismatch')
    _lib.require_gpu(dz, 'dz')
    lib = _lib.load()
    need = lib.rlg_narrow_dw_blocks(rows) * No * Mi
    key = (str(dz.device), need)
    if key not in _narrow_scratch:          # (fixed address per shape: the launches are replayed from HIP graphs)
        _narrow_scratch[key] = torch.empty(need, dtype=F64, device=dz.device)
    _lib.check(lib.rlg_narrow_dw(dz.data_ptr(), dz.stride(0), x.data_ptr(), x.stride(0), _need(grad, F32, 'grad'),
                                 _narrow_scratch[key].data_ptr(), rows, No, Mi, _stream(dz)), 'rlg_narrow_dw')


# ------------------------------------------------------------------ fused MLP chain (MFMA, LDS-resident)

chain_timers = None     # bench.py: {'fwd': [...], 'bwd': [...]} of gae.HipEventPair, one per eager chain launch


# fixed operand scales of the split-fp16 form (csrc/bx_form.hpp kBxScaleH / kBxScaleObsNorm)
SPLIT_SCALE_HIDDEN = 16.0
SPLIT_SCALE_OBS_NORM = 4096.0


def chain_split_form():
    """(plane products per fp32 product, plane type) of the split-product chain kernels: (3, 'fp16')."""
    return int(_lib.load().rlg_mlp_chain_split_products()), 'fp16'


def _chain_call(kind, entry, *descs, rows, stream, groups=0):
    """Calls a launching chain entry with `descs` and the launch descriptor of (rows, groups).  With chain_timers a dict,
    outside stream capture, the launch carries a HipEventPair that is appended under `kind`; an entry that declines the
    shape (hipErrorNotSupported, 801) has launched nothing: the pair is dropped again.  Returns the entry's code."""
    launch = _lib.ChainLaunch(rows, groups)
    timed = chain_timers is not None and not torch.cuda.is_current_stream_capturing()
    if timed:
        from .gae import HipEventPair
        ev = HipEventPair()
        launch.ev_start_or_null, launch.ev_stop_or_null = ev.start, ev.stop
        chain_timers.setdefault(kind, []).append(ev)
    err = entry(*[ctypes.byref(d) for d in descs], ctypes.byref(launch), stream)
    if timed and err == 801:
        chain_timers[kind].pop()
    return err


class MlpChain:
    """The whole MLP (hidden layers + the fused value|mu head as the last layer) as ONE forward and
    ONE backward launch (csrc/mlp_chain.hip).  `layers`: list of (weight [out, in], bias [out], act
    name) - tensors are referenced, not copied, so optimiser updates are seen.  Raises
    NotImplementedError if the network does not fit the LDS even with one 16-row group.
    products: 'auto' - the library's choice per launch: fp16 plane products under fixed operand scales (the 64-row split
    kernels, the lean 16-row kernels; |weight| < 1023, |hidden activation| < 4094) wherever they apply - or 'exact': every
    launch of forward / backward / step takes the exact-f32-product kernels that split_products=False selects, which
    have the full fp32 range.  The attribute may be set at any time; it is part of cache_state().
    Derived weight copies (weight_forms.py), both fp16 plane fragments: `planes` (64-row split kernels), `frags` (lean)."""

    PRODUCTS = ('auto', 'exact')

    def __init__(self, layers, device, weights_version=None, products='auto'):
        self.n = n = len(layers)
        self.layers = layers
        self.device = device
        self.ins = [int(w.shape[1]) for w, _, _ in layers]
        self.outs = [int(w.shape[0]) for w, _, _ in layers]
        P, I, L = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_longlong * n
        self._P, self._I, self._L = P, I, L
        self._w = P(*[_need(w, F32, 'weight') for w, _, _ in layers])
        self._b = P(*[_need(b, F32, 'bias') for _, b, _ in layers])
        self._in, self._out = I(*self.ins), I(*self.outs)
        self._act = I(*[ACT_KINDS[a] for _, _, a in layers])
        self._net = _lib.ChainNet(n, *[ctypes.addressof(a) for a in (self._w, self._b, self._in, self._out, self._act)])
        lib = _lib.load()
        _lib.check(lib.rlg_mlp_chain_prepare(), 'rlg_mlp_chain_prepare')
        max_groups = {}
        for direction in (0, 1):
            best = 0
            for g in (1, 2, 4):
                if lib.rlg_mlp_chain_lds_bytes(n, self._in, self._out, g, direction) >= 0:
                    best = g
            if best == 0 and (direction == 0 or n > 1):
                raise NotImplementedError('MLP does not fit the LDS of the fused chain kernels')
            max_groups[direction] = best
        frag_bytes = [int(lib.rlg_mlp_chain_frags_bytes(n, self._in, self._out, 0)),
                      int(lib.rlg_mlp_chain_frags_bytes(n, self._in, self._out, 1)) if n > 1 else -1]
        # RLG_CHAIN_LEAN=0 keeps the pipelined kernels where the lean 16-row kernels would run
        self._set_shape(max_groups, frag_bytes, os.environ.get('RLG_CHAIN_LEAN', '1') != '0', weights_version, products)

    @classmethod
    def _from_shape(cls, n, max_groups, frag_bytes, weights_version=None, products='auto', lean=True, device=None):
        """Host-side tests: a chain of `n` layers from the library's answers about its shape.  It can launch nothing."""
        c = cls.__new__(cls)
        c.n, c.device, c._in, c._out = n, device, None, None
        c._set_shape(max_groups, frag_bytes, lean, weights_version, products)
        return c

    def _set_shape(self, max_groups, frag_bytes, lean, weights_version, products):
        self.max_groups = max_groups
        self._frag_bytes = frag_bytes
        self._lean = lean and frag_bytes[0] >= 0
        # callable -> a value that changes whenever the weights do (FlatArena.weights_token): the forms' stamp
        self._weights_version = weights_version
        self.planes = weight_forms.PlanesForm(self._alloc_planes, self._launch_pack_planes, jobs=2 * self.n - 1)
        self.frags = weight_forms.WeightForm(self._alloc_frags, self._launch_pack_frags)
        # split-fp16 backward: per 64-row workgroup the largest magnitude of every dZ tensor (csrc/bx_form.hpp), for the
        # weight-gradient launch that follows it; rows of the last backward that left them
        self._forms_read = {}
        self._grad_maxima = self._maxima_bwd = None
        self._maxima_rows = ctypes.c_int(0)   # what the last backward / step entry answered: rows per entry, 0: no maxima
        self._maxima_rows_at = ctypes.addressof(self._maxima_rows)
        self.maxima_rows_per_entry = 64       # 64: left by the 64-row split kernels, 16: by the lean 16-row kernels
        self._products = 'auto'
        self.products = products

    _planes = property(lambda self: self.planes.buffer)       # (None until a launch has asked for them)
    _frags = property(lambda self: self.frags.buffer)

    @property
    def products(self):
        return self._products

    @products.setter
    def products(self, mode):
        if mode not in self.PRODUCTS:
            raise ValueError(f"MlpChain products: 'auto' or 'exact' expected, got {mode!r}")
        if mode != self._products:
            self._products = mode
            self._maxima_bwd = None

    def _request_maxima(self, bwd, rows, per):
        """`bwd` asks its launch for one gradient-maxima entry per `per`-row workgroup (64: split, 16: lean)."""
        need = max(1024, -(-int(rows) // per))
        if self._grad_maxima is None or self._grad_maxima.shape[1] < need:
            self._grad_maxima = torch.zeros(8, need, dtype=F32, device=self.device)
        bwd.maxima_or_null, bwd.maxima_stride = self._grad_maxima.data_ptr(), self._grad_maxima.shape[1]

    def _maxima_left(self, rows):
        """Behind a backward / step launch of `rows` rows: whether it left maxima, and for how many rows per entry."""
        per = self._maxima_rows.value
        self._maxima_bwd = rows if per else None
        if per:
            self.maxima_rows_per_entry = per

    def gradient_maxima(self, rows):
        """[8, entries] fp32: row l = per 64-row workgroup the largest |dZ of layer l| of the backward of this step - when
        that backward (`rows` rows) ran the split-fp16 kernel, else None.  MlpDwPlan.launch(maxima=...) then runs its
        fp16 form."""
        if self._grad_maxima is not None and self._maxima_bwd == rows:
            return self._grad_maxima
        return None

    def _route(self, rows, kind, groups=0, split_products=None):
        """'lean' | 'split' | 'exact': the kernels for a launch of `kind` (0 inference forward, 1 backward, 2 training forward)
        over `rows` rows - lean 16-row (they read `frags`), else split 64-row (`planes`), else exact f32 products (the
        weights).  The PREFERENCE: the library may still decline a lean launch when issued (801); the exact one follows."""
        if self._products == 'exact' or split_products is False:
            return 'exact'
        def split(requested):
            return bool(_lib.load().rlg_mlp_chain_bx_supported(self.n, self._in, self._out, int(rows),
                                                               self.groups(rows, kind, requested), int(kind)))
        if (groups in (0, 1) and self._lean and (kind != 1 or self._frag_bytes[1] >= 0) and self.groups(rows, kind) == 1
                and not split(0)):
            return 'lean'
        return 'split' if split(groups) else 'exact'

    def lean_used(self, rows, direction, requested=0):
        """The launch runs the lean 16-row kernel (split-fp16 products on the fragments), row alignment permitting."""
        return self._route(rows, direction, requested) == 'lean'

    def split_products(self, rows, direction, requested=0):
        """The launch runs the 64-row split-product kernel.  Never under products='exact'."""
        return self._route(rows, direction, requested) == 'split'

    def forms_read(self, launches):
        """(fragments, planes): whether any of `launches` [(rows, kind), ...] reads them; kept per products mode."""
        key = (self._products, tuple(launches))
        if key not in self._forms_read:
            routes = [self._route(r, k) for r, k in key[1]]
            self._forms_read[key] = ('lean' in routes, 'split' in routes)
        return self._forms_read[key]

    def weights_token(self):
        return None if self._weights_version is None else self._weights_version()

    def cache_state(self):
        """What the forms hold, for callers that record launches WITHOUT running them (graph capture) and put it back behind
        (restore_cache_state).  Allocates the buffers (exact products: none): one first made under torch.cuda.graph would
        live in the graph's private pool and dangle behind a failed capture."""
        if self._products != 'exact':
            if self._lean:
                self.frags.allocate()
            try:
                self.planes.allocate()
            except ValueError:
                pass                      # (a network the split-product kernels do not take: they never ask for planes)
        p = self.planes
        return weight_forms.ChainSnapshot(p.holds, self.frags.holds, p.fresh, p.packed_once, self._products)

    def restore_cache_state(self, state):
        self.planes.holds, self.planes.fresh, self.planes.packed_once = state.planes, state.fresh, state.packed_once
        self.frags.holds, self.products = state.frags, state.products

    def _alloc_frags(self):                   # [forward | backward fragments], typed fp32 for its size only
        return torch.empty((self._frag_bytes[0] + max(self._frag_bytes[1], 0)) // 4, dtype=F32, device=self.device)

    def _frags_ptr(self, direction):
        return self.frags.allocate().data_ptr() + (self._frag_bytes[0] if direction == 1 else 0)

    def _launch_pack_frags(self, stream_of):
        bwd = self._frags_ptr(1) if self._frag_bytes[1] >= 0 else None
        _lib.check(_lib.load().rlg_mlp_chain_pack_frags_both(self.n, self._w, self._b, self._in, self._out, self._frags_ptr(0),
                                                             bwd, _stream(stream_of)), 'rlg_mlp_chain_pack_frags_both')

    def _alloc_planes(self):
        """ONE buffer for both directions: forward fragments at 0, backward fragments at _bwd_offset."""
        lib = _lib.load()
        nbytes = lib.rlg_mlp_chain_planes_bytes(self.n, self._in, self._out, 2)
        off = lib.rlg_mlp_chain_planes_offset(self.n, self._in, self._out, 1)
        if nbytes < 0 or off < 0:
            raise ValueError('rlg_mlp_chain_planes_bytes: bad network')
        self._bwd_offset = int(off)
        self._fwd_bytes, self._bwd_bytes = (int(lib.rlg_mlp_chain_planes_bytes(self.n, self._in, self._out, d)) for d in (0, 1))
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)

    def _plane_buffer(self):
        return self.planes.allocate()

    def _planes_ptr(self, direction):
        return self.planes.allocate().data_ptr() + (self._bwd_offset if direction == 1 else 0)

    def _launch_pack_planes(self, direction, stream_of):
        buf = self.planes.allocate()
        view = (buf[:self._fwd_bytes], buf[self._bwd_offset:self._bwd_offset + self._bwd_bytes], buf)[direction]
        if view.numel() > 0:
            _lib.check(_lib.load().rlg_mlp_chain_pack_planes(self.n, self._w, self._in, self._out, int(direction),
                                                             view.data_ptr(), _stream(stream_of)), 'rlg_mlp_chain_pack_planes')
        return view

    def pack_planes(self, direction, stream_of):
        """Weights -> fp16 plane fragments (direction 0 forward operand, 1 backward, 2 both); returns that direction's
        view (2: the whole buffer).  Stamps nothing: forward() / backward() pack for themselves unless planes.current()."""
        return self.planes.pack(stream_of, direction)

    def adam_pack_target(self):
        """(n, weights, in, out, planes address) for ops.adam_step(pack=...), or None when this network has no use for
        planes / no version source.  The first call packs the whole buffer once (the fragments' zero padding)."""
        if self._weights_version is None or self.n < 1 or self._products == 'exact':
            return None
        self.planes.pack_once(self.weights_token(), self.layers[0][0])
        return self.n, self._w, self._in, self._out, self.planes.allocate().data_ptr()

    def groups(self, rows, direction, requested=0):
        """direction names the launch kind: 0 inference forward, 1 backward, 2 training forward (csrc/mlp_chain.hip
        chain_bx_min_rows: the training pair takes the 64-row split kernels from 8,192 rows, inference from 16,384)."""
        g = _lib.load().rlg_mlp_chain_groups(int(rows), int(requested), int(direction))
        return min(g, self.max_groups[1 if direction == 1 else 0])

    def num_blocks(self, rows, direction, requested=0):
        return _lib.load().rlg_mlp_chain_num_blocks(int(rows), self.groups(rows, direction, requested))

    def _forward_args(self, x, outs, rms, eps, xn_out, rms_fold):
        """rlg_chain_fwd without its weight form: pointers and row strides of `outs` (per layer the activation output or
        None, the heads last), x and its row stride, the normaliser state, eps, xn_out, the five rms_fold pointers."""
        ptrs = self._P(*[None if t is None else _need(t, F32, 'act_out', contiguous=False) for t in outs])
        lds = self._L(*[0 if t is None else t.stride(0) for t in outs])
        _lib.require_gpu(x, 'x')
        if x.dtype != F32 or (x.dim() == 2 and x.shape[1] != 1 and x.stride(1) != 1):
            raise ValueError('x: fp32 rows with unit inner stride expected')
        mean = var = None
        if rms is not None:
            mean, var = _need(rms[0], F64, 'running_mean'), _need(rms[1], F64, 'running_var')
        fold = [None] * 5
        if rms_fold is not None:
            if rms is None:
                raise ValueError('rms_fold needs rms')
            row, cnt, mean_o, var_o, cnt_o = rms_fold
            if row.numel() != 2 * self.ins[0] + 1:
                raise ValueError('rms_fold: moments row of 2*in0+1 doubles expected')
            fold = [_need(row, F64, 'moments row'), _need(cnt, torch.int64, 'count'), _need(mean_o, F64, 'mean out'),
                    _need(var_o, F64, 'var out'), _need(cnt_o, torch.int64, 'count out')]
        fwd = _lib.ChainFwd(ctypes.addressof(ptrs), ctypes.addressof(lds), x.data_ptr(), x.stride(0), mean, var,
                            float(np.float32(eps)), _opt(xn_out, F32, 'xn_out'), *fold)
        fwd.arrays = ptrs, lds                          # (alive as long as the descriptor)
        return fwd

    def _backward_args(self, d_heads, acts, dz_out, bias_partials, ppo_loss):
        """rlg_chain_bwd without its weight form and maxima: d_heads, per hidden layer H (acts; None for the step entries,
        which read their forward half's), the dZ output and their row strides, the fp64 bias partials or None, the loss
        descriptor or None.  The entry's answer about maxima goes to _maxima_rows."""
        h = hl = None
        if acts is not None:
            h = self._P(*([_need(t, F32, 'H', contiguous=False) for t in acts] + [None]))
            hl = self._L(*([t.stride(0) for t in acts] + [0]))
        dz = self._P(*([_need(t, F32, 'dz', contiguous=False) for t in dz_out] + [None]))
        dl = self._L(*([t.stride(0) for t in dz_out] + [0]))
        bp = None
        if bias_partials is not None:
            bp = self._P(*([_need(t, F64, 'bias partials') for t in bias_partials] + [None]))
        at = ctypes.addressof
        bwd = _lib.ChainBwd(None if h is None else at(h), None if h is None else at(hl),
                            _need(d_heads, F32, 'd_heads', contiguous=False), d_heads.stride(0), at(dz), at(dl),
                            None if bp is None else at(bp), None if ppo_loss is None else at(ppo_loss), None, None, 0,
                            self._maxima_rows_at)
        bwd.arrays = h, hl, dz, dl, bp                  # (alive as long as the descriptor)
        return bwd

    def forward(self, x, heads, act_out=None, rms=None, eps=1e-5, xn_out=None, groups=0, rms_fold=None,
                split_products=None):
        """x [rows, in0] (row stride free), heads [rows, out_last] out.  act_out: per hidden layer a
        [rows, out_l] tensor or None.  rms = (running_mean, running_var) fp64 -> the observations are
        normalised on the way in (xn_out [rows, in0] optionally receives them).  rms_fold =
        (moments_row [2*in0+1] fp64, count int64, mean_out, var_out, count_out): training-mode
        RunningMeanStd - the minibatch's moments are folded into the state first, the new state is
        written to the *_out tensors (a second buffer set).
        split_products: None = the library's choice (_route), False = exact f32 products."""
        rows = x.shape[0]
        n = self.n
        outs = list(act_out) if act_out is not None else [None] * (n - 1)
        fwd = self._forward_args(x, outs + [heads], rms, eps, xn_out, rms_fold)
        # A training forward also leaves the planes of the backward that follows it: its own pack launch takes both
        # directions, an exact-product forward splits them in extra workgroups.  That backward alone uses them (fresh).
        kind = 2 if (act_out is not None and self.n > 1 and any(t is not None for t in act_out)) else 0
        route = self._route(rows, kind, groups, split_products)
        token = self.weights_token()
        self.planes.drop_fresh()
        timer = 'fwd_train' if act_out is not None else 'fwd_infer'
        if route == 'lean':
            self.frags.ensure(token, x)
            fwd.weight_form_or_null = self._frags_ptr(0)
            err = _chain_call(timer, _lib.load().rlg_mlp_chain_forward_lean, self._net, fwd, rows=rows, stream=_stream(x))
            if err != 801:                              # (hipErrorNotSupported: the pipelined / unit-structured launch)
                _lib.check(err, 'rlg_mlp_chain_forward_lean')
                return
        bwd_split = act_out is not None and n > 1 and self._route(rows, 1) == 'split'
        planes = fwd_planes = None
        if route == 'split':
            if not self.planes.current(token):
                self.planes.pack(x, 2 if bwd_split else 0)
                if bwd_split:
                    self.planes.mark(token)
            fwd_planes = self._planes_ptr(0)
        elif bwd_split and not self.planes.current(token):
            planes = self._planes_ptr(1)
        fwd.weight_form_or_null, fwd.pack_backward_planes_or_null = fwd_planes, planes
        _lib.check(_chain_call(timer, _lib.load().rlg_mlp_chain_forward, self._net, fwd, rows=rows, stream=_stream(x),
                               groups=self.groups(rows, kind, groups)), 'rlg_mlp_chain_forward')
        if bwd_split:                                   # (behind a launch that succeeded, for the weights as they are)
            self.planes.fresh = (rows, token)

    def step(self, x, heads, act_out, d_heads, dz_out, bias_partials, ppo_loss, rms=None, eps=1e-5, xn_out=None,
             rms_fold=None):
        """forward(x, heads, act_out, ...) and backward(d_heads, act_out, dz_out, bias_partials, ppo_loss=...) as ONE
        launch (rlg_mlp_chain_step: 16-row workgroups, minibatches < 16,384 rows).  Returns False - having launched
        nothing - when the shape is outside that kernel's envelope; the caller then issues the two launches."""
        rows = x.shape[0]
        n = self.n
        if act_out is None or any(t is None for t in act_out) or ppo_loss is None or n < 2:
            return False
        routes = (self._route(rows, 2), self._route(rows, 1))
        if 'split' in routes or self.groups(rows, 2) != 1 or self.groups(rows, 1) != 1:
            return False
        lean = routes == ('lean', 'lean')
        fwd = self._forward_args(x, list(act_out) + [heads], rms, eps, xn_out, rms_fold)
        bwd = self._backward_args(d_heads, None, dz_out, bias_partials, ppo_loss)
        if lean:
            # (outside the lean step's envelope the caller's two lean launches beat the pipelined one-launch step)
            self.frags.ensure(self.weights_token(), x)
            fwd.weight_form_or_null, bwd.weight_form_or_null = self._frags_ptr(0), self._frags_ptr(1)
            self._request_maxima(bwd, rows, 16)
        entry = 'rlg_mlp_chain_step_lean' if lean else 'rlg_mlp_chain_step'
        self._maxima_bwd = None
        err = _chain_call('step16', getattr(_lib.load(), entry), self._net, fwd, bwd, rows=rows, stream=_stream(x))
        if err == 801:                                  # hipErrorNotSupported: outside the fused kernel's envelope
            return False
        _lib.check(err, entry)
        self.planes.drop_fresh()
        self._maxima_left(rows)
        return True

    def backward(self, d_heads, acts, dz_out, bias_partials=None, groups=0, ppo_loss=None, split_products=None):
        """d_heads [rows, out_last]; acts / dz_out: per hidden layer H_l (forward's act_out) and the
        dZ_l output; bias_partials: per hidden layer fp64 [num_blocks(rows, 1), out_l] or None.
        ppo_loss = ops.ppo_loss_desc(...): the launch first evaluates the PPO loss of its row tiles, i.e.
        it produces d_heads itself (and the loss partials, the mu/sigma write-back).
        split_products: None = the library's choice (_route), False = exact f32 products."""
        rows = d_heads.shape[0]
        bwd = self._backward_args(d_heads, acts, dz_out, bias_partials, ppo_loss)
        route = self._route(rows, 1, groups, split_products)
        token = self.weights_token()
        fresh = self.planes.take_fresh(rows, token)             # (packed with the forward launch of this step)
        timer = 'bwd_loss' if ppo_loss is not None else 'bwd'
        self._maxima_bwd = None
        if route == 'lean':
            self.frags.ensure(token, d_heads)
            bwd.weight_form_or_null = self._frags_ptr(1)
            self._request_maxima(bwd, rows, 16)
            err = _chain_call(timer, _lib.load().rlg_mlp_chain_backward_lean, self._net, bwd, rows=rows,
                              stream=_stream(d_heads))
            if err != 801:
                _lib.check(err, 'rlg_mlp_chain_backward_lean')
                self._maxima_left(rows)
                return
        bwd.weight_form_or_null = bwd.maxima_or_null = None
        if route == 'split':
            if not self.planes.current(token) and not fresh:
                self.planes.pack(d_heads, 1)
            bwd.weight_form_or_null = self._planes_ptr(1)
            # the split-fp16 launch leaves the gradient maxima the weight-gradient launch scales by; whether it ran is
            # the library's answer
            self._request_maxima(bwd, rows, 64)
        _lib.check(_chain_call(timer, _lib.load().rlg_mlp_chain_backward, self._net, bwd, rows=rows, stream=_stream(d_heads),
                               groups=self.groups(rows, 1, groups)), 'rlg_mlp_chain_backward')
        self._maxima_left(rows)


# ------------------------------------------------------------------ MLP weight gradients (MFMA)

class MlpDwPlan:
    """All weight-gradient GEMMs of one MLP backward as one launch (csrc/mlp_dw.hip).

    shapes: [(No, Mi)] per weight matrix, for minibatches of `rows` rows.  The plan owns the split-K
    workspaces; `launch(jobs)` takes the (dz [rows, No], x [rows, Mi], grad [No, Mi]) tensors of the
    step.  Raises NotImplementedError when a shape is outside the kernel's envelope (callers use
    the library GEMMs then)."""

    def __init__(self, shapes, rows, device, target_blocks=None):
        import ctypes
        lib = _lib.load()
        n = len(shapes)
        if target_blocks is None:
            # 0: the library's default workgroup count; RLG_DW_BLOCKS: A/B measurements of it (tools only)
            target_blocks = max(int(os.environ.get('RLG_DW_BLOCKS') or 0), 0)
        self.rows, self.n, self.shapes = int(rows), n, [tuple(s) for s in shapes]
        self._plans = (ctypes.c_int * (4 * n))()
        self.workspaces = []
        for k, (No, Mi) in enumerate(self.shapes):
            p4 = (ctypes.c_int * 4)()
            need = lib.rlg_mlp_dw_plan(self.rows, No, Mi, target_blocks, p4)
            if need < 0:
                raise NotImplementedError(f'dW shape [{No} x {Mi}] is not supported by the MFMA path')
            self._plans[4 * k:4 * k + 4] = list(p4)
            self.workspaces.append(torch.empty(need, dtype=F32, device=device))
        P = ctypes.c_void_p * n
        self._dz, self._x, self._grad = P(), P(), P()
        self._ws = P(*[w.data_ptr() for w in self.workspaces])
        self._no = (ctypes.c_int * n)(*[s[0] for s in self.shapes])
        self._mi = (ctypes.c_int * n)(*[s[1] for s in self.shapes])
        # rlg_mlp_dw_desc from dz to plans4: the arrays live with the plan
        self._arrays = [ctypes.addressof(a) for a in (self._dz, self._x, self._ws, self._grad, self._no, self._mi, self._plans)]
        self._device = device

    def plan(self, k):
        return tuple(self._plans[4 * k:4 * k + 4])

    def finalize_blocks(self, colsums=(), loss_finalize=None):
        """Workgroups of the finalise launch (= entries of the optional norm partials)."""
        n = sum((No * Mi // 4 + 15) // 16 for No, Mi in self.shapes)
        n += sum((int(c[2]) + 15) // 16 for c in colsums)
        if loss_finalize is not None:
            n += 1 + (2 * loss_finalize.actions_num + 7) // 8
        return n

    FORMS = {None: -1, 'auto': -1, 'exact': 0, 'bf16': 1, 'fp16': 2}

    def launch(self, jobs, colsums=(), loss_finalize=None, norm=None, maxima=None, form=None):
        """jobs: (dz, x, grad) per planned layer.  maxima = (MlpChain.gradient_maxima() [8, entries], layer of each job's
        dz, fixed scale of each job's x - SPLIT_SCALE_HIDDEN / SPLIT_SCALE_OBS_NORM): the launch runs on three fp16 plane
        products per fp32 product (csrc/split_f16.hpp), dz scaled by the power of two the largest entry over a wave's
        rows asks for, x by the scale the forward splits the same tensor with; without them: six bf16 plane products.  colsums: optional (partials fp64 [blocks*cols],
        blocks, cols, out fp32 [cols]) items - bias gradients finished in the same finalise launch.
        loss_finalize: ops.loss_finalize_desc(...) - the PPO loss partials are folded there as well.
        norm = (partials fp64 [>= finalise blocks], grad_scale, step_counter int64 [1]): the finalise
        launch also leaves per-block sums of (g * grad_scale)^2 and advances the Adam step counter (what
        grad_sumsq does) - only meaningful when this launch writes every gradient of the arena.
        form: the product form of THIS launch - None / 'auto' the library's choice as described (the environment's
        RLG_DW_BF16 / RLG_DW_F16 are the defaults of that choice), 'exact' f32 products (the full fp32 range), 'bf16',
        'fp16' (needs maxima; |x| times its scale must stay below 65,504) - rlg_mlp_dw_launch_form.
        Returns the number of finalise blocks (= valid entries of the norm partials)."""
        import ctypes
        if form not in self.FORMS:
            raise ValueError(f'weight-gradient form {form!r}: one of {sorted(k for k in self.FORMS if k)} or None')
        if len(jobs) != self.n:
            raise ValueError('job count does not match the plan')
        nc = len(colsums)
        cs = ()
        if nc:                              # rlg_mlp_dw_desc's colsum_partials, colsum_blocks, colsum_cols, colsum_out
            P = ctypes.c_void_p * nc
            cs = (P(*[_need(c[0], F64, 'colsum partials') for c in colsums]), (ctypes.c_int * nc)(*[int(c[1]) for c in colsums]),
                  (ctypes.c_int * nc)(*[int(c[2]) for c in colsums]), P(*[_need(c[3], F32, 'colsum out') for c in colsums]))
        nfin = ctypes.c_int(0)
        if norm is not None:
            need = self.finalize_blocks(colsums, loss_finalize)
            if norm[0].numel() < need:
                raise ValueError(f'norm partials: {need} entries needed, {norm[0].numel()} given')
        for k, (dz, x, grad) in enumerate(jobs):
            No, Mi = self.shapes[k]
            if tuple(dz.shape) != (self.rows, No) or tuple(x.shape) != (self.rows, Mi) or \
                    tuple(grad.shape) != (No, Mi):
                raise ValueError(f'layer {k}: dz {tuple(dz.shape)} / x {tuple(x.shape)} / grad {tuple(grad.shape)} '
                                 f'do not match the planned [{self.rows}] x [{No} x {Mi}]')
            self._dz[k] = _need(dz, F32, 'dz')
            self._x[k] = _need(x, F32, 'x')
            self._grad[k] = _need(grad, F32, 'grad')
        desc = _lib.MlpDwDesc(
            self.n, self.rows, *self._arrays, nc, *([ctypes.addressof(a) for a in cs] or [None] * 4),
            None if loss_finalize is None else ctypes.addressof(loss_finalize),
            None if norm is None else _need(norm[0], F64, 'norm partials'),
            1.0 if norm is None else float(np.float32(norm[1])),
            None if norm is None else _need(norm[2], torch.int64, 'step_counter'), ctypes.addressof(nfin))
        if maxima is not None:
            entries, dzs, xscales = maxima[:3]
            if len(dzs) != self.n or len(xscales) != self.n or entries.dim() != 2 or entries.shape[0] != 8:
                raise ValueError('maxima: [8, entries] fp32, one dz layer and one x scale per job')
            desc.maxima_or_null, desc.maxima_stride = _need(entries, F32, 'gradient maxima'), int(entries.shape[1])
            desc.maxima_rows_per_entry = int(maxima[3]) if len(maxima) > 3 else 64   # 64, or 16 (the lean kernels)
            slots = (ctypes.c_int * self.n)(*[int(v) for v in dzs])
            scales = (ctypes.c_float * self.n)(*[float(v) for v in xscales])
            desc.dz_slot, desc.x_scale = ctypes.addressof(slots), ctypes.addressof(scales)
        stream = _lib.stream_handle(self._device)
        if self.FORMS[form] < 0:
            _lib.check(_lib.load().rlg_mlp_dw_launch(ctypes.byref(desc), stream), 'rlg_mlp_dw_launch')
        else:
            _lib.check(_lib.load().rlg_mlp_dw_launch_form(self.FORMS[form], ctypes.byref(desc), stream),
                       'rlg_mlp_dw_launch_form')
        return nfin.value


# ------------------------------------------------------------------ recurrent policy (LSTM, GRU)

# One problem's descriptor (_lib.LstmFwd, ...) from the arguments of the wrapper below it: the shapes that must agree
# with gates, then _need or _opt per field, in the descriptor's order.

def _lstm_fwd(gates, w_hh, h0, c0, dones, out, c_all=None, hprev=None, h_final=None, c_final=None):
    G = gates.shape[1]
    H = G // 4
    if G != 4 * H or tuple(w_hh.shape) != (G, H) or out.shape != (gates.shape[0], H):
        raise ValueError(f'gates [rows, 4H], w_hh [4H, H] and out [rows, H] do not agree: {tuple(gates.shape)}, '
                         f'{tuple(w_hh.shape)}, {tuple(out.shape)}')
    return _lib.LstmFwd(_need(gates, F32, 'gates'), _need(w_hh, F32, 'w_hh'), _need(h0, F32, 'h0'),
                        _need(c0, F32, 'c0'), _opt(dones, torch.uint8, 'dones'), _need(out, F32, 'out'),
                        _opt(c_all, F32, 'c_all'), _opt(hprev, F32, 'hprev'), _opt(h_final, F32, 'h_final'),
                        _opt(c_final, F32, 'c_final'))


def _lstm_bwd(gates, c_all, c0, dones, w_hh, d_out, d_gates):
    G = gates.shape[1]
    H = G // 4
    if G != 4 * H or tuple(w_hh.shape) != (G, H) or d_gates.shape != gates.shape:
        raise ValueError(f'gates / d_gates [rows, 4H] and w_hh [4H, H] do not agree: {tuple(gates.shape)}, '
                         f'{tuple(d_gates.shape)}, {tuple(w_hh.shape)}')
    return _lib.LstmBwd(_need(gates, F32, 'gates'), _need(c_all, F32, 'c_all'), _need(c0, F32, 'c0'),
                        _opt(dones, torch.uint8, 'dones'), _need(w_hh, F32, 'w_hh'), _need(d_out, F32, 'd_out'),
                        _need(d_gates, F32, 'd_gates'))


def _gru_fwd(gates, w_hh, b_hh, h0, dones, out, hn_all=None, hprev=None, h_final=None):
    G = gates.shape[1]
    H = G // 3
    if G != 3 * H or tuple(w_hh.shape) != (G, H) or b_hh.numel() != G:
        raise ValueError(f'gates [rows, 3H], w_hh [3H, H] and b_hh [3H] do not agree: {tuple(gates.shape)}, '
                         f'{tuple(w_hh.shape)}, {tuple(b_hh.shape)}')
    return _lib.GruFwd(_need(gates, F32, 'gates'), _need(w_hh, F32, 'w_hh'), _need(b_hh, F32, 'b_hh'),
                       _need(h0, F32, 'h0'), _opt(dones, torch.uint8, 'dones'), _need(out, F32, 'out'),
                       _opt(hn_all, F32, 'hn_all'), _opt(hprev, F32, 'hprev'), _opt(h_final, F32, 'h_final'))


def _gru_bwd(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh):
    G = gates.shape[1]
    H = G // 3
    if G != 3 * H or tuple(w_hh.shape) != (G, H) or d_gx.shape != gates.shape or d_gh.shape != gates.shape:
        raise ValueError(f'gates / d_gx / d_gh [rows, 3H] and w_hh [3H, H] do not agree: {tuple(gates.shape)}, '
                         f'{tuple(d_gx.shape)}, {tuple(d_gh.shape)}, {tuple(w_hh.shape)}')
    return _lib.GruBwd(_need(gates, F32, 'gates'), _need(hn_all, F32, 'hn_all'), _need(hprev, F32, 'hprev'),
                       _opt(dones, torch.uint8, 'dones'), _need(w_hh, F32, 'w_hh'), _need(d_out, F32, 'd_out'),
                       _need(d_gx, F32, 'd_gx'), _need(d_gh, F32, 'd_gh'))


# (cell, direction): the entry, one problem's descriptor from its arguments, an array of two, the gates per unit
_RNN_SEQ = {
    ('lstm', 'forward'): ('rlg_lstm_seq_forward', _lstm_fwd, _lib.LstmFwd * 2, 4),
    ('lstm', 'backward'): ('rlg_lstm_seq_backward', _lstm_bwd, _lib.LstmBwd * 2, 4),
    ('gru', 'forward'): ('rlg_gru_seq_forward', _gru_fwd, _lib.GruFwd * 2, 3),
    ('gru', 'backward'): ('rlg_gru_seq_backward', _gru_bwd, _lib.GruBwd * 2, 3),
}


def rnn_seq(cell, direction, problems, seq_len):
    """One sequence launch: cell 'lstm' / 'gru', direction 'forward' / 'backward', on one or two problems - each the
    arguments of {cell}_seq_{direction} below in its order, without seq_len, as a tuple.  Two problems have one shape
    and run in ONE launch (twice the workgroups; bit-identical to the two single launches); dones and the optional
    outputs may be given for one problem and not for the other.  No output buffer may be shared.
    (The four single-problem wrappers below make the same call for one problem without the way through the table: a
    T = 1 launch is host-bound, and they are what a caller outside a captured graph uses.)"""
    entry, describe, pair_type, gates_per_unit = _RNN_SEQ[cell, direction]
    n = len(problems)
    if n != 1 and n != 2:
        raise ValueError(f'{entry}: one or two problems, {n} given')
    gates = problems[0][0]
    if n == 2:
        descs = pair_type(describe(*problems[0]), describe(*problems[1]))
        if problems[1][0].shape != gates.shape:
            raise ValueError(f'a paired launch needs two problems of one shape: gates {tuple(gates.shape)} and '
                             f'{tuple(problems[1][0].shape)}')
    B, G = gates.shape
    if (B // seq_len) * seq_len != B:
        raise ValueError(f'rows ({B}) must be a multiple of seq_len ({seq_len})')
    if n == 1:
        descs = ctypes.byref(describe(*problems[0]))
    _lib.check(getattr(_lib.load(), entry)(descs, n, B // seq_len, seq_len, G // gates_per_unit, _stream(gates)), entry)


def lstm_supported(hidden):
    """16, 32, 64 (W_hh in LDS, csrc/lstm.hip) and 128 (W_hh in registers as MFMA fragments, csrc/lstm_wide.hip)."""
    return bool(_lib.load().rlg_lstm_supported(int(hidden)))


def lstm_seq_forward(gates, w_hh, h0, c0, dones, out, c_all=None, hprev=None, h_final=None, c_final=None,
                     seq_len=1):
    """gates [S*T, 4H] (row = seq*seq_len + t): input projection (+ both biases) in, activated gates out; out [S*T, H].
    c_all / hprev [S*T, H] (cell states, state entering each step after the reset) are kept for backward when given,
    h_final / c_final [S, H] likewise.  H must satisfy lstm_supported: csrc/lstm.hip (16/32/64) or
    csrc/lstm_wide.hip (128, w_hh 16-byte aligned)."""
    B, G = gates.shape
    if (B // seq_len) * seq_len != B:
        raise ValueError(f'rows ({B}) must be a multiple of seq_len ({seq_len})')
    desc = _lstm_fwd(gates, w_hh, h0, c0, dones, out, c_all, hprev, h_final, c_final)
    _lib.check(_lib.load().rlg_lstm_seq_forward(ctypes.byref(desc), 1, B // seq_len, seq_len, G // 4, _stream(gates)),
               'rlg_lstm_seq_forward')


def lstm_seq_backward(gates, c_all, c0, dones, w_hh, d_out, d_gates, seq_len):
    """d_gates [S*T, 4H] = d loss / d gate pre-activations from d_out [S*T, H] and what lstm_seq_forward kept.
    Same widths as lstm_seq_forward; the weight gradients are whole-sequence products of d_gates outside."""
    B, G = gates.shape
    if (B // seq_len) * seq_len != B:
        raise ValueError(f'rows ({B}) must be a multiple of seq_len ({seq_len})')
    desc = _lstm_bwd(gates, c_all, c0, dones, w_hh, d_out, d_gates)
    _lib.check(_lib.load().rlg_lstm_seq_backward(ctypes.byref(desc), 1, B // seq_len, seq_len, G // 4, _stream(gates)),
               'rlg_lstm_seq_backward')


def gru_supported(hidden):
    """16, 32, 64 (W_hh in LDS, csrc/gru.hip) and 128 (W_hh in registers as MFMA fragments, csrc/gru_wide.hip)."""
    return bool(_lib.load().rlg_gru_supported(int(hidden)))


def gru_seq_forward(gates, w_hh, b_hh, h0, dones, out, hn_all=None, hprev=None, h_final=None, seq_len=1):
    """gates [S*T, 3H] (row = seq*seq_len + t): x W_ih^T + b_ih in, activated (r, z, n) out; b_hh [3H]; out [S*T, H].
    hn_all / hprev [S*T, H] (W_hn h + b_hn before the gating by r, state entering each step after the reset) are kept
    for backward when given, h_final [S, H] likewise.  H must satisfy gru_supported: csrc/gru.hip (16/32/64) or
    csrc/gru_wide.hip (128, w_hh 16-byte aligned)."""
    B, G = gates.shape
    if (B // seq_len) * seq_len != B:
        raise ValueError(f'rows ({B}) must be a multiple of seq_len ({seq_len})')
    desc = _gru_fwd(gates, w_hh, b_hh, h0, dones, out, hn_all, hprev, h_final)
    _lib.check(_lib.load().rlg_gru_seq_forward(ctypes.byref(desc), 1, B // seq_len, seq_len, G // 3, _stream(gates)),
               'rlg_gru_seq_forward')


def gru_seq_backward(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh, seq_len):
    """From d_out [S*T, H] and what gru_seq_forward kept: d_gx [S*T, 3H] = (dr_pre, dz_pre, dn_pre), the gradient of
    x W_ih^T + b_ih, and d_gh [S*T, 3H] = (dr_pre, dz_pre, dn_pre * r), the gradient of h W_hh^T + b_hh.  The weight
    gradients are whole-sequence products of the two outside (dW_ih = d_gx^T x, dW_hh = d_gh^T hprev)."""
    B, G = gates.shape
    if (B // seq_len) * seq_len != B:
        raise ValueError(f'rows ({B}) must be a multiple of seq_len ({seq_len})')
    desc = _gru_bwd(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh)
    _lib.check(_lib.load().rlg_gru_seq_backward(ctypes.byref(desc), 1, B // seq_len, seq_len, G // 3, _stream(gates)),
               'rlg_gru_seq_backward')


# Two problems of one shape in ONE launch, a and b each a tuple as rnn_seq takes it: the names under which
# tests/test_rnn_pair_gpu.py makes its paired launches; everything else calls rnn_seq.
def lstm_seq_forward_pair(a, b, seq_len=1):
    rnn_seq('lstm', 'forward', (a, b), seq_len)


def lstm_seq_backward_pair(a, b, seq_len):
    rnn_seq('lstm', 'backward', (a, b), seq_len)


def gru_seq_forward_pair(a, b, seq_len=1):
    rnn_seq('gru', 'forward', (a, b), seq_len)


def gru_seq_backward_pair(a, b, seq_len):
    rnn_seq('gru', 'backward', (a, b), seq_len)


# ------------------------------------------------------------------ layer norm behind the recurrent layer

def rnn_layer_norm_blocks(rows, hidden):
    """Workgroups (= rows of the fp64 column partials) of rnn_layer_norm_backward; 0: width outside 16 / 32 / 64 / 128
    or no rows."""
    return _lib.load().rlg_rnn_layer_norm_num_blocks(int(rows), int(hidden))


def rnn_layer_norm_forward(x, gamma, beta, eps, y, stats=None):
    """y = nn.LayerNorm(H)(x) for x [rows, H] behind the RNN (csrc/rnn_layer_norm.hip); stats [rows, 2] receives each
    row's (mean, rstd) for rnn_layer_norm_backward (None: inference)."""
    for t, name in ((x, 'x'), (gamma, 'gamma'), (beta, 'beta'), (y, 'y')):
        _need(t, F32, name)
    rows, H = x.shape
    if y.shape != x.shape or gamma.numel() != H or beta.numel() != H or (stats is not None and stats.shape != (rows, 2)):
        raise ValueError(f'rnn_layer_norm_forward: x / y [rows, H], gamma / beta [H] and stats [rows, 2] do not agree: '
                         f'{tuple(x.shape)}, {tuple(y.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}')
    _lib.check(_lib.load().rlg_rnn_layer_norm_forward(
        _need(x, F32, 'x'), _need(gamma, F32, 'gamma'), _need(beta, F32, 'beta'), float(eps), _need(y, F32, 'y'),
        _opt(stats, F32, 'stats'), rows, H, _stream(x)), 'rlg_rnn_layer_norm_forward')


def rnn_layer_norm_backward(d_y, x, stats, gamma, d_x, d_gamma_partials, d_beta_partials, num_blocks):
    """d_x from d_y, the forward's input x and its stats; d_gamma_partials / d_beta_partials fp64 [num_blocks * H]: the
    column partials of d gamma = sum d_y * xhat and d beta = sum d_y for colsum_finalize / MlpDwPlan.launch(colsums=)."""
    for t, name in ((d_y, 'd_y'), (x, 'x'), (stats, 'stats'), (gamma, 'gamma'), (d_x, 'd_x')):
        _need(t, F32, name)
    rows, H = x.shape
    if d_y.shape != x.shape or d_x.shape != x.shape or stats.shape != (rows, 2) or gamma.numel() != H:
        raise ValueError(f'rnn_layer_norm_backward: d_y / x / d_x [rows, H], stats [rows, 2] and gamma [H] do not agree: '
                         f'{tuple(d_y.shape)}, {tuple(x.shape)}, {tuple(d_x.shape)}, {tuple(stats.shape)}')
    if min(d_gamma_partials.numel(), d_beta_partials.numel()) < int(num_blocks) * H:
        raise ValueError(f'rnn_layer_norm_backward: {int(num_blocks) * H} partials needed per array')
    _lib.check(_lib.load().rlg_rnn_layer_norm_backward(
        _need(d_y, F32, 'd_y'), _need(x, F32, 'x'), _need(stats, F32, 'stats'), _need(gamma, F32, 'gamma'),
        _need(d_x, F32, 'd_x'), _need(d_gamma_partials, F64, 'd_gamma_partials'),
        _need(d_beta_partials, F64, 'd_beta_partials'), int(num_blocks), rows, H, _stream(x)),
        'rlg_rnn_layer_norm_backward')


# ------------------------------------------------------------------ value tail behind the recurrent layer of a critic

def rnn_value_tail_blocks(rows, hidden):
    """Workgroups (= rows of the fp64 partials) of rnn_value_tail; 0: width outside 16 / 32 / 64 / 128 or no rows."""
    return _lib.load().rlg_rnn_value_tail_num_blocks(int(rows), int(hidden))


def rnn_value_head(feat, w, b, values):
    """values [rows] = feat [rows, H] w [H] + b [1] (csrc/rnn_value_tail.hip, the inference form): fp64 products and
    sum, one rounding."""
    for t, name in ((feat, 'feat'), (w, 'w'), (b, 'b'), (values, 'values')):
        _need(t, F32, name)
    rows, H = feat.shape
    if w.numel() != H or b.numel() != 1 or values.numel() != rows:
        raise ValueError(f'rnn_value_head: feat [rows, H], w [H], b [1] and values [rows] do not agree: '
                         f'{tuple(feat.shape)}, {tuple(w.shape)}, {tuple(b.shape)}, {tuple(values.shape)}')
    _lib.check(_lib.load().rlg_rnn_value_head(
        _need(feat, F32, 'feat'), _need(w, F32, 'w'), _need(b, F32, 'b'), _need(values, F32, 'values'), rows, H,
        _stream(feat)), 'rlg_rnn_value_head')


def rnn_value_tail(feat, w, b, old_values, returns, values, d_values, d_feat, loss_partials, d_w_partials, d_b_partials,
                   num_blocks, e_clip, clip_value=True, mask=None, mask_sum=None):
    """The value column over feat [rows, H], the critic loss of value_loss on it and its backward in one launch: values /
    d_values [rows], d_feat [rows, H]; loss_partials fp64 [num_blocks * 7] for ppo_loss_finalize(actions_num 0),
    d_w_partials fp64 [num_blocks * H] and d_b_partials fp64 [num_blocks] for colsum_finalize /
    MlpDwPlan.launch(colsums=).  num_blocks: rnn_value_tail_blocks(rows, H)."""
    for t, name in ((feat, 'feat'), (w, 'w'), (b, 'b'), (old_values, 'old_values'), (returns, 'returns'),
                    (values, 'values'), (d_values, 'd_values'), (d_feat, 'd_feat')):
        _need(t, F32, name)
    rows, H = feat.shape
    if (w.numel() != H or b.numel() != 1 or d_feat.shape != feat.shape
            or any(t.numel() != rows for t in (old_values, returns, values, d_values))
            or (mask is not None and mask.numel() != rows)):
        raise ValueError(f'rnn_value_tail: feat / d_feat [rows, H], w [H], b [1] and {rows} rows of old_values / returns '
                         f'/ values / d_values / mask expected: {tuple(feat.shape)}, {tuple(d_feat.shape)}, {tuple(w.shape)}')
    nb = int(num_blocks)
    if loss_partials.numel() < nb * 7 or d_w_partials.numel() < nb * H or d_b_partials.numel() < nb:
        raise ValueError(f'rnn_value_tail: {nb * 7} / {nb * H} / {nb} partials needed')
    _lib.check(_lib.load().rlg_rnn_value_tail(
        _need(feat, F32, 'feat'), _need(w, F32, 'w'), _need(b, F32, 'b'), _need(old_values, F32, 'old_values'),
        _need(returns, F32, 'returns'), _opt(mask, F32, 'mask'), _opt(mask_sum, F32, 'mask_sum'),
        _need(values, F32, 'values'), _need(d_values, F32, 'd_values'), _need(d_feat, F32, 'd_feat'),
        _need(loss_partials, F64, 'loss_partials'), _need(d_w_partials, F64, 'd_w_partials'),
        _need(d_b_partials, F64, 'd_b_partials'), nb, rows, H, float(np.float32(e_clip)), 1 if clip_value else 0,
        _stream(feat)), 'rlg_rnn_value_tail')
