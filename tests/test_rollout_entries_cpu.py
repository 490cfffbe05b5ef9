"""CPU: the rollout step's entry points and the discrete loss (csrc/experience.hip, csrc/rollout_categorical.hip,
csrc/ppo_loss.hip) at the boundary.

Each of the four takes one descriptor.  Every malformed call listed in include/rlg_hip.h is answered on the host -
hipErrorInvalidValue, more than 16 branches of the categorical head hipErrorNotSupported - before the runtime is asked
for anything; no rows returns 0.  The table runs in a child process that sees no GPU, as tests/test_play_entries_cpu.py
does: the pointers are small fake addresses the host code dereferences none of (the branch sizes are a real host array),
and the well-formed calls of each entry show the runtime's own code, which is not hipErrorInvalidValue.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, NOT_SUPPORTED = 1, 801
ENTRIES = {'rlg_rollout_post_step': 'PostStepDesc', 'rlg_rollout_policy_head': 'PolicyHeadDesc',
           'rlg_rollout_categorical_head': 'CategoricalHeadDesc', 'rlg_ppo_loss_discrete_nlp': 'DiscreteLossDesc'}
P = [0x100000 * (k + 1) for k in range(20)]            # fake aligned addresses

POST_REQUIRED = ('rewards', 'dones', 'values', 'rewards_buf', 'cur_rewards', 'cur_shaped', 'cur_lengths', 'ep_partials')
HEAD_REQUIRED = ('heads', 'logstd', 'noise', 'actions_out', 'values_out', 'buf_actions', 'buf_mus', 'buf_sigmas',
                 'buf_neglogp', 'buf_values')
CAT_REQUIRED = ('logits', 'branch_sizes', 'exp_noise', 'value', 'actions_out', 'values_out', 'buf_actions',
                'buf_neglogp', 'buf_values')
LOSS_REQUIRED = ('logits', 'values', 'actions', 'branch_sizes', 'old_neglogp', 'advantages', 'old_values', 'returns',
                 'd_logits', 'd_values', 'partials')


def _fill(entry, base, o):
    """(entry, fields): the well-formed description with the overrides `o`; desc=None stands for a NULL descriptor."""
    if o.get('desc', 0) is None:
        return (entry, None)
    a = dict(base)
    a.update(o)
    return (entry, a)


def _post(**o):
    base = dict({k: P[i] for i, k in enumerate(POST_REQUIRED)}, time_outs=P[8], time_outs_kind=1, live_rows=P[9],
                shift=0.0, scale=1.0, rmin=-1.0, rmax=1.0, clamp_rewards=1, bootstrap=1, gamma=0.99, N=5, H=4, V=1, step=2,
                num_agents=1)
    return _fill('rlg_rollout_post_step', base, o)


def _head(**o):
    base = dict({k: P[i] for i, k in enumerate(HEAD_REQUIRED)}, ld=4, eps=1e-5, N=5, H=4, A=3, step=2)
    return _fill('rlg_rollout_policy_head', base, o)


def _cat(**o):
    base = dict({k: P[i] for i, k in enumerate(CAT_REQUIRED)}, ld_logits=7, branch_sizes=[3, 4], masks_or_null=P[9],
                ld_masks=7, ld_value=1, value_repeat=1, eps=1e-5, num_envs=5, horizon=4, step=2)
    return _fill('rlg_rollout_categorical_head', base, o)


def _loss(**o):
    base = dict({k: P[i] for i, k in enumerate(LOSS_REQUIRED)}, ld_logits=7, ld_values=1, branch_sizes=[3, 4],
                ld_d_logits=7, ld_d_values=1, minibatch=5, e_clip=0.2, critic_coef=1.0, entropy_coef=0.01, clip_value=1,
                use_smooth_clamp=0)
    return _fill('rlg_ppo_loss_discrete_nlp', base, o)


VALUE = dict(value=P[12], ld_value=1, value_repeat=1)      # the policy head with a value column of its own
STATS = dict(v_mean=P[13], v_var=P[14])
CLIP = dict(env_actions_out=P[15], act_low=P[16], act_high=P[17])


def _rows():
    """(id, (entry, fields), expected code; None: reaches the runtime, whose code is its own and not INVALID)"""
    t = [('post: well formed', _post(), None), ('post: no time_outs, no live_rows', _post(time_outs=None, live_rows=None), None),
         ('post: num_agents 0 is read as 1', _post(num_agents=0), None), ('post: V 8', _post(V=8), None),
         ('post: no descriptor', _post(desc=None), INVALID),
         ('post: N 0', _post(N=0), 0), ('post: N < 0', _post(N=-3), 0), ('post: N 0 comes first', _post(N=0, rewards=None, V=0), 0),
         ('post: V 0', _post(V=0), INVALID), ('post: V 9', _post(V=9), INVALID),
         ('post: step < 0', _post(step=-1), INVALID), ('post: step = H', _post(step=4), INVALID)]
    t += [(f'post: no {k}', _post(**{k: None}), INVALID) for k in POST_REQUIRED]
    t += [('head: well formed, value NULL', _head(), None),
          ('head: value NULL, ld_value and value_repeat not read', _head(ld_value=0, value_repeat=0), None),
          ('head: value given', _head(**VALUE), None), ('head: value for 5 agents', _head(**dict(VALUE, value_repeat=5)), None),
          ('head: value statistics', _head(**STATS), None), ('head: env actions', _head(**CLIP), None),
          ('head: no descriptor', _head(desc=None), INVALID),
          ('head: N 0', _head(N=0), 0), ('head: N < 0', _head(N=-1), 0), ('head: N 0 comes first', _head(N=0, heads=None, A=0), 0),
          ('head: step < 0', _head(step=-1), INVALID), ('head: step = H', _head(step=4), INVALID),
          ('head: A 0', _head(A=0), INVALID), ('head: A < 0', _head(A=-2), INVALID),
          ('head: env actions without low', _head(**dict(CLIP, act_low=None)), INVALID),
          ('head: env actions without high', _head(**dict(CLIP, act_high=None)), INVALID),
          ('head: v_mean without v_var', _head(v_mean=P[13]), INVALID),
          ('head: value_repeat 0', _head(**dict(VALUE, value_repeat=0)), INVALID),
          ('head: value_repeat < 0', _head(**dict(VALUE, value_repeat=-2)), INVALID),
          ('head: ld_value 0', _head(**dict(VALUE, ld_value=0)), INVALID)]
    t += [(f'head: no {k}', _head(**{k: None}), INVALID) for k in HEAD_REQUIRED]
    t += [('cat: well formed', _cat(), None), ('cat: no masks, ld_masks not read', _cat(masks_or_null=None, ld_masks=0), None),
          ('cat: value statistics', _cat(v_mean_or_null=P[13], v_var_or_null=P[14]), None),
          ('cat: value for 5 agents', _cat(value_repeat=5, ld_value=3), None),
          ('cat: 16 branches', _cat(branch_sizes=[2] * 16, ld_logits=32, ld_masks=32), None),
          ('cat: no descriptor', _cat(desc=None), INVALID),
          ('cat: num_envs 0', _cat(num_envs=0), 0), ('cat: num_envs < 0', _cat(num_envs=-4), 0),
          ('cat: num_envs 0 comes first', _cat(num_envs=0, logits=None, branch_sizes=[2] * 17), 0),
          ('cat: 17 branches', _cat(branch_sizes=[2] * 17, ld_logits=34, ld_masks=34), NOT_SUPPORTED),
          ('cat: no branches', _cat(branch_sizes=[]), INVALID),
          ('cat: branch size 0', _cat(branch_sizes=[3, 0]), INVALID), ('cat: branch size < 0', _cat(branch_sizes=[-1, 4]), INVALID),
          ('cat: ld_logits 0', _cat(ld_logits=0), INVALID), ('cat: ld_logits below the columns', _cat(ld_logits=6), INVALID),
          ('cat: ld_masks 0', _cat(ld_masks=0), INVALID), ('cat: ld_masks below the columns', _cat(ld_masks=6), INVALID),
          ('cat: step < 0', _cat(step=-1), INVALID), ('cat: step = horizon', _cat(step=4), INVALID),
          ('cat: v_mean without v_var', _cat(v_mean_or_null=P[13]), INVALID),
          ('cat: value_repeat 0', _cat(value_repeat=0), INVALID), ('cat: value_repeat < 0', _cat(value_repeat=-2), INVALID),
          ('cat: ld_value 0', _cat(ld_value=0), INVALID)]
    t += [(f'cat: no {k}', _cat(**{k: None}), INVALID) for k in CAT_REQUIRED]
    t += [('loss: well formed', _loss(), None),
          ('loss: masks, row mask, neglogp out', _loss(action_masks_or_null=P[12], mask_or_null=P[13], mask_sum_or_null=P[14],
                                                       new_neglogp_or_null=P[15]), None),
          ('loss: heads inside wider rows', _loss(ld_logits=9, ld_values=9, ld_d_logits=8, ld_d_values=8), None),
          ('loss: 16 branches', _loss(branch_sizes=[2] * 16, ld_logits=32, ld_d_logits=32), None),
          ('loss: no descriptor', _loss(desc=None), INVALID),
          ('loss: minibatch 0', _loss(minibatch=0), INVALID), ('loss: minibatch < 0', _loss(minibatch=-5), INVALID),
          ('loss: 17 branches', _loss(branch_sizes=[2] * 17, ld_logits=34, ld_d_logits=34), INVALID),
          ('loss: no branches', _loss(branch_sizes=[]), INVALID),
          ('loss: branch size 0', _loss(branch_sizes=[3, 0]), INVALID), ('loss: branch size < 0', _loss(branch_sizes=[-1, 4]), INVALID),
          ('loss: ld_values 0', _loss(ld_values=0), INVALID), ('loss: ld_d_values 0', _loss(ld_d_values=0), INVALID),
          ('loss: ld_logits below the columns', _loss(ld_logits=6), INVALID),
          ('loss: ld_d_logits below the columns', _loss(ld_d_logits=6), INVALID),
          ('loss: mask without its sum', _loss(mask_or_null=P[13]), INVALID)]
    t += [(f'loss: no {k}', _loss(**{k: None}), INVALID) for k in LOSS_REQUIRED]
    return t


def run_table():
    sys.path.insert(0, ROOT)
    from rl_games_amd import _lib
    lib = _lib.load()
    codes = {}
    for name, (entry, fields), _ in _rows():
        assert name not in codes, name
        address, keep = None, []
        if fields is not None:
            fields = dict(fields)
            if 'branch_sizes' in fields:                  # a host array; None: a NULL array said to hold two sizes
                sizes = fields.pop('branch_sizes')
                keep.append((ctypes.c_int * max(len(sizes or ()), 1))(*(sizes or ())))
                fields.update(branch_sizes=None if sizes is None else ctypes.addressof(keep[0]),
                              num_branches=2 if sizes is None else len(sizes))
            desc = getattr(_lib, ENTRIES[entry])(**fields)
            address = ctypes.addressof(desc)
        codes[name] = getattr(lib, entry)(address, None)
    return codes


def test_the_entries_are_exported_and_bound():
    from rl_games_amd import _lib
    lib, table = _lib.load(), _lib.exported_prototypes()
    for name in ENTRIES:
        assert hasattr(lib, name) and table[name] == [ctypes.c_void_p, ctypes.c_void_p], name


def test_malformed_rollout_calls_are_rejected_on_the_host():
    env = dict(os.environ)
    env['HIP_VISIBLE_DEVICES'] = '-1'             # no device for the child: nothing that got past validation reaches one
    env['CUDA_VISIBLE_DEVICES'] = '-1'
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    codes = json.loads(out.stdout.strip().splitlines()[-1])
    rows = _rows()
    assert set(codes) == {r[0] for r in rows}
    wrong = {name: codes[name] for name, _, want in rows
             if (codes[name] != want if want is not None else codes[name] in (0, INVALID, NOT_SUPPORTED))}
    assert not wrong, f'codes against the table: {wrong}'


if __name__ == '__main__':
    print(json.dumps(run_table()))
