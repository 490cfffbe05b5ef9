"""Host side of the range guard of the split-fp16 products (INTEGRATION.md "Range limit").

The fused chain kernels and the fp16 weight-gradient form multiply fp16 planes under FIXED operand scales
(csrc/bx_form.hpp): a hidden activation of 4,094 or more, or a weight of 1,023 or more, is Inf in its plane and
everything computed from it is Inf / NaN - never a finite wrong value.  The reference keeps the fp32 range.  Two
configuration keys, honoured by A2CAgent, DiscreteA2CAgent and CentralValueTrain:

  split_range     'warn'  (default) the guard is not armed: one RuntimeWarning behind the first non-finite epoch, nothing
                          else - no extra launch, the unguarded optimiser entries.
                  'raise' armed; a trip raises SplitRangeError.
                  'exact' armed; a trip prints one notice, drops the rest of that epoch's work, puts every chain of the
                          agent on exact fp32 products (the weight gradients too) and training goes on.
  chain_products  'auto'  (default) the library's choice of product form per launch.
                  'exact' exact fp32 products from the start: no range limit, slower kernels.

Armed, nothing computed from an overflowed plane reaches parameters, Adam moments, learning rate or normalisers:
one rlg_range_scan launch at the end of the rollout looks through what the policy (and a central value critic) wrote and
through the returns - they carry the bootstrap values of the observation behind the last step, which no buffer keeps -
before prepare_dataset touches value_mean_std, and every optimiser step is the guarded launch, which skips itself - and
every step after it - once the gradient norm is not finite.  The device-resident record says what tripped; the host reads
it once per phase.  This module has no kernel code: the policy values, the tags, the error and the collective verdict.
"""

SPLIT_RANGE_POLICIES = ('warn', 'raise', 'exact')
CHAIN_PRODUCTS = ('auto', 'exact')

# tags of the guard record (the agents' ops.range_scan arrays; TAG_ADAM = RLG_GUARD_TAG_ADAM of include/rlg_hip.h for an
# optimiser step).  ops.py takes the Adam tag and the two limits from here.
TAG_VALUES, TAG_NEGLOGPS, TAG_POLICY, TAG_CRITIC_VALUES, TAG_RETURNS = 1, 2, 3, 4, 5
TAG_ADAM = 0x4144414d
TAG_NAMES = {TAG_VALUES: 'values', TAG_NEGLOGPS: 'neglogps', TAG_POLICY: 'mus / logits',
             TAG_CRITIC_VALUES: 'central value critic values',
             TAG_RETURNS: 'returns (the bootstrap values of the observation behind the last step, or the rewards)',
             TAG_ADAM: 'gradient norm of an optimiser step'}

LIMIT_WEIGHT, LIMIT_HIDDEN = 1023.0, 4094.0


class SplitRangeError(RuntimeError):
    """The range guard tripped: a launch on fp16 plane products produced non-finite values (policy 'raise'), or exact
    fp32 products did as well (policy 'exact': the inputs themselves are not finite).  phase: 'rollout' / 'update';
    tag, index: the guard record - which array and the smallest offending flat index, or TAG_ADAM and the optimiser
    step."""

    def __init__(self, message, phase=None, tag=None, index=None):
        super().__init__(message)
        self.phase, self.tag, self.index = phase, tag, index


def policy_from_config(config):
    """(split_range, chain_products) of a configuration dict; ValueError for anything but the documented values."""
    split_range = config.get('split_range', 'warn')
    products = config.get('chain_products', 'auto')
    if split_range not in SPLIT_RANGE_POLICIES:
        raise ValueError(f'split_range must be one of {SPLIT_RANGE_POLICIES}, got {split_range!r}')
    if products not in CHAIN_PRODUCTS:
        raise ValueError(f'chain_products must be one of {CHAIN_PRODUCTS}, got {products!r}')
    return split_range, products


def describe(phase, tag, index, products):
    """One sentence for the error / the notice: phase, what tripped and where, the two limits."""
    what = TAG_NAMES.get(tag, f'tag {tag}')
    where = f'optimiser step {index}' if tag == TAG_ADAM else f'flat index {index}'
    if products == 'exact':
        return (f'range guard tripped in the {phase}: non-finite {what} ({where}) on exact fp32 products - exact products '
                f'are non-finite too, so the inputs are (the split-fp16 limits |weight| < {LIMIT_WEIGHT:g} and '
                f'|hidden activation| < {LIMIT_HIDDEN:g} do not apply to them)')
    return (f'range guard tripped in the {phase}: non-finite {what} ({where}).  The split-fp16 chain kernels hold '
            f'|weight| < {LIMIT_WEIGHT:g} and |hidden activation| < {LIMIT_HIDDEN:g} (fixed operand scales, '
            f'csrc/bx_form.hpp); chain_products: exact, or split_range: exact, runs on exact fp32 products')


def collective_trip(tripped, device='cpu'):
    """The verdict of all ranks: True on every rank when any rank tripped (one MAX all-reduce, as for the in-graph
    all-reduce's time-out flag), so that every rank takes the same branch in the same epoch.  Needs an initialised
    process group; a single process calls nothing."""
    import torch
    import torch.distributed as dist
    flag = torch.tensor([1.0 if tripped else 0.0], device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    return bool(flag.item() != 0)


def verdict(record, phase, policy, products, multi_gpu, device, read):
    """One host read of a guard record (`read` = ops.read_guard; this module has no kernel bindings) and what follows
    from it, for the agent and for a central value network trained on its own: under multi_gpu the verdict is
    collective.  Clean: None.  Tripped: SplitRangeError under policy 'raise', or when the products are exact already
    (then the inputs are not finite); under policy 'exact' the sentence for the caller's notice - the caller switches
    its chains to exact products and clears the record."""
    tag, index = read(record)
    tripped = tag != 0
    if multi_gpu:
        tripped = collective_trip(tripped, device)
    if not tripped:
        return None
    what = describe(phase, tag, index, products) if tag != 0 else f'range guard tripped in the {phase} on another rank'
    if policy == 'raise' or products == 'exact':
        raise SplitRangeError('rl_games_amd: ' + what, phase, tag, index)
    return what
