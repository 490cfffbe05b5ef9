"""The protocol that keeps a fused chain's derived weight copies current, as the ordered trace of launches it issues.

A real ops.MlpChain runs over a recording stand-in for librlg_hip.so (the row thresholds of csrc/mlp_chain.hip: lean
16-row kernels below 8,192 rows, the 64-row split kernels from 8,192 (training pair) / 16,384 (inference)) on CPU
tensors.  Every scenario asserts the FULL trace: which pack launch ran, and which of the forward / backward / step
launches was handed planes or fragments.  Scenarios 1-8 use only names that MlpChain had before weight_forms existed, so
they state that the launch sequence did not move; scenario 9 covers weight_forms.ChainFormSet.
"""
import ctypes

import pytest
import torch

LEAN, PAIR, SPLIT = 4096, 8192, 16384       # lean everywhere | split training pair, lean inference | split everywhere


class _Lib:
    def __init__(self):
        self.trace = []
        self.tag = False                    # scenario 9: every record starts with the chain's layer count

    def _rec(self, n, *what):
        self.trace.append(((n,) if self.tag else ()) + what)
        return 0

    def take(self):
        out, self.trace = self.trace, []
        return out

    # ---- host queries
    def rlg_mlp_chain_prepare(self):
        return 0

    def rlg_mlp_chain_lds_bytes(self, n, ins, outs, groups, direction):
        return 1024

    def rlg_mlp_chain_frags_bytes(self, n, ins, outs, direction):
        return 1024

    def rlg_mlp_chain_planes_bytes(self, n, ins, outs, direction):
        return (256, 256, 512)[direction]

    def rlg_mlp_chain_planes_offset(self, n, ins, outs, direction):
        return 256 * direction

    def rlg_mlp_chain_groups(self, rows, requested, direction):
        if requested:
            return requested
        return 1 if rows < (SPLIT if direction == 0 else PAIR) else 4

    def rlg_mlp_chain_bx_supported(self, n, ins, outs, rows, groups, direction):
        return int(rows >= (SPLIT if direction == 0 else PAIR))

    def rlg_mlp_chain_num_blocks(self, rows, groups):
        return -(-rows // (16 * groups))

    # ---- launches
    def rlg_mlp_chain_pack_planes(self, n, w, ins, outs, direction, out, stream):
        assert out
        return self._rec(n, 'pack_planes', direction)

    def rlg_mlp_chain_pack_frags_both(self, n, w, b, ins, outs, fwd, bwd, stream):
        assert fwd
        return self._rec(n, 'pack_frags')

    # (the launching entries take descriptors by reference: ctypes.byref(d)._obj is d)
    def rlg_mlp_chain_forward(self, net, fwd, launch, stream):
        fwd = fwd._obj
        return self._rec(net._obj.num_layers, 'forward', launch._obj.rows,
                         dict(pack_planes=bool(fwd.pack_backward_planes_or_null), weight_planes=bool(fwd.weight_form_or_null)))

    def rlg_mlp_chain_forward_lean(self, net, fwd, launch, stream):
        return self._rec(net._obj.num_layers, 'forward_lean', launch._obj.rows, dict(frags=bool(fwd._obj.weight_form_or_null)))

    def rlg_mlp_chain_backward(self, net, bwd, launch, stream):
        return self._rec(net._obj.num_layers, 'backward', launch._obj.rows, dict(planes=bool(bwd._obj.weight_form_or_null)))

    def rlg_mlp_chain_backward_lean(self, net, bwd, launch, stream):
        return self._rec(net._obj.num_layers, 'backward_lean', launch._obj.rows, dict(frags=bool(bwd._obj.weight_form_or_null)))

    def rlg_mlp_chain_step(self, net, fwd, bwd, launch, stream):
        return self._rec(net._obj.num_layers, 'step', launch._obj.rows, dict(frags=False))

    def rlg_mlp_chain_step_lean(self, net, fwd, bwd, launch, stream):
        return self._rec(net._obj.num_layers, 'step_lean', launch._obj.rows,
                         dict(frags=bool(fwd._obj.weight_form_or_null) and bool(bwd._obj.weight_form_or_null)))


# what the traces are made of
PACK_FRAGS = ('pack_frags',)


def PACK(direction):
    return ('pack_planes', direction)


def FWD(rows, pack_planes=False, weight_planes=False):
    return ('forward', rows, dict(pack_planes=pack_planes, weight_planes=weight_planes))


def BWD(rows, planes=False):
    return ('backward', rows, dict(planes=planes))


def FWD_LEAN(rows):
    return ('forward_lean', rows, dict(frags=True))


def BWD_LEAN(rows):
    return ('backward_lean', rows, dict(frags=True))


TRAINING = {LEAN: [FWD_LEAN(LEAN), BWD_LEAN(LEAN)],
            PAIR: [FWD(PAIR, weight_planes=True), BWD(PAIR, planes=True)],
            SPLIT: [FWD(SPLIT, weight_planes=True), BWD(SPLIT, planes=True)]}
COLD_PACK = {LEAN: [PACK_FRAGS], PAIR: [PACK(2)], SPLIT: [PACK(2)]}
ROWS = [LEAN, PAIR, SPLIT]


@pytest.fixture
def lib(monkeypatch):
    from rl_games_amd import _lib
    fake = _Lib()
    monkeypatch.setattr(_lib, 'load', lambda: fake)
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, what: None)
    monkeypatch.setattr(_lib, 'stream_handle', lambda device=None: 0)
    return fake


class _Net:
    """An MlpChain of `widths` on CPU tensors whose weights live in a FlatArena, and the tensors of its launches."""

    def __init__(self, widths=(8, 8, 8, 4), versioned=True, products='auto'):
        from rl_games_amd import ops
        from rl_games_amd.flat_optim import FlatArena
        params = []
        for i, o in zip(widths, widths[1:]):
            params += [torch.nn.Parameter(torch.zeros(o, i)), torch.nn.Parameter(torch.zeros(o))]
        self.arena = FlatArena(params)
        n = len(widths) - 1
        layers = [(params[2 * k].data, params[2 * k + 1].data, 'elu' if k < n - 1 else 'None') for k in range(n)]
        self.widths = widths
        self.chain = ops.MlpChain(layers, torch.device('cpu'), weights_version=self.arena.weights_token if versioned else None,
                                  products=products)
        self._tensors = {}

    def tensors(self, rows):
        if rows not in self._tensors:
            w = self.widths
            hidden = lambda: [torch.zeros(rows, o) for o in w[1:-1]]
            self._tensors[rows] = dict(x=torch.zeros(rows, w[0]), heads=torch.zeros(rows, w[-1]), acts=hidden(),
                                       d_heads=torch.zeros(rows, w[-1]), dz=hidden())
        return self._tensors[rows]

    def infer(self, rows, **kw):
        t = self.tensors(rows)
        self.chain.forward(t['x'], t['heads'], **kw)

    def train_forward(self, rows, **kw):
        t = self.tensors(rows)
        self.chain.forward(t['x'], t['heads'], act_out=t['acts'], **kw)

    def backward(self, rows, **kw):
        t = self.tensors(rows)
        self.chain.backward(t['d_heads'], t['acts'], t['dz'], **kw)

    def train(self, rows):
        self.train_forward(rows)
        self.backward(rows)

    def step(self, rows):
        t = self.tensors(rows)
        return self.chain.step(t['x'], t['heads'], t['acts'], t['d_heads'], t['dz'], None, ctypes.c_longlong(0))


# ----------------------------------------------------------------------------- 1, 2: cold start, repeat

@pytest.mark.parametrize('rows', ROWS)
def test_cold_start_packs_in_front_of_the_forward_and_a_repeat_packs_nothing(lib, rows):
    net = _Net()
    net.train(rows)
    assert lib.take() == COLD_PACK[rows] + TRAINING[rows]           # (the backward packs nothing)
    net.train(rows)
    assert lib.take() == TRAINING[rows]
    net.infer(rows)                                                 # (at 8,192 rows the first launch on the fragments)
    net.infer(rows)
    assert lib.take() == {LEAN: [FWD_LEAN(LEAN)] * 2, PAIR: [PACK_FRAGS] + [FWD_LEAN(PAIR)] * 2,
                          SPLIT: [FWD(SPLIT, weight_planes=True)] * 2}[rows]


def test_cold_start_backward_planes_ride_in_an_exact_forward(lib):
    net = _Net()
    net.train_forward(PAIR, split_products=False)
    net.backward(PAIR)
    assert lib.take() == [FWD(PAIR, pack_planes=True), BWD(PAIR, planes=True)]
    # the hand-over is for one backward: the next one packs for itself, and goes on doing so (nothing was stamped)
    net.backward(PAIR)
    net.backward(PAIR)
    assert lib.take() == [PACK(1), BWD(PAIR, planes=True)] * 2


def test_without_a_version_source_every_forward_packs_and_hands_the_backward_its_planes(lib):
    net = _Net(versioned=False)
    for _ in range(2):
        net.train(SPLIT)
        assert lib.take() == [PACK(2)] + TRAINING[SPLIT]
        net.train(LEAN)                                             # (no hand-over between the lean launches)
        assert lib.take() == [PACK_FRAGS, FWD_LEAN(LEAN), PACK_FRAGS, BWD_LEAN(LEAN)]


def test_one_launch_step_reads_the_fragments_and_declines_the_split_sizes(lib):
    net = _Net()
    assert net.step(LEAN) is True and net.step(LEAN) is True
    assert lib.take() == [PACK_FRAGS] + [('step_lean', LEAN, dict(frags=True))] * 2
    assert net.step(PAIR) is False and net.step(SPLIT) is False and lib.take() == []
    net.chain.products = 'exact'
    assert net.step(LEAN) is True and lib.take() == [('step', LEAN, dict(frags=False))]


# ----------------------------------------------------------------------------- 3: weight change

@pytest.mark.parametrize('rows', ROWS)
def test_a_weight_change_costs_one_pack_of_the_form_the_next_launch_reads(lib, rows):
    net = _Net()
    net.train(rows)
    net.infer(rows)
    lib.take()
    net.arena.weights_changed()
    net.infer(rows)
    assert lib.take() == ([PACK_FRAGS, FWD_LEAN(rows)] if rows < SPLIT else [PACK(0), FWD(rows, weight_planes=True)])
    # (a pack of the forward direction alone stamps nothing: the split inference forward packs again)
    net.infer(rows)
    assert lib.take() == ([FWD_LEAN(rows)] if rows < SPLIT else [PACK(0), FWD(rows, weight_planes=True)])
    net.arena.weights_changed()
    net.train(rows)
    assert lib.take() == COLD_PACK[rows] + TRAINING[rows]


# ----------------------------------------------------------------------------- 4: backward after another launch

@pytest.mark.parametrize('versioned', [True, False])
def test_a_backward_whose_forward_was_followed_by_another_launch_packs_for_itself(lib, versioned):
    net = _Net(versioned=versioned)
    net.train_forward(PAIR, split_products=False)                   # (leaves the backward planes, stamps nothing)
    net.infer(LEAN)
    net.backward(PAIR)
    assert lib.take() == [FWD(PAIR, pack_planes=True), PACK_FRAGS, FWD_LEAN(LEAN), PACK(1), BWD(PAIR, planes=True)]
    # ... and so does one for another row count than its forward's
    net.train_forward(PAIR, split_products=False)
    net.backward(SPLIT)
    assert lib.take() == [FWD(PAIR, pack_planes=True), PACK(1), BWD(SPLIT, planes=True)]
    # ... and one behind a weight change
    net.train_forward(PAIR, split_products=False)
    net.arena.weights_changed()
    net.backward(PAIR)
    assert lib.take() == [FWD(PAIR, pack_planes=True)] + ([PACK(1)] if versioned else []) + [BWD(PAIR, planes=True)]


def test_a_split_forward_between_forward_and_backward_without_a_version_source(lib):
    net = _Net(versioned=False)
    net.train_forward(SPLIT)
    net.infer(SPLIT)
    net.backward(SPLIT)
    assert lib.take() == [PACK(2), FWD(SPLIT, weight_planes=True), PACK(0), FWD(SPLIT, weight_planes=True),
                          PACK(1), BWD(SPLIT, planes=True)]


# ----------------------------------------------------------------------------- 5, 6: recorded only

@pytest.mark.parametrize('rows', ROWS)
def test_launches_that_were_only_recorded_do_not_count_as_packed(lib, rows):
    net = _Net()
    state = net.chain.cache_state()
    net.train(rows)
    net.chain.restore_cache_state(state)
    assert lib.take() == COLD_PACK[rows] + TRAINING[rows]
    net.train(rows)
    assert lib.take() == COLD_PACK[rows] + TRAINING[rows]
    # a recording behind real launches: what those left stays
    state = net.chain.cache_state()
    net.arena.weights_changed()
    net.train(rows)
    net.arena.weights_version -= 1                                  # (a capture puts the host mirrors back)
    net.chain.restore_cache_state(state)
    lib.take()
    net.train(rows)
    assert lib.take() == TRAINING[rows]


@pytest.mark.parametrize('rows', ROWS)
def test_a_recording_that_fails_half_way_leaves_nothing_marked(lib, rows):
    net = _Net()

    def body():
        net.train_forward(rows)
        raise RuntimeError('capture failed')

    state = net.chain.cache_state()
    with pytest.raises(RuntimeError):
        try:
            body()
        finally:
            net.chain.restore_cache_state(state)
    assert lib.take() == COLD_PACK[rows] + TRAINING[rows][:1]
    net.backward(rows)                                              # (no hand-over from the forward that never ran)
    assert lib.take() == ([PACK_FRAGS, BWD_LEAN(rows)] if rows == LEAN else [PACK(1), BWD(rows, planes=True)])
    net.train(rows)
    assert lib.take() == ([] if rows == LEAN else [PACK(2)]) + TRAINING[rows]


# ----------------------------------------------------------------------------- 7: mode switch and back

def test_exact_products_pack_nothing_and_pass_no_form_and_the_routes_come_back(lib):
    net = _Net(products='exact')
    exact = [step for rows in ROWS for step in (FWD(rows), BWD(rows), FWD(rows))]

    def everything():
        for rows in ROWS:
            net.train(rows)
            net.infer(rows)

    everything()
    assert lib.take() == exact
    state = net.chain.cache_state()
    assert net.chain._planes is None and net.chain._frags is None and net.chain.adam_pack_target() is None
    net.chain.restore_cache_state(state)
    assert net.chain.products == 'exact'

    net.chain.products = 'auto'
    auto = net.chain.cache_state()
    net.train(PAIR)
    assert lib.take() == COLD_PACK[PAIR] + TRAINING[PAIR]
    net.chain.products = 'exact'
    net.arena.weights_changed()
    everything()
    assert lib.take() == exact
    net.chain.restore_cache_state(auto)
    assert net.chain.products == 'auto'
    everything()
    assert lib.take() == ([PACK_FRAGS] + TRAINING[LEAN] + [FWD_LEAN(LEAN)]
                          + [PACK(2)] + TRAINING[PAIR] + [FWD_LEAN(PAIR)]
                          + TRAINING[SPLIT] + [FWD(SPLIT, weight_planes=True)])
    with pytest.raises(ValueError):
        net.chain.products = 'fp16'


# ----------------------------------------------------------------------------- 8: Adam pack target

def test_adam_pack_target_packs_the_whole_buffer_once(lib):
    from rl_games_amd import ops
    net = _Net()
    target = net.chain.adam_pack_target()
    assert lib.take() == [PACK(2)]
    assert target[0] == 3 and target[4] == net.chain._plane_buffer().data_ptr()
    assert net.chain.adam_pack_target() == target and lib.take() == []
    net.train(SPLIT)                                                # (that pack counts for the weights as they are)
    assert lib.take() == TRAINING[SPLIT]
    net.arena.weights_changed()
    assert net.chain.adam_pack_target() == target and lib.take() == []
    net.train(SPLIT)
    assert lib.take() == [PACK(2)] + TRAINING[SPLIT]
    # pack_planes: the view of the direction, and no claim that anything is current
    net.arena.weights_changed()
    views = [net.chain.pack_planes(d, net.arena.flat_params) for d in (0, 1, 2)]
    assert [v.numel() for v in views] == [256, 256, 512] and views[1].data_ptr() == views[2].data_ptr() + 256
    net.infer(SPLIT)
    assert lib.take() == [PACK(0), PACK(1), PACK(2), PACK(0), FWD(SPLIT, weight_planes=True)]

    assert _Net(products='exact').chain.adam_pack_target() is None
    assert _Net(versioned=False).chain.adam_pack_target() is None
    assert lib.take() == []
    assert ops.MlpChain.PRODUCTS == ('auto', 'exact')


def test_a_full_pack_of_more_jobs_than_one_launch_carries_is_two_launches(lib):
    net = _Net(widths=(8, 8, 8, 8, 8, 4))                           # 5 layers: 2n-1 = 9 jobs
    whole = net.chain.pack_planes(2, net.arena.flat_params)
    assert lib.take() == [PACK(0), PACK(1)] and whole.numel() == 512
    net.chain.adam_pack_target()
    net.train(SPLIT)
    assert lib.take() == [PACK(0), PACK(1)] + TRAINING[SPLIT]


# ----------------------------------------------------------------------------- 9: ChainFormSet

def _form_set(lib, actor_planes=True):
    from rl_games_amd.weight_forms import ChainFormSet, _ChainForms
    lib.tag = True
    actor, critic = _Net(), _Net(widths=(8, 8, 1))                  # 3 and 2 layers: the first field of every record
    forms = ChainFormSet([
        _ChainForms(actor.chain, ((PAIR, 2), (PAIR, 1), (LEAN, 0)), actor.arena.flat_params, True, actor_planes),
        _ChainForms(critic.chain, ((SPLIT, 0),), critic.arena.flat_params)])
    return forms, actor, critic


def test_form_set_brings_the_forms_up_to_date_in_front_of_a_replay(lib):
    forms, actor, critic = _form_set(lib)
    assert forms.lean_chain() is actor.chain and forms.adam_pack_chain() is actor.chain
    assert [f.chain for f in forms] == [actor.chain, critic.chain]
    forms.before_replay()                                           # (an update graph: the actor's chains only)
    assert lib.take() == [(3, 'pack_planes', 2), (3, 'pack_frags')]
    forms.before_replay(rollout=True)
    assert lib.take() == [(2, 'pack_planes', 2)]
    forms.before_replay(rollout=True)
    assert lib.take() == []
    critic.arena.weights_changed()
    forms.before_replay()
    assert lib.take() == []
    forms.before_replay(rollout=True)
    assert lib.take() == [(2, 'pack_planes', 2)]


def test_form_set_leaves_the_planes_of_a_chain_whose_graphs_pack_them_alone(lib):
    forms, actor, critic = _form_set(lib, actor_planes=False)
    assert forms.lean_chain() is actor.chain and forms.adam_pack_chain() is None
    forms.before_replay(rollout=True)
    assert lib.take() == [(3, 'pack_frags'), (2, 'pack_planes', 2)]
    assert actor.chain.planes.holds is None


def test_form_set_after_step_stamps_the_adam_written_planes_and_packs_or_stamps_the_fragments(lib):
    forms, actor, critic = _form_set(lib)
    forms.before_replay(rollout=True)
    lib.take()
    critic_holds = (critic.chain.planes.holds, critic.chain.frags.holds)
    actor.arena.weights_changed()
    forms.after_step(actor.arena)                                   # (the eager step: the pack launch is issued here)
    assert lib.take() == [(3, 'pack_frags')]
    token = actor.arena.weights_token()
    assert actor.chain.planes.holds == token and actor.chain.frags.holds == token
    actor.arena.weights_changed()
    forms.after_step(actor.arena, packed=True)                      # (behind a replayed graph that holds that launch)
    token = actor.arena.weights_token()
    assert lib.take() == [] and actor.chain.planes.holds == token and actor.chain.frags.holds == token
    assert (critic.chain.planes.holds, critic.chain.frags.holds) == critic_holds
    forms.before_replay(rollout=True)
    assert lib.take() == []
    # under exact products nothing reads a form: nothing is packed or stamped
    forms.set_products('exact')
    assert forms.lean_chain() is None and forms.adam_pack_chain() is None
    actor.arena.weights_changed()
    forms.after_step(actor.arena)
    forms.before_replay(rollout=True)
    assert lib.take() == [] and actor.chain.planes.holds == token
    forms.set_products('auto')
    assert forms.lean_chain() is actor.chain and forms.adam_pack_chain() is actor.chain


def test_form_set_capture_restores_every_chain_on_success_and_on_failure(lib):
    forms, actor, critic = _form_set(lib)
    for fails in (False, True):
        before = [c.chain.cache_state() for c in (actor, critic)]
        try:
            with forms.captured():
                actor.train(PAIR)
                critic.infer(SPLIT)
                forms.after_step(actor.arena)
                assert [c.chain.cache_state() for c in (actor, critic)] != before
                if fails:
                    raise RuntimeError('capture failed')
        except RuntimeError:
            assert fails
        assert [c.chain.cache_state() for c in (actor, critic)] == before
        assert lib.take() == [(3, 'pack_planes', 2), (3, 'forward', PAIR, dict(pack_planes=False, weight_planes=True)),
                              (3, 'backward', PAIR, dict(planes=True)), (2, 'pack_planes', 0),
                              (2, 'forward', SPLIT, dict(pack_planes=False, weight_planes=True)), (3, 'pack_frags')]
    assert actor.chain.planes.buffer is not None and actor.chain.frags.buffer is not None
