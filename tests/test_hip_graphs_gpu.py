"""GPU: rl_games_amd/hip_graphs.py on its own - the capturer, the step-graph cache and the update-graph holder, on tensors
of a handful of elements and bodies of torch's element-wise ops, with no agent (the agents' and players' suites check what
they capture).  Every comparison is bit for bit: a replay runs the kernels the eager body ran.
"""
import gc
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _capturer(optimizer=None):
    from rl_games_amd.hip_graphs import GraphCapturer
    from rl_games_amd.weight_forms import ChainFormSet
    return GraphCapturer(ChainFormSet(), optimizer)


def _body(x):
    return (x * 3.0 + 1.0).sin()


def _values(seed, n=7):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_a_captured_body_replays_what_the_eager_body_gives():
    x, out = _values(0), []
    g = _capturer().capture(lambda: out.append(_body(x)))
    for seed in (1, 2):
        x.copy_(_values(seed))
        g.replay()
        assert torch.equal(out[0], _body(x))


@pytest.mark.parametrize('gc_enabled', [True, False])
def test_a_failed_capture_raises_graph_capture_error_and_puts_everything_back(gc_enabled):
    from rl_games_amd.hip_graphs import GraphCaptureError
    opt = SimpleNamespace(step_count=5, weights_version=9)
    capturer = _capturer(opt)
    x, out = _values(3), []
    error = RuntimeError('raised inside the capture')

    def failing():
        assert torch.cuda.is_current_stream_capturing()
        out.append(_body(x))
        opt.step_count += 1
        opt.weights_version += 1
        raise error

    def advancing():
        out.append(_body(x))
        opt.step_count += 1
        opt.weights_version += 1

    was_enabled = gc.isenabled()
    try:
        gc.enable() if gc_enabled else gc.disable()
        with pytest.raises(GraphCaptureError) as caught:
            capturer.capture(failing)
        assert caught.value.__cause__ is error
        assert not torch.cuda.is_current_stream_capturing()
        assert gc.isenabled() == gc_enabled
        assert (opt.step_count, opt.weights_version) == (5, 9)
        del out[:]
        g = capturer.capture(advancing)                      # the same capturer, the same pool
        assert gc.isenabled() == gc_enabled and (opt.step_count, opt.weights_version) == (5, 9)
    finally:
        gc.enable() if was_enabled else gc.disable()
    x.copy_(_values(4))
    g.replay()
    assert torch.equal(out[0], _body(x))


def _step_body(calls):
    def body(a=None, pair=None, nothing=None):
        calls.append((a, pair, nothing))
        return {'sum': _body(a) + pair[0] * pair[1]}
    return body


def _eager_sum(inputs):
    return _body(inputs['a']) + inputs['pair'][0] * inputs['pair'][1]


def test_step_graphs_stage_inputs_once_per_key_and_hand_back_the_recorded_result():
    from rl_games_amd.hip_graphs import StepGraphs
    graphs, calls = StepGraphs(_capturer()), []
    body = _step_body(calls)
    assert len(graphs) == 0 and not graphs

    def inputs(seed, n=7):
        return {'a': _values(seed, n), 'pair': [_values(seed + 1, n), _values(seed + 2, n)], 'nothing': None}

    first = inputs(10)
    res = graphs.step('k', body, first)
    assert len(calls) == 1 and len(graphs) == 1 and torch.equal(res['sum'], _eager_sum(first))
    a, pair, nothing = calls[0]                              # the statics the body was recorded on
    assert nothing is None and torch.equal(a, first['a']) and all(torch.equal(s, t) for s, t in zip(pair, first['pair']))
    ptrs = [a.data_ptr(), pair[0].data_ptr(), pair[1].data_ptr()]
    assert len(set(ptrs)) == 3
    assert not set(ptrs) & {first['a'].data_ptr(), first['pair'][0].data_ptr(), first['pair'][1].data_ptr()}

    second = inputs(20)
    kept = {k: [t.clone() for t in (v if isinstance(v, list) else [v])] for k, v in second.items() if v is not None}
    again = graphs.step('k', body, second)
    assert again is res and len(calls) == 1 and len(graphs) == 1              # a replay: the body did not run
    assert torch.equal(res['sum'], _eager_sum(second))
    assert [a.data_ptr(), pair[0].data_ptr(), pair[1].data_ptr()] == ptrs     # the statics were allocated once
    assert torch.equal(second['a'], kept['a'][0]) and all(torch.equal(s, t) for s, t in zip(second['pair'], kept['pair']))

    other = inputs(30, n=5)                                  # a second key: its own statics and graph
    res_other = graphs.step('other', body, other)
    assert len(calls) == 2 and len(graphs) == 2 and res_other is not res
    assert calls[1][0].data_ptr() not in ptrs and calls[1][0].shape == (5,)
    assert torch.equal(res_other['sum'], _eager_sum(other))
    assert graphs.step('k', body, first) is res and torch.equal(res['sum'], _eager_sum(first))

    graphs.step('k', body, first, index=1)                   # another step index of the key: a graph on the same statics
    assert len(calls) == 3 and len(graphs) == 3 and calls[2][0].data_ptr() == ptrs[0]

    graphs.clear()
    assert len(graphs) == 0 and not graphs
    res = graphs.step('k', body, second)
    assert len(calls) == 4 and len(graphs) == 1 and torch.equal(res['sum'], _eager_sum(second))


def test_step_graphs_without_inputs_capture_and_replay_a_body_on_the_callers_tensor():
    from rl_games_amd.hip_graphs import StepGraphs
    graphs, x, calls = StepGraphs(_capturer()), _values(40), []

    def body():
        calls.append(None)
        return _body(x)

    res = graphs.step('direct', body)
    assert len(calls) == 1 and len(graphs) == 1 and torch.equal(res, _body(x))
    x.copy_(_values(41))
    assert graphs.step('direct', body) is res and len(calls) == 1 and torch.equal(res, _body(x))


def test_update_graphs_are_forgotten_together_when_the_signature_changes():
    from rl_games_amd.hip_graphs import UpdateGraphs
    graphs = UpdateGraphs()
    assert graphs.signature is None and graphs.minibatch == {} and graphs.optimizer is None and graphs.epoch is None
    graphs.refresh(('ptrs', 0.2, 'auto', True))
    graphs.minibatch[0], graphs.minibatch[1], graphs.optimizer, graphs.epoch = 'mb0', 'mb1', 'opt', 'epoch'
    graphs.norm_state = ('partials', 3)
    graphs.refresh(('ptrs', 0.2, 'auto', True))              # equal: everything stays
    assert graphs.minibatch == {0: 'mb0', 1: 'mb1'} and (graphs.optimizer, graphs.epoch) == ('opt', 'epoch')
    assert graphs.norm_state == ('partials', 3) and graphs.signature == ('ptrs', 0.2, 'auto', True)
    graphs.refresh(('ptrs', 0.2, 'exact', True))
    assert graphs.minibatch == {} and graphs.optimizer is None and graphs.epoch is None and graphs.norm_state is None
    assert graphs.signature == ('ptrs', 0.2, 'exact', True)
    graphs.epoch = 'epoch'
    graphs.clear()                                           # the signature outlives a clear()
    assert graphs.epoch is None and graphs.signature == ('ptrs', 0.2, 'exact', True)
