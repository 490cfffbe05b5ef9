"""GPU: the one-launch weight gradient for widths off a multiple of 4 on minibatches below ops.RAGGED_MIN_ROWS rows
(csrc/mlp_dw_ragged.hip, mlp_dw_ragged_short_kernel; ops.ragged_dw_short), its route through chain_net.WeightGrads and
the agents' `short_ragged_dw` key.  Operands, reference and bound are tests/test_dw_ragged_gpu.py's: NaN rows behind
`rows`, a NaN grad, the fp64 product on the CPU, and max-abs error <= max(4 x torch.mm's error, 1e-5 max|G|); the
ratio is printed (profiles/dw_ragged_short.txt).  The partial tiles of the workspace are NaN in front of every call, the
counter words zero as the contract wants them."""
import copy

import pytest
import torch

from test_dw_ragged_gpu import SHAPES as SIBLING_SHAPES, _check, _operands as _sibling_operands

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
# (rows, No, Mi).  No one past a tile of 32, Mi 1 / 98; two bursts whose second is short (runs of 2 x 44 rows, a last run
# of 84); then the kernel instantiations that only long minibatches reach - tiles of 64 / 128 outputs: <2, 1> at 2 x 2
# waves, <2, 1> and <2, 8> at 4 x 1, <1, 8> (a listed shape).  The rows around a run's end: test_run_edges
SHAPES = SIBLING_SHAPES + [(40, 33, 98), (40, 33, 1), (700, 512, 98), (102500, 33, 1), (103000, 65, 1), (37200, 65, 130),
                           (16384, 400, 105)]
_GUARDED = {}


def _operands(rows, No, Mi, seed=0):
    """The sibling's operands; the workspace ops.ragged_dw_short will use is the front of a larger buffer: counter words
    zero, partial tiles NaN, and NaN behind it for the 15 partials a 16-wide sum could reach past its end."""
    from rl_games_amd import _lib, ops
    dz, x, grad = _sibling_operands(rows, No, Mi, seed)
    need = _lib.load().rlg_mlp_dw_ragged_short_workspace
    floats, counters = need(rows, No, Mi), need(1, 1, 1)     # (one workgroup per tile: the counter words and nothing else)
    if (DEV, floats) not in _GUARDED:                         # (once: a captured graph holds the address)
        behind = min(15 * (floats - counters), 15 << 19)     # (15 partials of any shape with this many floats)
        _GUARDED[DEV, floats] = torch.zeros(floats + behind, device=DEV)
        ops._ragged_short_scratch[DEV, floats] = _GUARDED[DEV, floats][:floats]
    _GUARDED[DEV, floats][counters:].fill_(NAN)
    return dz, x, grad


@pytest.mark.parametrize('rows,No,Mi', SHAPES)
def test_ragged_dw_short_against_fp64(rows, No, Mi):
    from rl_games_amd import ops
    dz, x, grad = _operands(rows, No, Mi)
    ops.ragged_dw_short(dz, x, grad)
    _check(grad, dz, x, f'dw_ragged_short {rows} x {No} x {Mi}')


@pytest.mark.parametrize('runs,more', [(1, -1), (1, 0), (1, 1), (2, 3)])
def test_run_edges(runs, more):
    """R - 1, R, R + 1 and 2 R + 3 rows at 64 x 17, R the shipped plan's run there: the most rows that one workgroup per
    tile covers (a workspace of counter words only); one row more gives every tile exactly two."""
    from rl_games_amd import _lib, ops
    need = _lib.load().rlg_mlp_dw_ragged_short_workspace
    No, Mi = 64, 17
    R = max(r for r in range(1, 256) if need(r, No, Mi) == need(1, 1, 1))
    assert R % 4 == 0 and need(R + 1, No, Mi) == need(1, 1, 1) + 2 * No * Mi
    rows = runs * R + more
    dz, x, grad = _operands(rows, No, Mi)
    ops.ragged_dw_short(dz, x, grad)
    _check(grad, dz, x, f'dw_ragged_short {rows} x {No} x {Mi} (R = {R})')


def test_deterministic_counters_reset_and_graph_replays():
    from rl_games_amd import ops
    rows, No, Mi = 200, 64, 17                       # 13 workgroups for each of 2 tiles
    dz, x, grad = _operands(rows, No, Mi)
    again = torch.empty_like(grad)
    ops.ragged_dw_short(dz, x, grad)
    ops.ragged_dw_short(dz, x, again)
    assert torch.equal(grad, again)
    out, graph = torch.empty_like(grad), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ragged_dw_short(dz, x, out)
    for seed in (1, 2, 3):                            # a counter left off zero or a stale partial shows here
        dz2, x2, _ = _operands(rows, No, Mi, seed)
        dz.copy_(dz2)
        x.copy_(x2)
        graph.replay()
        ops.ragged_dw_short(dz, x, again)
        assert torch.equal(out, again) and not torch.equal(out, grad)


@pytest.mark.parametrize('rows', [256, 20479])
def test_weight_grads_route(rows):
    from rl_games_amd.chain_net import WeightGrads
    for kw, library in (({'ragged_short': True}, 0), ({}, 1)):
        jobs = [_operands(rows, No, Mi) for No, Mi in [(32, 64), (64, 9)]]
        wg = WeightGrads(**kw)
        wg.finish(jobs, rows)
        assert wg.last_dw_library_jobs == library
        _check(jobs[1][2], jobs[1][0], jobs[1][1], f'route {kw} {rows} x 64 x 9')


def test_envelope():
    from rl_games_amd import _lib, ops
    need = _lib.load().rlg_mlp_dw_ragged_short_workspace
    assert need(8, 1025, 4) == 0 and need(8, 4, 513) == 0 and need(8, 1024, 512) > 0
    dz, _, grad = _operands(64, 20, 9)
    wide = torch.full((64, 12), NAN, device=DEV)
    with pytest.raises(NotImplementedError):          # a strided x
        ops.ragged_dw_short(dz, wide[:, :9], grad)
    with pytest.raises(NotImplementedError):          # a base pointer off a 16-byte boundary
        ops.ragged_dw_short(dz, torch.zeros(64 * 9 + 1, device=DEV)[1:].view(64, 9), grad)
    torch.cuda.synchronize()
    assert torch.isnan(grad).all()


def test_short_ragged_dw_key_keeps_an_update_off_the_library():
    """A discrete agent over 9 observations, 64 envs x horizon 8, minibatch 256: with the key no first-layer gradient of
    an epoch is a library product; the parameters after the epoch agree with the default route's as two product orders
    of one update do in tests/test_chain_ln_agent_gpu.py (_close: 1e-5 of the tensor's largest magnitude)."""
    from rl_games_amd import configs
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    from test_chain_ln_agent_gpu import _close
    flats = []
    for over, library in (({'short_ragged_dw': True}, 0), ({}, 1)):
        params = configs.cartpole_discrete(num_actors=64, normalize_input=True, normalize_value=True, horizon_length=8,
                                           minibatch_size=256, **over)
        params['network']['mlp']['units'] = [32, 16]
        params['config']['env_config'].update(obs_dim=9, discrete_actions=4, autoreset_mode='same_step')
        torch.manual_seed(4)
        agent = DiscreteA2CAgent('short_ragged_dw', copy.deepcopy(params))
        agent.init_tensors()
        agent.obs = agent.env_reset()
        agent.update_epoch()
        agent.train_epoch()
        assert agent._path.engines and all(e.weight_grads.last_dw_library_jobs == library for e in agent._path.engines)
        flats.append({n: p.detach().clone() for n, p in agent.model.named_parameters()})
    for n in flats[1]:
        _close(n, flats[0][n], flats[1][n])
