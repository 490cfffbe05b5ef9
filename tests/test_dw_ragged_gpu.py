"""GPU: csrc/mlp_dw_ragged.hip - the weight gradient dZ^T X for widths off a multiple of 4 (ops.ragged_dw) and its route
through chain_net.WeightGrads - against the fp64 product on the CPU.  Bound as in tests/test_chain_ln_gpu.py: the max-abs
error may be at most the larger of 4 x the error of torch.mm in fp32 on the GPU for the same product and 1e-5 of the
largest |G|; the ratio error / bound is printed per shape (profiles/dw_ragged.txt)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
# (rows, No, Mi): one row, rows off a multiple of 4, one short of / exactly / one past four slices, a last slice of 8 rows,
# 17 workgroups per tile with a last slice of 3 rows; widths of 1 column, below / just past one block, tiles in both dimensions
SHAPES = [(1, 4, 1), (3, 20, 9), (63, 64, 17), (64, 272, 98), (65, 4, 130), (200, 20, 98), (4099, 272, 130), (4099, 64, 9),
          (65, 272, 17), (200, 64, 1), (3, 272, 130), (64, 20, 17)]


def _operands(rows, No, Mi, seed=0):
    """dz, x: the first `rows` rows of buffers whose other rows are NaN; a NaN grad; the NaN workspace of the shape."""
    from rl_games_amd import _lib, ops
    g = torch.Generator().manual_seed(1000 * rows + 10 * No + Mi + seed)
    bufs = []
    for w in (No, Mi):
        b = torch.full((rows + 5, w), NAN)
        b[:rows] = torch.randn(rows, w, generator=g)
        bufs.append(b.to(DEV)[:rows])
    need = _lib.load().rlg_mlp_dw_ragged_workspace(rows, No, Mi)
    ops._ragged_scratch.setdefault((DEV, need), torch.empty(need, device=DEV)).fill_(NAN)     # (in place: graphs hold it)
    return bufs[0], bufs[1], torch.full((No, Mi), NAN, device=DEV)


def _check(got, dz, x, what):
    ref = dz.double().cpu().t() @ x.double().cpu()
    lib_err = (torch.mm(dz.t(), x).double().cpu() - ref).abs().max().item()
    bound = max(4.0 * lib_err, 1e-5 * ref.abs().max().item())
    err = (got.double().cpu() - ref).abs().max().item()
    print(f'{what}: err {err:.3e} torch.mm {lib_err:.3e} ratio {err / bound:.3f}')
    assert err <= bound, (what, err, bound)         # (a NaN fails it)


@pytest.mark.parametrize('rows,No,Mi', SHAPES)
def test_ragged_dw_against_fp64(rows, No, Mi):
    from rl_games_amd import ops
    dz, x, grad = _operands(rows, No, Mi)
    ops.ragged_dw(dz, x, grad)
    _check(grad, dz, x, f'dw_ragged {rows} x {No} x {Mi}')


def test_ragged_dw_is_deterministic_and_replays_from_a_graph():
    from rl_games_amd import ops
    rows, No, Mi = 200, 64, 17
    dz, x, grad = _operands(rows, No, Mi)
    again = torch.empty_like(grad)
    ops.ragged_dw(dz, x, grad)
    ops.ragged_dw(dz, x, again)
    assert torch.equal(grad, again)
    out, graph = torch.empty_like(grad), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ragged_dw(dz, x, out)
    for seed in (1, 2, 3):                            # several replays, each against the eager call on the new inputs
        dz2, x2, _ = _operands(rows, No, Mi, seed)
        dz.copy_(dz2)
        x.copy_(x2)
        graph.replay()
        ops.ragged_dw(dz, x, again)
        assert torch.equal(out, again) and not torch.equal(out, grad)


ROUTE_ROWS = 20480                               # ops.RAGGED_MIN_ROWS: shorter minibatches stay with the library


def _jobs(shapes, rows=ROUTE_ROWS):
    return [_operands(rows, No, Mi) for No, Mi in shapes]


def test_weight_grads_route():
    from rl_games_amd.chain_net import WeightGrads
    jobs = _jobs([(32, 64), (64, 9)])
    wg = WeightGrads()
    wg.finish(jobs, ROUTE_ROWS)
    assert wg.last_dw_library_jobs == 0
    _check(jobs[1][2], jobs[1][0], jobs[1][1], 'route 20480 x 64 x 9')
    for kw, shapes, rows in (({'ragged': False}, [(32, 64), (64, 9)], ROUTE_ROWS), ({}, [(16, 513)], ROUTE_ROWS),
                             ({}, [(64, 9)], ROUTE_ROWS - 1)):
        jobs = _jobs(shapes, rows)
        wg = WeightGrads(**kw)
        wg.finish(jobs, rows)
        assert wg.last_dw_library_jobs == 1
        dz, x, grad = jobs[-1]
        assert torch.equal(grad, torch.mm(dz.t(), x))


def test_envelope():
    from rl_games_amd import _lib, ops
    need = _lib.load().rlg_mlp_dw_ragged_workspace
    for shape, ok in (((1, 1, 1), True), ((1, 1024, 512), True), ((1 << 30, 98, 98), True), ((0, 4, 4), False),
                      ((8, 0, 4), False), ((8, 4, 0), False), ((8, 1025, 4), False), ((8, 4, 513), False),
                      (((1 << 30) + 1, 4, 4), False)):
        assert (need(*shape) > 0) == ok and need(*shape) % max(shape[1] * shape[2], 1) == 0, shape
        # the route also wants the rows from which the kernel is the faster one
        assert ops.ragged_dw_supported(*shape) == (ok and shape[0] >= ROUTE_ROWS), shape
        assert ops.ragged_dw_supported(ROUTE_ROWS, *shape[1:]) == (need(ROUTE_ROWS, *shape[1:]) > 0), shape
    dz, _, grad = _operands(64, 20, 9)
    wide = torch.full((64, 12), NAN, device=DEV)
    with pytest.raises(NotImplementedError):          # a strided x: declined - its NaN never reach grad, nothing does
        ops.ragged_dw(dz, wide[:, :9], grad)
    with pytest.raises(NotImplementedError):          # a base pointer off a 16-byte boundary
        ops.ragged_dw(dz, torch.zeros(64 * 9 + 1, device=DEV)[1:].view(64, 9), grad)
    torch.cuda.synchronize()
    assert torch.isnan(grad).all()
