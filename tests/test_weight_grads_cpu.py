"""CPU: chain_net.WeightGrads.finish - the host code between a backward launch and the optimiser that ManualMLP, ChainNet
and RecurrentChainNet share - with every launch it can issue replaced by a recorder: which (dZ, X, grad) products go
into the MFMA launch and in which order, which plans are built and kept, which column sums and loss partials the
finalise launch takes, and what is left to the library or the narrow kernel.
"""
import types

import pytest
import torch

ROWS = 96


class _Plan:
    """Stands in for ops.MlpDwPlan: records its constructions and launches."""
    built = []
    decline = False

    def __init__(self, shapes, rows, device):
        _Plan.built.append((list(shapes), rows))
        if _Plan.decline:
            raise NotImplementedError('declined')
        self.launches = []

    def finalize_blocks(self, colsums=(), loss_finalize=None):
        return 10 + len(colsums)

    def launch(self, jobs, colsums=(), loss_finalize=None, norm=None, maxima=None):
        self.launches.append(types.SimpleNamespace(jobs=list(jobs), colsums=list(colsums), loss_finalize=loss_finalize,
                                                   norm=norm, maxima=maxima))
        return self.finalize_blocks(colsums, loss_finalize)


@pytest.fixture
def rec(monkeypatch):
    from rl_games_amd import ops
    calls = types.SimpleNamespace(colsum=[], narrow=[], loss=[], mm=[])
    _Plan.built, _Plan.decline = [], False
    real_mm = torch.mm

    def mm(a, b, out=None):
        calls.mm.append(out)
        return real_mm(a, b, out=out)
    monkeypatch.setattr(ops, 'MlpDwPlan', _Plan)
    monkeypatch.setattr(ops, 'colsum_finalize', lambda part, nb, cols, out: calls.colsum.append(out))
    monkeypatch.setattr(ops, 'narrow_dw', lambda dz, x, g: calls.narrow.append(g))
    monkeypatch.setattr(ops, 'ppo_loss_finalize_from', lambda desc, device: calls.loss.append(desc))
    monkeypatch.setattr(torch, 'mm', mm)
    return calls


def _job(no, mi, layer=None):
    job = (torch.randn(ROWS, no), torch.randn(ROWS, mi), torch.full((no, mi), float('nan')))
    return job if layer is None else job + (layer,)


def _colsum(cols):
    return (torch.zeros(2 * cols, dtype=torch.float64), 2, cols, torch.empty(cols))


def _is(a, b):
    return len(a) == len(b) and all(p is q for p, q in zip(a, b))


def _finisher(**kw):
    from rl_games_amd.chain_net import WeightGrads
    return WeightGrads(**kw)


def test_fast_jobs_are_one_launch_heaviest_first_on_a_plan_kept_per_shape_key(rec):
    wg = _finisher()
    jobs = [_job(4, 32), _job(32, 64), _job(64, 12)]            # 128, 2048, 768 elements
    colsums = [_colsum(32), _colsum(64)]
    assert wg.finish(jobs, ROWS, colsums) is None
    assert _Plan.built == [([(32, 64), (64, 12), (4, 32)], ROWS)]
    _, plan, mx = wg.last_dw_jobs
    assert mx is None and len(plan.launches) == 1
    launch = plan.launches[0]
    assert [_is(got, want) for got, want in zip(launch.jobs, (jobs[1], jobs[2], jobs[0]))] == [True] * 3
    assert _is([c[3] for c in launch.colsums], [c[3] for c in colsums])
    assert launch.loss_finalize is None and launch.norm is None and launch.maxima is None
    assert wg.last_dw_path == 'mfma' and wg.last_dw_library_jobs == 0
    assert not (rec.mm or rec.narrow or rec.colsum or rec.loss)
    wg.finish(jobs, ROWS, colsums)                              # the plan is reused
    assert len(_Plan.built) == 1 and wg.last_dw_jobs[1] is plan and len(plan.launches) == 2
    wg.finish(jobs[:2], ROWS, colsums)                          # other shapes: another plan
    assert len(_Plan.built) == 2 and wg.last_dw_jobs[1] is not plan


def test_a_job_over_9_input_columns_is_a_library_product(rec):
    wg = _finisher(narrow=False)
    jobs = [_job(32, 64), _job(64, 9)]
    wg.finish(jobs, ROWS, [_colsum(32)])
    assert _Plan.built == [([(32, 64)], ROWS)]
    assert _is(wg.last_dw_jobs[1].launches[0].jobs[0], jobs[0])
    assert _is(rec.mm, [jobs[1][2]]) and not rec.narrow
    assert wg.last_dw_path == 'mfma' and wg.last_dw_library_jobs == 1
    assert torch.equal(jobs[1][2], jobs[1][0].t() @ jobs[1][1])


@pytest.mark.parametrize('narrow', [True, False])
def test_a_job_over_3_input_columns_goes_to_the_narrow_kernel_only_where_asked(rec, narrow):
    wg = _finisher(narrow=narrow)
    jobs = [_job(32, 64), _job(64, 3)]
    wg.finish(jobs, ROWS)
    if narrow:
        assert _is(rec.narrow, [jobs[1][2]]) and not rec.mm and wg.last_dw_library_jobs == 0
    else:
        assert _is(rec.mm, [jobs[1][2]]) and not rec.narrow and wg.last_dw_library_jobs == 1
    assert wg.last_dw_path == 'mfma'


def test_the_narrow_kernel_keeps_its_shape_rule(rec):
    wg = _finisher(narrow=True)
    jobs = [_job(257, 3), _job(64, 9)]                          # more than 256 outputs / more than 8 input columns
    wg.finish(jobs, ROWS)
    assert not rec.narrow and _is(rec.mm, [j[2] for j in jobs]) and wg.last_dw_library_jobs == 2


def test_nine_fast_jobs_are_past_the_launch_and_all_go_to_the_library(rec):
    wg = _finisher()
    jobs = [_job(8, 16) for _ in range(9)]
    colsums = [_colsum(8) for _ in range(9)]
    assert wg.finish(jobs, ROWS, colsums) is None
    assert _Plan.built == [] and wg.last_dw_jobs is None
    assert _is(rec.mm, [j[2] for j in jobs]) and _is(rec.colsum, [c[3] for c in colsums])
    assert wg.last_dw_path == 'library' and wg.last_dw_library_jobs == 9


def test_eight_column_sums_ride_in_the_launch_and_the_rest_are_finalised_singly(rec):
    wg = _finisher()
    jobs = [_job(8, 16) for _ in range(8)]
    colsums = [_colsum(8) for _ in range(10)]
    wg.finish(jobs, ROWS, colsums)
    launch = wg.last_dw_jobs[1].launches[0]
    assert len(launch.jobs) == 8 and _is([c[3] for c in launch.colsums], [c[3] for c in colsums[:8]])
    assert _is(rec.colsum, [c[3] for c in colsums[8:]]) and not rec.mm
    assert wg.last_dw_path == 'mfma'


def test_a_declined_plan_is_remembered_and_the_library_takes_over(rec):
    _Plan.decline = True
    wg = _finisher()
    jobs = [_job(32, 64), _job(64, 12)]
    colsums = [_colsum(32)]
    for _ in range(2):
        rec.mm.clear(), rec.colsum.clear()
        assert wg.finish(jobs, ROWS, colsums, norm=(torch.zeros(64, dtype=torch.float64), 1.0, None)) is None
        assert _is(rec.mm, [j[2] for j in jobs]) and _is(rec.colsum, [colsums[0][3]])
        assert wg.last_dw_path == 'library' and wg.last_dw_library_jobs == 2 and wg.last_dw_jobs is None
    assert len(_Plan.built) == 1                                # no second construction


def test_mfma_off_sends_everything_the_slow_way(rec):
    wg = _finisher(mfma=False, narrow=True)
    jobs = [_job(32, 64), _job(64, 3)]
    colsums = [_colsum(32)]
    wg.finish(jobs, ROWS, colsums)
    assert _Plan.built == [] and _is(rec.mm, [jobs[0][2]]) and _is(rec.narrow, [jobs[1][2]])
    assert _is(rec.colsum, [colsums[0][3]]) and wg.last_dw_path == 'library' and wg.last_dw_library_jobs == 1


def test_loss_finalize_is_folded_into_the_launch_or_launched_on_its_own(rec):
    desc = object()
    wg = _finisher()
    wg.finish([_job(32, 64)], ROWS, [_colsum(32)], loss_finalize=desc)
    assert wg.last_dw_jobs[1].launches[0].loss_finalize is desc and not rec.loss
    wg = _finisher(mfma=False)
    wg.finish([_job(32, 64)], ROWS, [_colsum(32)], loss_finalize=desc)
    assert rec.loss == [desc]


def test_norm_is_passed_on_only_when_the_launch_writes_every_gradient(rec):
    desc = object()
    jobs, colsums = [_job(32, 64), _job(64, 12)], [_colsum(32), _colsum(64)]
    need = 10 + len(colsums)                                    # (_Plan.finalize_blocks)

    def run(jobs, partials, loss_finalize=desc):
        wg = _finisher()
        norm = (torch.zeros(partials, dtype=torch.float64), 0.5, torch.zeros(1, dtype=torch.int64))
        got = wg.finish(jobs, ROWS, colsums, loss_finalize, norm)
        return got, wg.last_dw_jobs[1].launches[0].norm, norm

    got, passed, norm = run(jobs, need)
    assert got == need and passed is norm
    got, passed, _ = run(jobs, need - 1)                        # too few partials for the finalise grid
    assert got is None and passed is None
    got, passed, _ = run(jobs + [_job(64, 9)], need)            # one gradient comes from the library
    assert got is None and passed is None
    got, passed, _ = run(jobs, need, loss_finalize=None)        # the head bias gradients come from elsewhere
    assert got is None and passed is None


def test_maxima_go_with_jobs_that_all_name_their_layer(rec):
    from rl_games_amd import ops
    entries = torch.zeros(8, 4)
    wg = _finisher()
    wg.finish([_job(4, 32), _job(32, 64), _job(64, 12)], ROWS, maxima=(entries, 16))
    assert wg.last_dw_jobs[2] is None and wg.last_dw_jobs[1].launches[0].maxima is None
    wg = _finisher()
    jobs = [_job(4, 32, 2), _job(32, 64, 1), _job(64, 12, 0)]
    wg.finish(jobs, ROWS, maxima=(entries, 16))
    triples, plan, mx = wg.last_dw_jobs
    assert plan.launches[0].maxima is mx and all(len(t) == 3 for t in triples)
    assert mx[0] is entries and mx[1] == [1, 0, 2] and mx[3] == 16           # (heaviest first)
    assert mx[2] == [ops.SPLIT_SCALE_HIDDEN, ops.SPLIT_SCALE_OBS_NORM, ops.SPLIT_SCALE_HIDDEN]
    wg = _finisher()
    wg.finish(jobs, ROWS, maxima=None)
    assert wg.last_dw_jobs[2] is None
