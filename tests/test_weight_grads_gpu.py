"""GPU: the weight-gradient launch (csrc/mlp_dw.hip), bit for bit, at every edge of its schedule.

With small-integer operands every product and every partial sum of dZ^T X is exactly representable in fp32, and every
bf16 or fp16 plane split is exact (the values have two or three significant bits).  All three product forms - exact f32,
six bf16 plane products, three fp16 plane products under per-wave scales - must then return the BITS of the fp64 product,
whatever the tiling, the summation order, the K-split or the pipeline state: a dropped or doubled row, a misplaced
fragment, a column that should have been clamped, a wrong slice in the finalise or a wrong scale entry gives other bits.
No tolerance anywhere but in the last test, which judges real-valued operands with the project's own criterion.

The cases (rows, target_blocks) and the eight layer shapes come from tests/test_dw_schedule_cpu.py, whose host mirror of
the schedule proves that they reach every tile template, pipeline state, ragged end and K-split; its owner_of() names
the tile and the rows behind an element that differs here.
"""
import pytest
import torch

from test_dw_schedule_cpu import BIG, DW_CASES, DW_SHAPES, case_ksplits

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
SENTINEL = -7.75e11               # round the gradients; no sum of the tests comes near it
HUGE = 3e38                       # table entries no wave may read: its rows would be scaled to nothing (fmaxf drops a NaN)
E_LAYER = [0, 7, 20, 30, 3, 12, 25, 16]       # dz of layer l is a multiple of 2^-(4 + E_LAYER[l]); all at least 2^3 apart
PAD = 4                           # poisoned rows in front of and behind the operands: 4 rows keep any width 16-byte aligned
FORMS = ('exact', 'bf16', 'fp16')


def _ops():
    from rl_games_amd import ops
    return ops


def _id(case):
    rows, tb = case
    return f'{rows}-{"default" if tb is None else "k8" if tb == 1 else "big"}'


def _placed(values, offset=None):
    """`values` [rows, cols] as a view with NaN around it: rows [PAD : PAD + rows] of a larger matrix, or - offset given -
    a run of a flat buffer that starts `offset` floats behind a 16-byte boundary."""
    rows, cols = values.shape
    if offset is None:
        buf = torch.full((rows + 2 * PAD, cols), NAN, device=DEV)
        view = buf[PAD:PAD + rows]
        assert view.data_ptr() % 16 == 0
    else:
        buf = torch.full((rows * cols + 8,), NAN, device=DEV)
        view = buf[offset:offset + rows * cols].view(rows, cols)
        assert view.data_ptr() % 16 == 4 * offset
    view.copy_(values)
    return view


def _integer_operands(rows, per, shapes, seed, offset=None):
    """Per layer (dz, x, block maxima of |dz|, fp64 product): x integer in [-7, 7]; dz = m 2^-s 2^-e with integer m in
    [-3, 3], s in 0..4 drawn per block of `per` rows, e per layer; every seventh block of rows all zero."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nblk = -(-rows // per)
    out = []
    for l, (No, Mi) in enumerate(shapes):
        e = E_LAYER[l]
        x = torch.randint(-7, 8, (rows, Mi), generator=g, device=DEV).float()
        m = torch.randint(-3, 4, (rows, No), generator=g, device=DEV).float()
        s = torch.randint(0, 5, (nblk,), generator=g, device=DEV).float()
        block = torch.exp2(-s - e)
        block[6::7] = 0.0
        dz = m * block.repeat_interleave(per)[:rows, None]
        padded = torch.zeros(nblk * per, No, device=DEV)
        padded[:rows] = dz.abs()
        maxima = padded.view(nblk, per * No).max(dim=1).values
        ref = dz.double().t() @ x.double()
        # the premise: in units of 2^-(4 + e) every product is an integer and the sum of their magnitudes - so every
        # partial sum in any order - stays below 2^24: fp32 adds them without rounding
        unit = 2.0 ** (4 + e)
        assert (dz.abs().double().t() @ x.abs().double()).max().item() * unit < 2 ** 24
        assert torch.equal((ref * unit).round(), ref * unit) and torch.equal(ref.float().double(), ref)
        assert (x.abs().max().item() * 4096) < 65504
        out.append((_placed(dz, offset), _placed(x, offset), maxima, ref))
    return out


class _Grads:
    """The gradients of one launch as 16-byte aligned runs of one buffer, sentinels between and around them."""

    def __init__(self, shapes):
        sizes = [No * Mi for No, Mi in shapes]
        assert all(n % 4 == 0 for n in sizes)
        self.buf = torch.full((sum(sizes) + 8 * (len(sizes) + 1),), SENTINEL, device=DEV)
        self.guard = torch.ones_like(self.buf, dtype=torch.bool)
        self.views, at = [], 8
        for (No, Mi), n in zip(shapes, sizes):
            self.views.append(self.buf[at:at + n].view(No, Mi))
            assert self.views[-1].data_ptr() % 16 == 0
            self.guard[at:at + n] = False
            at += n + 8

    def reset(self):
        for v in self.views:
            v.fill_(NAN)

    def check_guard(self):
        assert (self.buf[self.guard] == SENTINEL).all(), 'the launch wrote outside the gradients'

    def untouched(self):
        return all(torch.isnan(v).all() for v in self.views)


def _table(maxima, slots, ncol):
    """[8, ncol] gradient maxima: row slots[l] = the block maxima of layer l, every other row HUGE."""
    entries = torch.full((8, ncol), HUGE, device=DEV)
    for m, slot in zip(maxima, slots):
        assert m.numel() == ncol
        entries[slot] = m
    return entries


def _launch(plan, jobs, grads, form, maxima=None, **kw):
    for w in plan.workspaces:
        w.fill_(NAN)
    grads.reset()
    n = plan.launch([(dz, x, gv) for (dz, x), gv in zip(jobs, grads.views)], maxima=maxima, form=form, **kw)
    torch.cuda.synchronize()
    grads.check_guard()
    return n


def _check_bits(grads, refs, what):
    for l, (gv, ref) in enumerate(zip(grads.views, refs)):
        if not torch.equal(gv.double(), ref):
            bad = (gv.double() != ref).nonzero()
            o, i = bad[0].tolist()
            raise AssertionError(f'{what}: layer {l} {tuple(ref.shape)}: {len(bad)} elements differ, the first at '
                                 f'[{o}, {i}]: {gv[o, i].item()!r} for {ref[o, i].item()!r}')


# ----------------------------------------------------------------------------- a, b: integer operands, poisoned surroundings

@pytest.mark.parametrize('per', [64, 16])
@pytest.mark.parametrize('case', DW_CASES, ids=_id)
def test_every_form_returns_the_bits_of_the_fp64_product(case, per):
    """Exactness: with x integer in [-7, 7] and dz = m 2^-s 2^-e, |m| <= 3, s <= 4, every product is an integer multiple
    of 2^-(4+e) and the magnitudes of a column pair's products sum to at most 21 * 16 * rows <= 5.8e6 < 2^24 such units
    (rows <= 17,024): every partial sum is exact in fp32 in any order, each operand is its own first bf16 / fp16 plane
    (7 * 4096 < 65,504), and the per-wave scales and the layers' 2^-e are powers of two.  _integer_operands asserts this
    on the operands before any kernel runs.  All eight layers go into one launch (a full descriptor table; every other
    case in reverse order), dz and x are row slices with NaN rows before and behind, the gradients lie between
    sentinels, the split-K workspaces are NaN before every launch, the fp16 form's table of maxima has exactly
    ceil(rows / per) columns and the layers' rows of it are permuted.  One plan serves the three forms and a repeat."""
    ops = _ops()
    rows, tb = case
    order = list(range(8)) if DW_CASES.index(case) % 2 == 0 else list(reversed(range(8)))
    shapes = [DW_SHAPES[k] for k in order]
    data = _integer_operands(rows, per, shapes, seed=rows * 131 + per)
    jobs, refs = [d[:2] for d in data], [d[3] for d in data]
    plan = ops.MlpDwPlan(shapes, rows, DEV, target_blocks=tb)
    assert [plan.plan(k)[3] for k in range(8)] == [case_ksplits(rows, tb)[k] for k in order]
    slots = [(3 * l + 1) % 8 for l in range(8)]
    entries = _table([d[2] for d in data], slots, -(-rows // per))
    xscale = [ops.SPLIT_SCALE_OBS_NORM if l == 1 else ops.SPLIT_SCALE_HIDDEN for l in range(8)]
    grads = _Grads(shapes)
    for form in FORMS + ('fp16',):
        before = entries.clone()
        _launch(plan, jobs, grads, form, maxima=(entries, slots, xscale, per) if form == 'fp16' else None)
        _check_bits(grads, refs, f'{form}, per {per}')
        assert torch.equal(entries, before)


@pytest.mark.parametrize('per', [64, 16])
@pytest.mark.parametrize('case', [(515, None), (8192, BIG)], ids=_id)
def test_fp16_form_reads_its_own_rows_of_the_table_only(case, per):
    """Three layers whose maxima are rows 5, 0 and 6 of the table; the other five rows hold 3e38 - a wave that took its
    scale from one of them would scale its rows to nothing."""
    ops = _ops()
    rows, tb = case
    shapes = [DW_SHAPES[5], DW_SHAPES[0], DW_SHAPES[4]]
    data = _integer_operands(rows, per, shapes, seed=rows + per)
    plan = ops.MlpDwPlan(shapes, rows, DEV, target_blocks=tb)
    slots = [5, 0, 6]
    entries = _table([d[2] for d in data], slots, -(-rows // per))
    assert (entries == HUGE).all(dim=1).sum().item() == 5
    grads = _Grads(shapes)
    xscale = [ops.SPLIT_SCALE_HIDDEN, ops.SPLIT_SCALE_OBS_NORM, ops.SPLIT_SCALE_HIDDEN]
    _launch(plan, [d[:2] for d in data], grads, 'fp16', maxima=(entries, slots, xscale, per))
    _check_bits(grads, [d[3] for d in data], f'fp16, per {per}')


# ----------------------------------------------------------------------------- c: operand alignment, the envelope

NARROW = [s if s != (130, 260) else (130, 256) for s in DW_SHAPES]      # 16 tiles of 16 columns are the most


@pytest.mark.parametrize('offset', [2, 1], ids=['8-byte', '4-byte'])
@pytest.mark.parametrize('form', FORMS)
def test_operands_at_8_and_4_byte_aligned_addresses(form, offset):
    """The launch re-tiles from the operand addresses (dw_max_b): 8-byte aligned operands are read two floats per lane
    in tiles of at most 32 columns, 4-byte aligned ones one float per lane in tiles of 16.  Same bits."""
    ops = _ops()
    rows, per = 515, 64
    shapes = DW_SHAPES if offset == 2 else NARROW
    data = _integer_operands(rows, per, shapes, seed=offset, offset=offset)
    plan = ops.MlpDwPlan(shapes, rows, DEV)
    slots = [(3 * l + 1) % 8 for l in range(8)]
    entries = _table([d[2] for d in data], slots, -(-rows // per))
    xscale = [ops.SPLIT_SCALE_HIDDEN] * 8
    grads = _Grads(shapes)
    _launch(plan, [d[:2] for d in data], grads, form, maxima=(entries, slots, xscale, per) if form == 'fp16' else None)
    _check_bits(grads, [d[3] for d in data], f'{form}, operands {4 * offset} bytes behind a 16-byte boundary')


def test_a_width_above_256_at_a_4_byte_aligned_address_is_refused():
    from rl_games_amd._lib import HipLibraryError
    ops = _ops()
    rows = 257
    data = _integer_operands(rows, 64, DW_SHAPES, seed=9, offset=1)
    plan = ops.MlpDwPlan(DW_SHAPES, rows, DEV)
    grads = _Grads(DW_SHAPES)
    for form in ('exact', 'bf16'):
        with pytest.raises(HipLibraryError):
            _launch(plan, [d[:2] for d in data], grads, form)
        torch.cuda.synchronize()
        grads.check_guard()
        assert grads.untouched()


def test_the_envelope_of_the_plan():
    ops = _ops()
    rows = 257
    for shape in ((1028, 4), (257, 4)):
        with pytest.raises(NotImplementedError):
            ops.MlpDwPlan([shape], rows, DEV)
    shapes = [(1024, 4)]
    data = _integer_operands(rows, 64, shapes, seed=10)
    plan = ops.MlpDwPlan(shapes, rows, DEV)
    assert plan.plan(0)[1:3] == (16, 1)
    grads = _Grads(shapes)
    entries = _table([data[0][2]], [2], -(-rows // 64))
    for form in FORMS:
        _launch(plan, [data[0][:2]], grads, form, maxima=(entries, [2], [ops.SPLIT_SCALE_HIDDEN], 64) if form == 'fp16' else None)
        _check_bits(grads, [data[0][3]], form)


# ----------------------------------------------------------------------------- d: the fp16 form without usable maxima

@pytest.mark.parametrize('rows,per', [(515, 64), (515, 16), (4096, 64)])
def test_fp16_form_refuses_a_table_that_is_one_column_short(rows, per):
    from rl_games_amd._lib import HipLibraryError
    ops = _ops()
    shapes = DW_SHAPES[:3]
    data = _integer_operands(rows, per, shapes, seed=11)
    plan = ops.MlpDwPlan(shapes, rows, DEV)
    grads = _Grads(shapes)
    ncol = -(-rows // per)
    entries = _table([d[2] for d in data], [0, 1, 2], ncol)[:, :ncol - 1].contiguous()
    with pytest.raises(HipLibraryError):
        _launch(plan, [d[:2] for d in data], grads, 'fp16', maxima=(entries, [0, 1, 2], [ops.SPLIT_SCALE_HIDDEN] * 3, per))
    torch.cuda.synchronize()
    grads.check_guard()
    assert grads.untouched()
    # (the refused request is spent: the next launch does not find it)
    _launch(plan, [d[:2] for d in data], grads, None)
    _check_bits(grads, [d[3] for d in data], 'after the refusal')


# ----------------------------------------------------------------------------- e: what the finalise launch adds

CS_WIDTHS = (400, 22, 7, 1)


def _colsum_items(nblocks, seed):
    """Integer-valued fp64 partials [nblocks, width] with NaN behind them, outputs between sentinels."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.full((sum(CS_WIDTHS) + 4 * (len(CS_WIDTHS) + 1),), SENTINEL, device=DEV)
    guard = torch.ones_like(out, dtype=torch.bool)
    items, want, at = [], [], 4
    for w in CS_WIDTHS:
        buf = torch.full((nblocks * w + 2 * w + 3,), NAN, dtype=torch.float64, device=DEV)
        part = buf[:nblocks * w]
        part.copy_(torch.randint(-1000, 1001, (nblocks * w,), generator=g, device=DEV).double())
        o = out[at:at + w]
        o.fill_(NAN)
        guard[at:at + w] = False
        at += w + 4
        items.append((part, nblocks, w, o))
        want.append(part.view(nblocks, w).sum(0))
    return items, want, out, guard


@pytest.mark.parametrize('nblocks', [1, 15, 16, 17, 127, 128, 129])
def test_finalise_sums_the_bias_partials_exactly(nblocks):
    """Bias gradients = column sums of per-block fp64 partials, 16 row slices per column and, from 113 blocks on, eight
    loads in flight: integer partials (|sum| <= 129,000 < 2^24) give exact fp32 sums.  The gradients of the same launch
    and the sums of (0.5 g)^2 it leaves per finalise block are exact as well: with integer dz every gradient is an integer
    below 2^24, a square of half of it a multiple of 1/4 below 2^46, and all of them together stay below 2^53 quarters."""
    ops = _ops()
    rows = 515
    shapes = [DW_SHAPES[0], DW_SHAPES[4], DW_SHAPES[6]]
    data = _integer_operands(rows, rows, shapes, seed=nblocks)          # one block of rows: s is one number per layer
    unscale = [2.0 ** (E_LAYER[l] + 4) for l in range(3)]
    jobs = [(_placed(dz * u), x) for (dz, x, _, _), u in zip(data, unscale)]
    refs = [d[3] * u for d, u in zip(data, unscale)]
    items, want, out, guard = _colsum_items(nblocks, seed=nblocks)
    plan = ops.MlpDwPlan(shapes, rows, DEV)
    grads = _Grads(shapes)
    nfin = plan.finalize_blocks(items)
    partials = torch.full((nfin + 5,), NAN, dtype=torch.float64, device=DEV)
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    n = _launch(plan, jobs, grads, 'exact', colsums=items, norm=(partials, 0.5, counter))
    _check_bits(grads, refs, 'with column sums and the norm')
    assert (out[guard] == SENTINEL).all()
    for (part, _, w, o), t in zip(items, want):
        assert t.abs().max().item() < 2 ** 24 and torch.equal(o.double(), t), w
    assert n == nfin and counter.item() == 42
    assert torch.isnan(partials[n:]).all() and not torch.isnan(partials[:n]).any()
    squares = torch.cat([r.reshape(-1) for r in refs] + want)
    total = ((0.5 * squares) ** 2).sum()
    assert ((0.5 * squares.abs().max()) ** 2 * squares.numel()).item() < 2 ** 51
    assert partials[:n].sum().item() == total.item()


def test_loss_partials_in_the_same_finalise_leave_the_gradients_alone():
    ops = _ops()
    rows, A, nblk = 257, 5, 37
    data = _integer_operands(rows, 64, DW_SHAPES, seed=12)
    plan = ops.MlpDwPlan(DW_SHAPES, rows, DEV)
    grads = _Grads(DW_SHAPES)
    g = torch.Generator(device=DEV).manual_seed(12)
    partials = torch.randn(nblk, 7 + 2 * A, generator=g, dtype=torch.float64, device=DEV)
    partials[:, 5] = 64.0
    scalars = torch.full((8,), NAN, device=DEV)
    d_logstd, dmb = torch.full((A,), NAN, device=DEV), torch.full((A,), NAN, device=DEV)
    kl, dvb = torch.full((1,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
    desc = ops.loss_finalize_desc(partials, nblk, A, nblk * 64, False, 2.0, 0.01, 1e-4, scalars, d_logstd, kl, dmb, dvb)
    n = _launch(plan, [d[:2] for d in data], grads, 'bf16', loss_finalize=desc)
    assert n == plan.finalize_blocks((), desc) == plan.finalize_blocks() + 1 + (2 * A + 7) // 8
    _check_bits(grads, [d[3] for d in data], 'with a loss descriptor')
    for t in (scalars, d_logstd, dmb, kl, dvb):
        assert torch.isfinite(t).all()


# ----------------------------------------------------------------------------- f: real-valued operands, the exact form

@pytest.mark.parametrize('case', [(1, None), (3, None), (5, None), (257, None), (515, None), (4096, None), (3075, 1),
                                  (8192, BIG), (16384, BIG)], ids=_id)
def test_exact_form_on_gaussian_operands_is_as_accurate_as_the_library(case):
    """The exact-product kernel alone on the edge cases above - K-splits 1, 2, 4, 8, 16, 32 and 64, ragged rows, waves
    without steps - judged like every exact-product kernel of the project: within 4x the error of the library's fp32
    product against fp64, floor 1e-6 of the tensor's scale (test_mlp_chain_gpu._close)."""
    from test_mlp_chain_gpu import _close
    ops = _ops()
    assert case in DW_CASES
    rows, tb = case
    g = torch.Generator(device=DEV).manual_seed(rows)
    jobs = [(_placed(1e-3 * torch.randn(rows, No, generator=g, device=DEV)),
             _placed(torch.randn(rows, Mi, generator=g, device=DEV))) for No, Mi in DW_SHAPES]
    plan = ops.MlpDwPlan(DW_SHAPES, rows, DEV, target_blocks=tb)
    grads = _Grads(DW_SHAPES)
    _launch(plan, jobs, grads, 'exact')
    for (dz, x), gv in zip(jobs, grads.views):
        assert torch.isfinite(gv).all()
        _close(gv, dz.double().t() @ x.double(), dz.t() @ x)
