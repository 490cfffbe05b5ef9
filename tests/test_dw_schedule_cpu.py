"""CPU: a host mirror of the weight-gradient launch's schedule (csrc/mlp_dw.hip), and proof that DW_CASES covers it.

The mirror restates, in plain Python, the parts of the launch that decide which rows and columns go where: the tile
split of a dimension (dw_split / dw_max_b), the plan's K-split (rlg_mlp_dw_plan), the workgroup decode of mlp_dw_body
(block_begin, then (tile, z) in one of two orders), the run of k-steps of every (z, wave) with its batches, its
register-set pipeline (plain / piped / rounds) and its predicated tail (dw_tile), and the range of gradient-maxima
entries an fp16-form wave scales by.  The exact form runs batches of 4 k-steps through three register sets, both split
forms batches of 8 through two.

DW_CASES and DW_SHAPES are what tests/test_weight_grads_gpu.py launches with integer operands, where every form must
return the bits of the fp64 product.  The tests below assert that these cases reach every tile template, every state of
both pipelines, every kind of ragged end and every K-split - each item by name, so a case that is dropped or a schedule
that is changed shows up here first.  A change to the launch has to keep this mirror in step with the kernel: the K-split
and the tile counts are checked against the library itself, the rest is what the GPU test's bit comparisons rest on.

When a GPU comparison fails, owner_of() names the (tile, wave, z -> rows) that produce an element of a layer's gradient.
"""
import ctypes
import os

import pytest

MAX_LAYERS = 8                    # kDwMaxLayers
MAX_TILES = 16                    # kDwMaxTiles
EXACT = dict(batch=4, sets=3)     # kDwBatch, kDwSets
SPLIT = dict(batch=8, sets=2)     # kDwSplitBatch, S
BIG = 1 << 20                     # a target_blocks that never limits the K-split

# (out_features, in_features) of the eight layers of one launch: together all nine (BO, BI) tile templates
DW_SHAPES = [(22, 100), (36, 20), (20, 12), (8, 6), (7, 12), (130, 260), (64, 60), (100, 108)]

# (rows, target_blocks); target_blocks None = the default plan, 1 pins the K-split at 8, BIG lets it grow to 64
DW_CASES = [
    (1, None), (2, None), (3, None), (5, None), (257, None), (515, None), (4096, None),
    (2549, 1), (3075, 1), (5125, 1),
    (8192, BIG), (16384, BIG),
]


# ----------------------------------------------------------------------------- the mirror

def dw_split(width, max_b):
    """Tiles [(start, b)] of one dimension - 16*b columns each, b in {4, 2, 1} - or None beyond kDwMaxTiles."""
    tiles, c = [], 0
    while c < width and len(tiles) < MAX_TILES:
        left = width - c
        bb = 1
        if left > 48:
            bb = 4
        elif left > 32:
            bb = 2 if max_b >= 2 else 1
        elif left > 16:
            bb = 2
        bb = min(bb, max_b)
        tiles.append((c, bb))
        c += 16 * bb
    return tiles if c >= width else None


def dw_max_b(address, ld, width):
    """The widest vector load per lane that the operand's address and row stride allow (dw_max_b)."""
    b = 1
    if address % 8 == 0 and ld % 2 == 0 and width >= 2:
        b = 2
    if address % 16 == 0 and ld % 4 == 0 and width >= 4:
        b = 4
    return b


def aligned_max_b(width):
    """What the plan assumes: 16-byte aligned operands, row stride = width."""
    return 4 if width % 4 == 0 else (2 if width % 2 == 0 else 1)


def split_products_default():
    e = os.environ.get('RLG_DW_BF16')
    return e is None or int(e) != 0


def dw_plan(rows, out_features, in_features, target_blocks=None):
    """(tiles_o, tiles_i, ksplit) of rlg_mlp_dw_plan, or None where it declines."""
    if rows <= 0 or out_features <= 0 or in_features <= 0 or (out_features * in_features) % 4:
        return None
    to = dw_split(out_features, aligned_max_b(out_features))
    ti = dw_split(in_features, aligned_max_b(in_features))
    if to is None or ti is None:
        return None
    steps = (rows + 3) // 4
    split = split_products_default()
    batch = SPLIT['batch'] if split else EXACT['batch']
    tb = target_blocks or 0
    if tb <= 0:
        tb = 100 if rows <= 4096 else (256 if (split or rows <= 8192) else 1024)
    tiles = len(to) * len(ti)
    ksplit = 8
    while ksplit * 2 <= 64 and steps // (ksplit * 2 * 4) >= 2 * batch and tiles * ksplit < tb:
        ksplit *= 2
    while ksplit > 1 and steps // (ksplit * 4) < batch:
        ksplit //= 2
    return len(to), len(ti), ksplit


def decode_block(local, tiles, ksplit):
    """(tile, z) of workgroup `local` of a layer (mlp_dw_body): K-slices of a multiple of 8 go round the XCDs."""
    if ksplit % 8 == 0:
        zlo, q = local & 7, local >> 3
        zhi = q // tiles
        return q - zhi * tiles, zhi * 8 + zlo
    t = local // ksplit
    return t, local - t * ksplit


def wave_run(rows, ksplit, z, wave, batch, sets):
    """The k-steps (4 rows each) of wave `wave` of K-slice z and how dw_tile walks them."""
    steps_total = (rows + 3) >> 2
    per_block = (steps_total + ksplit - 1) // ksplit
    per_wave = (per_block + 3) >> 2
    s_begin = z * per_block + wave * per_wave
    s_end = min(s_begin + per_wave, (z + 1) * per_block, steps_total)
    s_full_end = min(s_end, rows >> 2)
    nb = (s_full_end - s_begin) // batch if s_full_end > s_begin else 0
    plain = (nb - (sets - 1)) % sets if nb >= sets - 1 else nb
    piped = nb - plain >= sets - 1
    rounds = len(range(plain + sets - 1, nb, sets)) if piped else 0
    assert plain + ((sets - 1) + sets * rounds if piped else 0) == nb          # every full batch is issued once
    tail = max(s_end - (s_begin + nb * batch), 0)                              # predicated steps
    return dict(s_begin=s_begin, s_end=s_end, s_full_end=s_full_end, nb=nb, plain=plain, piped=piped, rounds=rounds,
                tail=tail, tail_batches=-(-tail // batch), empty=s_end <= s_begin,
                ragged=s_end > s_begin and s_end > s_full_end,
                cut_by_slice=s_begin < s_end == (z + 1) * per_block < min(s_begin + per_wave, steps_total),
                slice_cut_by_total=z * per_block < steps_total < (z + 1) * per_block,
                row_begin=4 * s_begin, row_end=max(min(4 * s_end, rows), 4 * s_begin))


def f16_entries(rows, ksplit, z, wave, per):
    """(e0, e1), inclusive: the gradient-maxima entries an fp16-form wave takes its scale from; None for no steps."""
    w = wave_run(rows, ksplit, z, wave, **SPLIT)
    shift = {16: 4, 64: 6}[per]
    e0, e1 = (4 * w['s_begin']) >> shift, (min(4 * w['s_end'], rows) - 1) >> shift
    return (e0, e1) if e0 <= e1 and not w['empty'] else None


def layer_tiles(out_features, in_features, max_b_o=None, max_b_i=None):
    return (dw_split(out_features, max_b_o or aligned_max_b(out_features)),
            dw_split(in_features, max_b_i or aligned_max_b(in_features)))


def owner_of(rows, shape, ksplit, o, i):
    """Who computes gradient element [o, i] of a layer: its tile (index, (BO, BI)), and per K-slice z the row ranges of
    the four waves whose sums the workgroup combines - the finalise adds the slices."""
    to, ti = layer_tiles(*shape)
    a = next(k for k, (s, b) in enumerate(to) if s <= o < s + 16 * b)
    c = next(k for k, (s, b) in enumerate(ti) if s <= i < s + 16 * b)
    slices = [[(w['row_begin'], w['row_end']) for w in (wave_run(rows, ksplit, z, v, **EXACT) for v in range(4))]
              for z in range(ksplit)]
    return dict(tile=a * len(ti) + c, template=(to[a][1], ti[c][1]), slices=slices)


def case_ksplits(rows, target_blocks):
    return [dw_plan(rows, No, Mi, target_blocks)[2] for No, Mi in DW_SHAPES]


def _waves(form):
    """Every (rows, ksplit, z, wave) run of DW_CASES under one form's batching."""
    for rows, tb in DW_CASES:
        for ksplit in sorted(set(case_ksplits(rows, tb))):
            for z in range(ksplit):
                for wave in range(4):
                    yield rows, ksplit, z, wave, wave_run(rows, ksplit, z, wave, **form)


# ----------------------------------------------------------------------------- the mirror against the library

def _lib():
    from rl_games_amd import _lib
    return _lib.load()


def _lib_plan(rows, No, Mi, target_blocks):
    p4 = (ctypes.c_int * 4)()
    need = _lib().rlg_mlp_dw_plan(rows, No, Mi, target_blocks or 0, p4)
    return None if need < 0 else (p4[1], p4[2], p4[3], need)


def test_the_mirrored_plan_is_the_librarys_for_every_case():
    assert split_products_default(), 'the suite runs with the default product form'
    for rows, tb in DW_CASES:
        for No, Mi in DW_SHAPES:
            got = _lib_plan(rows, No, Mi, tb)
            want = dw_plan(rows, No, Mi, tb)
            assert got is not None and got[:3] == want, (rows, tb, No, Mi, got, want)
            assert got[3] == want[2] * No * Mi


@pytest.mark.parametrize('rows', [1, 129, 255, 257, 511, 769, 1023, 2049, 4096, 8192, 16384, 32768])
@pytest.mark.parametrize('tb', [None, 1, 256, BIG])
def test_the_mirrored_plan_is_the_librarys_beyond_the_cases(rows, tb):
    for No, Mi in DW_SHAPES + [(400, 108), (200, 400), (1024, 4), (1028, 4), (257, 4), (3, 5)]:
        got, want = _lib_plan(rows, No, Mi, tb), dw_plan(rows, No, Mi, tb)
        assert (got is None) == (want is None) and (got is None or got[:3] == want), (rows, tb, No, Mi)


def test_the_envelope_of_the_plan():
    """1,024 features are 16 tiles of 64; 1,028 need a 17th; an odd width is cut in 16-column tiles - 257 need 17."""
    assert dw_plan(64, 1024, 4)[0] == 16 and _lib_plan(64, 1024, 4, None) is not None
    for No in (1028, 257):
        assert dw_plan(64, No, 4) is None and _lib_plan(64, No, 4, None) is None
    # at a 4-byte aligned address every tile is 16 columns wide: more than 256 columns do not fit
    assert dw_split(260, dw_max_b(4, 260, 260)) is None and len(dw_split(256, 1)) == 16
    assert dw_max_b(8, 260, 260) == 2 and dw_max_b(16, 260, 260) == 4 and dw_max_b(16, 130, 130) == 2


# ----------------------------------------------------------------------------- properties of the schedule itself

def test_tiles_cover_every_column_once():
    for width in list(range(1, 300)) + [400, 1024]:
        for max_b in (1, 2, 4):
            tiles = dw_split(width, max_b)
            if tiles is None:
                assert max_b == 1 and width > 256 or max_b == 2 and width > 512
                continue
            end = 0
            for start, b in tiles:
                assert start == end and b in (1, 2, 4) and b <= max_b
                end += 16 * b
            assert width <= end < width + 16 * tiles[-1][1]


def test_the_workgroup_decode_is_one_to_one():
    for tiles in (1, 2, 3, 7, 15):
        for ksplit in (1, 2, 4, 8, 16, 32, 64):
            seen = {decode_block(b, tiles, ksplit) for b in range(tiles * ksplit)}
            assert seen == {(t, z) for t in range(tiles) for z in range(ksplit)}


def test_the_waves_of_a_launch_take_every_row_once():
    for form in (EXACT, SPLIT):
        last = None
        for rows, ksplit, z, wave, w in _waves(form):
            if (z, wave) == (0, 0):
                assert last is None or last[1] == last[0], last
                at = 0
            if not w['empty']:
                assert w['row_begin'] == at and w['row_end'] > at
                at = w['row_end']
                # unpredicated batch loads stay inside the rows
                assert 4 * (w['s_begin'] + w['nb'] * form['batch']) <= rows
            last = (rows, at)
        assert last[1] == last[0]


# ----------------------------------------------------------------------------- coverage of DW_CASES

def test_cases_are_small_and_the_launch_is_a_full_descriptor_table():
    assert len(DW_SHAPES) == MAX_LAYERS
    assert max(r for r, _ in DW_CASES) <= 17024 and max(No * Mi for No, Mi in DW_SHAPES) <= 130 * 260
    assert len(DW_CASES) == len(set(DW_CASES))


def test_cases_cover_all_nine_tile_templates():
    seen = set()
    for No, Mi in DW_SHAPES:
        to, ti = layer_tiles(No, Mi)
        seen |= {(a[1], b[1]) for a in to for b in ti}
    assert seen == {(a, b) for a in (1, 2, 4) for b in (1, 2, 4)}
    # the launch picks the template per tile and the schedule per (rows, ksplit): every case runs all nine, in every form


def test_cases_cover_both_workgroup_orders_of_a_layer():
    multi = {(k % 8 == 0) for rows, tb in DW_CASES for k, (No, Mi) in zip(case_ksplits(rows, tb), DW_SHAPES)
             if k > 1 and len(layer_tiles(No, Mi)[0]) * len(layer_tiles(No, Mi)[1]) > 1}
    assert multi == {True, False}


def test_cases_cover_the_exact_forms_pipeline():
    runs = [w for *_, w in _waves(EXACT)]
    assert {w['nb'] for w in runs} >= set(range(9))
    assert {w['plain'] for w in runs if w['piped']} == {0, 1, 2}
    assert {w['plain'] for w in runs if not w['piped']} >= {0, 1}            # (fewer than two batches: all of them plain)
    assert {min(w['rounds'], 2) for w in runs if w['piped']} == {0, 1, 2}
    assert {w['tail'] for w in runs} >= {0, 1, 2, 3}


def test_cases_cover_the_split_forms_pipeline():
    runs = [w for *_, w in _waves(SPLIT)]
    assert {w['nb'] for w in runs} >= set(range(5))
    assert {w['plain'] for w in runs if w['piped']} == {0, 1}
    assert {w['plain'] for w in runs if not w['piped']} == {0}                # (no batch at all)
    assert {min(w['rounds'], 2) for w in runs if w['piped']} == {0, 1, 2}
    assert any(w['tail_batches'] == 0 and w['nb'] > 0 for w in runs)         # no tail batch
    assert any(w['tail_batches'] == 1 and 0 < w['tail'] < 8 for w in runs)   # a tail batch with fewer than 8 steps
    assert any(w['tail_batches'] == 1 and w['tail'] == 8 for w in runs)      # (a full one whose last step is ragged)
    assert {w['tail'] % 8 for w in runs} == set(range(8))


def test_cases_cover_the_ragged_ends():
    all_rows = {r for r, _ in DW_CASES}
    assert {1, 2, 3} <= all_rows and {r % 4 for r in all_rows} == {0, 1, 2, 3}
    for form in (EXACT, SPLIT):
        runs = list(_waves(form))
        assert any(rows == 5 and w['empty'] for rows, *_, w in runs)
        assert any(w['empty'] and w['s_begin'] > w['s_end'] for *_, w in runs)      # a run that begins past the end
        for key in ('ragged', 'cut_by_slice', 'slice_cut_by_total'):
            assert any(w[key] for *_, w in runs), key
        for m in (1, 2, 3):
            assert any(w['ragged'] and rows % 4 == m for rows, *_, w in runs), m
        # ragged after full batches, and as the only step of a wave
        assert any(w['ragged'] and w['nb'] > 0 for *_, w in runs)
        assert any(w['ragged'] and w['s_end'] - w['s_begin'] == 1 for *_, w in runs)


def test_cases_cover_every_ksplit():
    seen, multi = set(), set()
    for rows, tb in DW_CASES:
        for k, (No, Mi) in zip(case_ksplits(rows, tb), DW_SHAPES):
            to, ti = layer_tiles(No, Mi)
            seen.add(k)
            if len(to) * len(ti) > 1:
                multi.add(k)
    assert seen == {1, 2, 4, 8, 16, 32, 64}
    assert multi >= {8, 16, 32, 64}                    # the (zhi, tile, zlo) order matters
    # 64 slices: the only count that enters the finalise's loop of four loads in flight (z + 48 < ksplit)
    assert [k for k in sorted(seen) if 0 + 3 * 16 < k] == [64]


def test_cases_cover_the_default_plan_and_the_pinned_ones():
    default = {k for rows, tb in DW_CASES if tb is None for k in case_ksplits(rows, tb)}
    assert default == {1, 2, 4, 8, 16}
    assert all(set(case_ksplits(rows, tb)) == {8} for rows, tb in DW_CASES if tb == 1)
    exact_nb = {w['nb'] for rows, tb in DW_CASES if tb == 1 for k in set(case_ksplits(rows, tb))
                for z in range(k) for v in range(4) for w in [wave_run(rows, k, z, v, **EXACT)]}
    assert exact_nb >= {5, 6, 7}


def test_cases_cover_the_fp16_forms_entry_ranges():
    spans = {16: set(), 64: set()}
    for per in (16, 64):
        for rows, ksplit, z, wave, w in _waves(SPLIT):
            e = f16_entries(rows, ksplit, z, wave, per)
            assert (e is None) == w['empty']
            if e is not None:
                assert 0 <= e[0] <= e[1] < -(-rows // per)                  # never past the last block of rows
                spans[per].add(e[1] - e[0] + 1)
    assert spans[64] >= {1, 2, 3}                      # (a run of 41 steps that straddles four is possible too)
    assert spans[16] >= {1, 2, 3, 4} and max(spans[16]) > 4
    for per in (16, 64):
        assert any(rows % per for rows, _ in DW_CASES) and any(rows % per == 0 for rows, _ in DW_CASES)
        # a wave whose first entry is not the slice's first, and the last entry of a ragged table
        assert any(f16_entries(rows, k, z, v, per) == ((rows - 1) // per,) * 2 and rows % per
                   for rows, k, z, v, w in _waves(SPLIT) if not w['empty'])


def test_owner_of_names_the_rows_of_an_element():
    rows, tb = 4099, None
    k = case_ksplits(rows, tb)[5]
    who = owner_of(rows, DW_SHAPES[5], k, 129, 259)
    assert who['template'] == (1, 1) and who['tile'] == 4 * 5 + 4      # (130 columns, 8-byte rows: 32 + 32 + 32 + 32 + 16)
    flat = [r for s in who['slices'] for r in s if r[1] > r[0]]
    assert flat[0][0] == 0 and flat[-1][1] == rows and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
