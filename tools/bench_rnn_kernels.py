"""Launch times of the sequence-persistent recurrent kernels (csrc/lstm*.hip, csrc/gru*.hip) on one MI355X:
forward (training: everything kept for backward; inference: final states only) and backward, LSTM next to GRU, for
H in {64, 128} at (S, T) in {(1024, 16), (4096, 1), (4096, 16)}.  Device events around 100 launches after 10 warm-up
launches, 5 % dones; the copy that restores the gate inputs in front of each forward is timed alone and subtracted.

    python tools/bench_rnn_kernels.py --pair

times the paired launches (csrc/rnn_seq.hpp, "paired launches": two problems of one shape in one launch) against the
two single launches back to back: both cells, H in {64, 128}, S in {16, 256, 4,096}, T in {1, 16} - T = 1 in the
rollout's form (final states only), T = 16 in the training form - forward and backward.  Per row the two versions
alternate over 7 windows of 50 launches each (10 warm-up launches per version first); printed are the medians, the
ratio pair / singles and each version's spread (max - min over its windows, as a share of its median): a ratio inside
the spreads is no difference.  The forwards run on the gates the launch before left (activated values, in (-1, 1)):
the same work, no restoring copy inside the window."""
import os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_games_amd import ops

DEV = 'cuda:0'
N, WARM = 100, 10


def timed(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(N):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / N          # us per call


def bench(cell, H, S, T):
    g = torch.Generator().manual_seed(1)
    ng = 4 if cell == 'lstm' else 3
    rows = S * T
    gin = torch.randn(rows, ng * H, generator=g).to(DEV)
    w_hh = (torch.randn(ng * H, H, generator=g) / H ** 0.5).to(DEV)
    b_hh = (0.1 * torch.randn(ng * H, generator=g)).to(DEV)
    h0, c0 = (0.5 * torch.randn(S, H, generator=g)).to(DEV), (0.5 * torch.randn(S, H, generator=g)).to(DEV)
    dones = (torch.rand(rows, generator=g) < 0.05).to(torch.uint8).to(DEV)
    d_out = torch.randn(rows, H, generator=g).to(DEV)
    gates = torch.empty_like(gin)
    out, kept, hprev = (torch.empty(rows, H, device=DEV) for _ in range(3))
    hT, cT = torch.empty(S, H, device=DEV), torch.empty(S, H, device=DEV)
    dg, dgh = torch.empty_like(gin), torch.empty_like(gin)

    def fwd(train):
        gates.copy_(gin)
        if cell == 'lstm':
            ops.lstm_seq_forward(gates, w_hh, h0, c0, dones, out, kept if train else None, hprev if train else None,
                                 None if train else hT, None if train else cT, seq_len=T)
        else:
            ops.gru_seq_forward(gates, w_hh, b_hh, h0, dones, out, kept if train else None, hprev if train else None,
                                None if train else hT, seq_len=T)

    def bwd():
        if cell == 'lstm':
            ops.lstm_seq_backward(gates, kept, c0, dones, w_hh, d_out, dg, T)
        else:
            ops.gru_seq_backward(gates, kept, hprev, dones, w_hh, d_out, dg, dgh, T)

    copy = timed(lambda: gates.copy_(gin))
    t_inf = timed(lambda: fwd(False)) - copy
    t_train = timed(lambda: fwd(True)) - copy       # leaves the activated gates and the kept arrays for bwd
    t_bwd = timed(bwd)
    print(f'{cell:4s} {H:4d} {S:6,d} {T:3d}   {t_train:8.1f}   {t_inf:8.1f}   {t_bwd:8.1f}   (copy {copy:.1f})', flush=True)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def alternate(pair, singles, windows=7, n=50):
    """(median us of the paired launch, of the two single launches, spread of each as a share of its median)"""
    for fn in (pair, singles):
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    tp, ts = [], []
    for _ in range(windows):
        tp.append(window(pair, n))
        ts.append(window(singles, n))
    mp, ms = statistics.median(tp), statistics.median(ts)
    return mp, ms, (max(tp) - min(tp)) / mp, (max(ts) - min(ts)) / ms


def bench_pair(cell, H, S, T):
    ng = 4 if cell == 'lstm' else 3
    rows = S * T
    train = T > 1

    def problem(seed):
        g = torch.Generator().manual_seed(seed)
        p = dict(gin=torch.randn(rows, ng * H, generator=g).to(DEV),
                 w_hh=(torch.randn(ng * H, H, generator=g) / H ** 0.5).to(DEV),
                 b_hh=(0.1 * torch.randn(ng * H, generator=g)).to(DEV),
                 h0=(0.5 * torch.randn(S, H, generator=g)).to(DEV), c0=(0.5 * torch.randn(S, H, generator=g)).to(DEV),
                 dones=(torch.rand(rows, generator=g) < 0.05).to(torch.uint8).to(DEV),
                 d_out=torch.randn(rows, H, generator=g).to(DEV))
        p['gates'] = p['gin'].clone()
        for k in ('out', 'kept', 'hprev'):
            p[k] = torch.empty(rows, H, device=DEV)
        p['hT'], p['cT'] = torch.empty(S, H, device=DEV), torch.empty(S, H, device=DEV)
        p['dg'], p['dgh'] = torch.empty_like(p['gin']), torch.empty_like(p['gin'])
        return p

    def fwd_args(p, keep):
        tail = (p['kept'] if keep else None, p['hprev'] if keep else None, None if keep else p['hT'])
        if cell == 'lstm':
            return (p['gates'], p['w_hh'], p['h0'], p['c0'], p['dones'], p['out']) + tail + (None if keep else p['cT'],)
        return (p['gates'], p['w_hh'], p['b_hh'], p['h0'], p['dones'], p['out']) + tail

    def bwd_args(p):
        if cell == 'lstm':
            return (p['gates'], p['kept'], p['c0'], p['dones'], p['w_hh'], p['d_out'], p['dg'])
        return (p['gates'], p['kept'], p['hprev'], p['dones'], p['w_hh'], p['d_out'], p['dg'], p['dgh'])

    a, b = problem(1), problem(2)
    f1, b1 = getattr(ops, f'{cell}_seq_forward'), getattr(ops, f'{cell}_seq_backward')
    fa, fb = fwd_args(a, train), fwd_args(b, train)

    def fwd_singles():
        f1(*fa, seq_len=T)
        f1(*fb, seq_len=T)
    res = [alternate(lambda: ops.rnn_seq(cell, 'forward', [fa, fb], T), fwd_singles)]
    # what the backward reads: one training forward from the gate inputs
    for p in (a, b):
        p['gates'].copy_(p['gin'])
        f1(*fwd_args(p, True), seq_len=T)
    ba, bb = bwd_args(a), bwd_args(b)

    def bwd_singles():
        b1(*ba, T)
        b1(*bb, T)
    res.append(alternate(lambda: ops.rnn_seq(cell, 'backward', [ba, bb], T), bwd_singles))
    for name, (mp, ms, sp, ss) in zip(('forward', 'backward'), res):
        print(f'{cell:4s} {H:4d} {S:6,d} {T:3d} {name:9s} {mp:9.1f} {ms:9.1f}   {mp / ms:5.2f}   {100 * sp:5.1f} %  {100 * ss:5.1f} %',
              flush=True)


if '--pair' in sys.argv[1:]:
    print('cell    H      S   T direction   pair us  2 single   ratio  spread pair  singles')
    for cell in ('lstm', 'gru'):
        for H in (64, 128):
            for S in (16, 256, 4096):
                for T in (1, 16):
                    bench_pair(cell, H, S, T)
else:
    print('cell    H      S   T   fwd train    fwd inf   backward   [us per launch]')
    for H in (64, 128):
        for S, T in ((1024, 16), (4096, 1), (4096, 16)):
            for cell in ('lstm', 'gru'):
                bench(cell, H, S, T)
