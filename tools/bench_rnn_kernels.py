"""Launch times of the sequence-persistent recurrent kernels (csrc/lstm*.hip, csrc/gru*.hip) on one MI355X:
forward (training: everything kept for backward; inference: final states only) and backward, LSTM next to GRU, for
H in {64, 128} at (S, T) in {(1024, 16), (4096, 1), (4096, 16)}.  Device events around 100 launches after 10 warm-up
launches, 5 % dones; the copy that restores the gate inputs in front of each forward is timed alone and subtracted."""
import os, sys, torch
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


print('cell    H      S   T   fwd train    fwd inf   backward   [us per launch]')
for H in (64, 128):
    for S, T in ((1024, 16), (4096, 1), (4096, 16)):
        for cell in ('lstm', 'gru'):
            bench(cell, H, S, T)
