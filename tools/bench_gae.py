"""Micro-benchmark of the GAE kernels on one MI355X (development tool, not the judged bench).

Prints kernel time from HIP events over back-to-back launches and the algorithmic GB/s
(17 B per env-step for the fused kernel: r 4 + v 4 + done 1 read, ret 4 + adv 4 written).

--long: horizons above 64.  Per ENVSxHORIZON shape, in one process on the same rotating buffers, the chunked fused
launch (rlg_gae_long) beside what runs without it for the same job: the strided scan on env-major views, `advs +
values`, `returns - values` and triple_moments (→ profiles/gae_long.txt)."""
import argparse
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_games_amd import gae, ops  # noqa: E402


def time_launches(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def bench_long(shapes, iters, repeats):
    dev = 'cuda:0'
    for N, H in shapes:
        set_bytes = N * H * 25 + N * 5            # r, v, ret, adv 4 B each, dones 1 B, and the torch path's advs + adv
        rotate = min(64, max(4, -(-600_000_000 // set_bytes)))      # over the 256 MB MALL, where memory allows
        sets = [dict(r=torch.randn(N, H, device=dev), v=torch.randn(N, H, device=dev),
                     d=(torch.rand(N, H, device=dev) < 0.05).to(torch.uint8), lv=torch.randn(N, device=dev),
                     ld=(torch.rand(N, device=dev) < 0.05).to(torch.uint8), ret=torch.empty(N, H, device=dev),
                     adv=torch.empty(N, H, device=dev),
                     part=torch.empty(gae.num_moment_partials(N), 6, dtype=torch.float64, device=dev))
                for _ in range(rotate)]
        k = [0]

        def fused():
            s = sets[k[0] % rotate]
            k[0] += 1
            gae.gae_returns_advantages(s['r'], s['v'], s['d'], s['lv'], s['ld'], 0.99, 0.95, out_returns=s['ret'],
                                       out_advantages=s['adv'], moment_partials=s['part'])

        def unfused():      # A2CAgent._finish_rollout's else branch + prepare_dataset's moments
            s = sets[k[0] % rotate]
            k[0] += 1
            vv = s['v'].t().unsqueeze(2)
            advs = gae.compute_gae(s['r'].t().unsqueeze(2), vv, s['d'].t(), s['lv'].unsqueeze(1), s['ld'], 0.99, 0.95,
                                   long_horizon=False)
            ret = (advs + vv).transpose(0, 1).reshape(-1)
            vf = s['v'].reshape(-1)
            ops.triple_moments(ret - vf, vf, ret)

        fused(), unfused()
        a = sets[0]                               # same results on the way: the timed paths do the same job
        advs = gae.compute_gae(a['r'].t().unsqueeze(2), a['v'].t().unsqueeze(2), a['d'].t(), a['lv'].unsqueeze(1),
                               a['ld'], 0.99, 0.95, long_horizon=False)
        assert torch.equal((advs + a['v'].t().unsqueeze(2))[..., 0].t(), a['ret']), 'fused returns != strided + add'
        del advs, a
        best = {}
        for _ in range(repeats):                  # alternating, the fastest window of each
            for name, fn in (('fused', fused), ('unfused', unfused)):
                us = time_launches(fn, iters, warmup=10)
                best[name] = min(best.get(name, us), us)
        gbs = N * H * 17 / best['fused'] * 1e-3
        print(f'{N:6d} x {H:5d}  rotate {rotate:2d}  chunked fused {best["fused"]:9.2f} us  strided + add + sub + moments '
              f'{best["unfused"]:9.2f} us  x{best["unfused"] / best["fused"]:5.2f}  {gbs:8.1f} GB/s on 17 B/env-step',
              flush=True)
        del sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--long', nargs='*', metavar='ENVSxHORIZON', default=None,
                    help='time the chunked long-horizon launch against the unfused sequence at these shapes '
                         '(default: 4096x128 4096x512 65536x128 1024x1024 16x4096)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--horizon', type=int, default=32)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rotate', type=int, default=16,
                    help='number of distinct buffer sets cycled through (defeats the 256 MB MALL when large)')
    a = ap.parse_args()
    if a.long is not None:
        shapes = a.long or ['4096x128', '4096x512', '65536x128', '1024x1024', '16x4096']
        return bench_long([tuple(int(x) for x in sh.split('x')) for sh in shapes], a.iters, a.repeats)
    dev = 'cuda:0'
    N, H = a.envs, a.horizon
    sets = []
    for i in range(a.rotate):
        sets.append(dict(
            r=torch.randn(N, H, device=dev), v=torch.randn(N, H, device=dev),
            d=(torch.rand(N, H, device=dev) < 0.05).to(torch.uint8),
            lv=torch.randn(N, device=dev), ld=(torch.rand(N, device=dev) < 0.05).to(torch.uint8),
            ret=torch.empty(N, H, device=dev), adv=torch.empty(N, H, device=dev),
            part=torch.empty(gae.num_moment_partials(N), 6, dtype=torch.float64, device=dev)))
    k = [0]

    def fused():
        s = sets[k[0] % len(sets)]
        k[0] += 1
        gae.gae_returns_advantages(s['r'], s['v'], s['d'], s['lv'], s['ld'], 0.99, 0.95,
                                   out_returns=s['ret'], out_advantages=s['adv'],
                                   moment_partials=s['part'])

    def raw_view():
        s = sets[k[0] % len(sets)]
        k[0] += 1
        gae.compute_gae(s['r'].t().unsqueeze(2), s['v'].t().unsqueeze(2), s['d'].t(),
                        s['lv'].unsqueeze(1), s['ld'], 0.99, 0.95)

    tm = dict(r=torch.randn(H, N, 1, device=dev), v=torch.randn(H, N, 1, device=dev),
              d=(torch.rand(H, N, device=dev) < 0.05).float(), lv=torch.randn(N, 1, device=dev),
              ld=(torch.rand(N, device=dev) < 0.05).float())

    def strided_tm():
        gae.compute_gae(tm['r'], tm['v'], tm['d'], tm['lv'], tm['ld'], 0.99, 0.95)

    steps = N * H
    for name, fn, bytes_per in (('fused env-major (ret+adv+moments)', fused, 17),
                                ('env-major raw (compute_gae view)', raw_view, 13),
                                ('strided time-major f32 dones', strided_tm, 16)):
        us = time_launches(fn, a.iters)
        gbs = steps * bytes_per / us * 1e-3
        print(f'{name:40s} {us:8.2f} us/launch  {gbs:8.1f} GB/s algorithmic  '
              f'({gbs / 8000 * 100:5.1f}% of 8 TB/s)  [{steps * bytes_per / 1e6:.2f} MB]')


if __name__ == '__main__':
    main()
