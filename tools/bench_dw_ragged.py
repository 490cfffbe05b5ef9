"""Time of the weight-gradient kernel for widths off a multiple of 4 (csrc/mlp_dw_ragged.hip, ops.ragged_dw) against the
library product it replaces, `torch.mm(dz.t(), x, out=g)`, in one process.

  shapes : (rows, No, Mi) - the SMAC first layer of profiles/chain_ln.txt at 2,560 and 20,480 rows, MuJoCo-sized first
           layers at the headline minibatch of 32,768 rows, and a rank's 4,096-row minibatch
  update : one whole train_actor_critic() of the layer-norm discrete agent of tools/bench_chain_ln.py (obs 98, [512, 256],
           15 actions) at 20,480 and 2,560 rows, its WeightGrads with `ragged` on and off.  Below ops.RAGGED_MIN_ROWS
           the route declines: the 2,560-row measurement lowers that constant, to time what the rule leaves out
Each shape is timed twice: as eager calls, and as replays of a captured graph of 20 calls (device time: what an update
that replays its launches sees).  Both settings are warmed up, then alternate for --rounds timed rounds of --calls calls each, every round between device
synchronisations.  One JSON line per measurement: median and spread (min .. max) over the rounds per setting, ms per call,
the ratio of the medians, and for a shape the largest difference between the two results over the largest |G|.

  --short: the one-launch kernel for short minibatches (ops.ragged_dw_short) instead, at the first-layer shapes of the
           reference's MuJoCo and SMAC configs on minibatches of 2,048 .. 16,384 rows: against the library product and
           against ops.ragged_dw (the long kernel, forced on), same method; no update measurement (profiles/dw_ragged_short.txt)

    python tools/bench_dw_ragged.py [--what shapes,update20480,update2560] [--rounds 7] [--calls 200] [--short]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from rl_games_amd import ops  # noqa: E402
from bench_chain_ln import _agent, _minibatch, _timed  # noqa: E402

SHAPES = [(2560, 512, 98), (20480, 512, 98), (32768, 256, 17), (32768, 400, 105), (4096, 256, 11)]
SHORT_SHAPES = [(2560, 512, 98), (4096, 256, 11), (2048, 256, 17), (8192, 512, 98), (16384, 400, 105)]


GRAPH_CALLS = 20


def _graphed(fn):
    """One replay of a captured graph of GRAPH_CALLS calls of fn (one stream, no branches); _measure's figures for it are
    per replay - divide by GRAPH_CALLS for a call."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_CALLS):
            fn()
    return graph.replay


def _measure(name, fns, rounds, calls, extra=None):
    for fn in fns.values():                    # warm-up of exactly the timed call
        _timed(fn, 3)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():              # the settings alternate
            times[k].append(_timed(fn, calls))
    out = {'what': name, 'unit': 'ms per call', 'rounds': rounds, 'calls': calls}
    for k, ts in times.items():
        out[k] = {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
    for k in times:
        if k != 'library':
            out[f'library_over_{k}'] = round(out['library']['median'] / out[k]['median'], 3)
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='shapes,update20480,update2560')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--short', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dw_ragged.py measures on the GPU; none found')
    dev = 'cuda:0'
    for what in (['shapes'] if args.short else args.what.split(',')):
        if what == 'shapes':
            for rows, No, Mi in (SHORT_SHAPES if args.short else SHAPES):
                torch.manual_seed(rows + No + Mi)
                dz, x = torch.randn(rows, No, device=dev), torch.randn(rows, Mi, device=dev)
                g, gl = torch.empty(No, Mi, device=dev), torch.empty(No, Mi, device=dev)
                fns = {'ragged': lambda: ops.ragged_dw(dz, x, g), 'library': lambda: torch.mm(dz.t(), x, out=gl)}
                if args.short:
                    g2 = torch.empty(No, Mi, device=dev)
                    fns = {'short': lambda: ops.ragged_dw_short(dz, x, g), 'library': fns['library'],
                           'ragged': lambda: ops.ragged_dw(dz, x, g2)}
                for fn in fns.values():
                    fn()
                diff = ((g - gl).abs().max() / gl.abs().max()).item()
                _measure(f'dw {rows} x {No} x {Mi}', fns, args.rounds, args.calls, {'max_diff_over_max': float(f'{diff:.3g}')})
                # the same launches replayed from a graph of GRAPH_CALLS calls, as an agent's update replays them: device
                # time without the host's share of an eager call (the two wrappers cost different host time)
                _measure(f'dw {rows} x {No} x {Mi} (ms per graph replay of {GRAPH_CALLS} calls)', {k: _graphed(fn) for k, fn in fns.items()},
                         args.rounds, max(args.calls // GRAPH_CALLS, 1))
        elif what.startswith('update'):
            mb = int(what[len('update'):])
            fns = {}
            if mb < ops.RAGGED_MIN_ROWS:
                ops.RAGGED_MIN_ROWS = 1
            for k, on in (('ragged', True), ('library', False)):
                ag = _agent(mb // 8, 8, mb, True)
                wg = ag._chains[0].weight_grads
                wg.ragged = on
                _minibatch(ag)
                fns[k] = (lambda a: lambda: a.train_actor_critic(a.dataset[0]))(ag)
                fns[k]()
                assert wg.last_dw_library_jobs == (0 if on else 1), (k, wg.last_dw_library_jobs)
            _measure(what, fns, args.rounds, args.calls)
        else:
            raise SystemExit(f'unknown measurement {what}')


if __name__ == '__main__':
    main()
