"""Cost of `use_diagnostics` on the headline epoch (65,536 envs x 32 steps, minibatch 32,768, 5 mini-epochs, the
mini-epoch HIP graph): ms per train_epoch with the option off and on, in one process.

    python tools/diag_overhead.py [--epochs 10] [--warmup 3]
"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rl_games_amd import configs  # noqa: E402
from rl_games_amd.agent import A2CAgent  # noqa: E402


def ms_per_epoch(use_diagnostics, epochs, warmup):
    params = configs.humanoid_65536(use_diagnostics=use_diagnostics, print_stats=False)
    torch.manual_seed(5)
    agent = A2CAgent('diag_overhead', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    times = []
    for e in range(warmup + epochs):
        agent.update_epoch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.train_epoch()
        if agent.global_rank == 0:
            agent.diagnostics.epoch(agent, current_epoch=e)
        torch.cuda.synchronize()
        if e >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    off, _ = ms_per_epoch(False, a.epochs, a.warmup)
    on, agent = ms_per_epoch(True, a.epochs, a.warmup)
    keys = {k: float(v.reshape(-1)[0]) for k, v in agent.diagnostics.diag_dict.items()}
    print(json.dumps({'ms_per_epoch_off': round(off, 3), 'ms_per_epoch_on': round(on, 3),
                      'added_pct': round(100.0 * (on - off) / off, 2), 'graph': agent._update_graphs.epoch is not None,
                      'diag': keys}))


if __name__ == '__main__':
    main()
