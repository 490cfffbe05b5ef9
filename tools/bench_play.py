"""Steps per second of the players with `player.fused` on (the engine's inference forward + one head launch of
csrc/play.hip, replayed as a HIP graph; run(): episode accounting on the device) against off (the torch modules, two
host reads per step in run()), in one process.

Configurations: the BASELINE MLP ([400, 200, 100], obs 108, 21 actions) at 4,096 and 65,536 envs, deterministic and
stochastic; `configs.smac_rnn_discrete` with a GRU of 128 units and action masks at 4,096 envs.  Per configuration one
player per setting (random weights: the time does not depend on them); both warm up (allocations, library algorithm
choice, the step graph's capture), then the two settings alternate for --rounds timed rounds of --steps steps, each round
between device synchronisations on the host clock.  Two figures per setting: the policy step alone (get_action /
get_masked_action on a device observation) and run() on the synthetic env (policy step + env step + accounting).
Launch counts: the library entries of one eager step, recorded by name as tests/test_actor_paths_gpu.py does (torch's
own launches - the torch path's modules, the draws - are not library entries and are not counted).
Writes profiles/play_fused.txt: the table, and the kernel-resource-usage remarks of csrc/play.hip.

    python tools/bench_play.py [--steps 200] [--rounds 5] [--only mlp4096,mlp65536,gru4096] [--skip-resources]
"""
import argparse
import copy
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl_games_amd import _lib, configs  # noqa: E402
from rl_games_amd.player import PpoPlayerContinuous, PpoPlayerDiscrete  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'play_fused.txt')
CONFIGS = {'mlp4096': ('BASELINE MLP, 4,096 envs', lambda: configs.humanoid_65536(num_actors=4096, minibatch_size=4096), (True, False)),
           'mlp65536': ('BASELINE MLP, 65,536 envs', lambda: configs.humanoid_65536(), (True, False)),
           'gru4096': ('smac_rnn_discrete GRU 128 masked, 4,096 envs',
                       lambda: configs.smac_rnn_discrete(num_actors=4096, cell='gru', units=128), (True,))}


class _Recorder:
    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('rlg_'):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def _player(params, fused, deterministic):
    pp = copy.deepcopy(params)
    pp['config']['player'] = {'fused': fused, 'print_stats': False, 'deterministic': deterministic,
                              'games_num': 10 ** 12}
    torch.manual_seed(0)
    cls = PpoPlayerDiscrete if params['algo']['name'] == 'a2c_discrete' else PpoPlayerContinuous
    player = cls(pp)
    if fused and player._fused is None:
        raise RuntimeError('the fused play path declined this configuration')
    player.has_batch_dimension = True
    player.batch_size = pp['config']['num_actors']
    player.init_rnn()
    return player


def _step(player, obs, masks, deterministic):
    if masks is not None:
        return player.get_masked_action(obs, masks, deterministic)
    return player.get_action(obs, deterministic)


def _timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def _entries_per_step(player, obs, masks, deterministic):
    """Library entries of the player's first step at this key: it runs eagerly (the second call captures the graph)."""
    recorder = _Recorder(_lib.load())
    real, _lib._lib = _lib._lib, recorder
    try:
        _step(player, obs, masks, deterministic)
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return len(recorder.names), sorted(set(recorder.names))


def bench(name, steps, rounds):
    title, make, modes = CONFIGS[name]
    params = make()
    rows = []
    for deterministic in modes:
        players = {fused: _player(params, fused, deterministic) for fused in (True, False)}
        env = players[True].env
        obs = env.reset()
        masks = env.get_action_mask() if getattr(env, 'action_masks', False) else None
        counts = {fused: _entries_per_step(p, obs, masks, deterministic) for fused, p in players.items()}
        step_fns, run_fns = {}, {}
        for fused, p in players.items():
            def policy(n, p=p):
                for _ in range(n):
                    _step(p, obs, masks, deterministic)

            def run(n, p=p):
                p.max_steps = n
                p.run()
            step_fns[fused], run_fns[fused] = policy, run
            policy(5)                                  # warm-up: the second call captures, the rest replay
            run(20)
        step_rate, run_rate = {True: [], False: []}, {True: [], False: []}
        for _ in range(rounds):                        # alternating
            for fused in (True, False):
                step_rate[fused].append(_timed(step_fns[fused], steps))
            for fused in (True, False):
                run_rate[fused].append(_timed(run_fns[fused], steps))
        rows.append((title, 'deterministic' if deterministic else 'stochastic',
                     {f: statistics.median(v) for f, v in step_rate.items()},
                     {f: statistics.median(v) for f, v in run_rate.items()}, counts))
        del players
        torch.cuda.empty_cache()
    return rows


def resource_lines():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        return ['not measured (no hipcc)']
    src = os.path.join(ROOT, 'rl_games_amd', 'csrc', 'play.hip')
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                              '-I' + os.path.join(ROOT, 'include'), '-Rpass-analysis=kernel-resource-usage', '-c', src,
                              '-o', os.path.join(tmp, 'play.o')], capture_output=True, text=True)
    keep = ('Function Name', 'SGPRs:', 'VGPRs:', 'AGPRs', 'ScratchSize', 'Occupancy', 'Spill', 'LDS Size')
    lines = [l.split('remark: ', 1)[1].replace(' [-Rpass-analysis=kernel-resource-usage]', '')
             for l in res.stderr.splitlines() if 'remark: ' in l and any(k in l for k in keep)]
    return lines or ['not measured (the compiler printed no remarks)']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', default=','.join(CONFIGS))
    ap.add_argument('--skip-resources', action='store_true')
    args = ap.parse_args()
    text = ['Players: `player.fused` on against off, steps per second (tools/bench_play.py: one process, the two settings',
            f'alternating, median of {args.rounds} rounds of {args.steps} steps, host clock around a device synchronise).',
            'policy: get_action / get_masked_action alone; run(): policy step + synthetic env step + episode accounting.',
            'entries: library entries of one eager step (torch\'s own launches are not counted).', '']
    slower = []
    if torch.cuda.is_available():
        text.append(f'{"configuration":46s} {"mode":13s} {"policy fused":>13s} {"policy torch":>13s} {"ratio":>6s} '
                    f'{"run() fused":>12s} {"run() torch":>12s} {"ratio":>6s} {"entries f/t":>11s}')
        for name in args.only.split(','):
            for title, mode, step, run, counts in bench(name, args.steps, args.rounds):
                text.append(f'{title:46s} {mode:13s} {step[True]:13.0f} {step[False]:13.0f} {step[True] / step[False]:6.2f} '
                            f'{run[True]:12.0f} {run[False]:12.0f} {run[True] / run[False]:6.2f} '
                            f'{counts[True][0]:5d}/{counts[False][0]:<5d}')
                text.append(f'    fused entries: {", ".join(counts[True][1])}')
                if '4,096' in title and (step[True] < step[False] or run[True] < run[False]):
                    slower.append(f'{title}, {mode}')
                print(text[-2], flush=True)
        text += ['', 'fused slower than `fused: False` of the same build at 4,096 envs: ' + ('; '.join(slower) or 'nowhere')]
    else:
        text.append('timing: not measured (no GPU)')
    text += ['', 'csrc/play.hip, -Rpass-analysis=kernel-resource-usage (gfx950):']
    text += ['not measured (--skip-resources)'] if args.skip_resources else ['  ' + l.strip() for l in resource_lines()]
    with open(OUT, 'w') as f:
        f.write('\n'.join(text) + '\n')
    print(f'wrote {OUT}')


if __name__ == '__main__':
    main()
