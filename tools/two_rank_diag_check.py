"""Launched by torch.distributed.run with RLG_TEST_SINGLE_GPU=1 (2 ranks on one GPU): a small continuous agent with
multi_gpu and use_diagnostics trains a few epochs; rank 0 must hold PpoDiagnostics with every key, the other rank
DefaultDiagnostics, and both ranks must end with bit-identical parameters."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch.distributed as dist  # noqa: E402

from rl_games_amd import configs  # noqa: E402
from rl_games_amd.agent import A2CAgent  # noqa: E402
from rl_games_amd.diagnostics import DefaultDiagnostics, PpoDiagnostics  # noqa: E402

rank = int(os.environ['RANK'])
torch.manual_seed(100 + rank)
params = configs.tiny(num_actors=64, horizon=8, multi_gpu=True, use_diagnostics=True)
params['config']['env_config']['seed'] = 10 + rank
agent = A2CAgent('diag_ranks', params)
agent.init_tensors()
agent.obs = agent.env_reset()
agent.broadcast_parameters()
keys = []
for e in range(3):
    agent.update_epoch()
    agent.train_epoch()
    if agent.global_rank == 0:
        agent.diagnostics.epoch(agent, current_epoch=e)
        keys = sorted(agent.diagnostics.diag_dict)
kind_ok = (type(agent.diagnostics) is PpoDiagnostics) if rank == 0 else (type(agent.diagnostics) is DefaultDiagnostics)
want = sorted([f'diagnostics/clip_frac/{m}' for m in range(agent.mini_epochs_num)] + ['diagnostics/exp_var'] +
              (['diagnostics/rms_value/mean', 'diagnostics/rms_value/var'] if agent.normalize_value else []))
keys_ok = keys == want if rank == 0 else True
finite_ok = all(bool(torch.isfinite(v).all()) for v in agent.diagnostics.diag_dict.values()) if rank == 0 else True
p = torch.stack([agent.optimizer.flat_params.double().sum(), agent.optimizer.flat_params.double().abs().sum()])
lo, hi = p.clone(), p.clone()
dist.all_reduce(lo, op=dist.ReduceOp.MIN)
dist.all_reduce(hi, op=dist.ReduceOp.MAX)
ok = kind_ok and keys_ok and finite_ok and bool(torch.equal(lo, hi))
flag = torch.tensor([0.0 if ok else 1.0], device=agent.ppo_device)
dist.all_reduce(flag, op=dist.ReduceOp.MAX)
if rank == 0:
    sys.stdout.write(f'TWO_RANK_DIAG {"ok" if flag.item() == 0 else "FAIL"} kind={kind_ok} keys={keys} '
                     f'sync={bool(torch.equal(lo, hi))}\n')
    sys.stdout.flush()
dist.barrier()
dist.destroy_process_group()
sys.exit(0 if flag.item() == 0 else 1)
