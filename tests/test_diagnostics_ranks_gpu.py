"""GPU: `use_diagnostics` with two ranks on one GPU (tools/two_rank_diag_check.py): rank 0 reports the diagnostics,
rank 1 holds DefaultDiagnostics, and the ranks stay bit-identical."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_rank0_reports_diagnostics_and_ranks_stay_in_sync():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RLG_TEST_SINGLE_GPU='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tools', 'two_rank_diag_check.py')]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert 'TWO_RANK_DIAG ok' in res.stdout, res.stdout[-2000:]
