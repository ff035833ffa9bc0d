"""bench.py's plain run (N = 1) with --dump-outputs on the HIP engine: one line without the --full blocks, and the dumped
arrays are the last timed step's outputs -- the oracle replayed through the same inputs gives them bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ENVS, STEPS, WARMUP = 512, 6, 3


def test_plain_run_dumps_the_last_timed_step(tmp_path):
  out_dir = str(tmp_path / 'out')
  env = dict(os.environ, PYTHONPATH=ROOT)
  for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
    env.pop(k, None)
  cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP),
         '--envs-per-gpu', str(ENVS), '--ramp-ms', '20', '--dump-outputs', out_dir]
  proc = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert proc.returncode == 0, proc.stderr[-2000:]
  lines = [l for l in proc.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, proc.stdout[-2000:]
  d = json.loads(lines[0])
  assert d['steps'] == STEPS and d['env_errors'] == 0 and d['full'] is False and d['ms_per_step'] > 0
  for key in ('verified_envs', 'extra', 'cpu_baseline'):
    assert key not in d, key

  from oracle import oracle
  from spriteworld_amd import workloads
  cfg, pool, actions_of_step = workloads.build_protocol_8d('cluster_s5', ENVS, 4, 5, env_offset=0, total_envs=ENVS)
  acts = [actions_of_step(t) for t in range(16)]
  ora = oracle.Engine(cfg, pool)
  for k in (WARMUP, STEPS):
    for i in range(k):
      want = ora.step(acts[i % 16])
  got = {n: np.load(os.path.join(out_dir, n + '.npy')) for n in d['outputs_dumped']}
  from tests import _util
  _util.check_dump_against(got, want, got['obs_env_index'].astype(np.int64))
