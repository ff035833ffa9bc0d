"""bench.py's plain run (N = 1) and --dump-outputs, run unattended on the CPU with the kernel source executed on the host in
place of the HIP engine (tests/_bench_dry_run.py).  Asserted: a plain run times exactly --steps steps and does nothing beside
the headline (no oracle check, no kernel split, no extras, no CPU baseline); --full still does them; the dumped arrays are the
outputs of the last timed step -- the oracle replayed through the same inputs gives them bit for bit --, in float32 / float64,
and the same in both modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, STEPS, WARMUP = 8, 3, 2


def _bench():
  import importlib.util
  spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _run(extra_args, timeout=600):
  from tests.emu import build_emu
  build_emu.build()
  env = dict(os.environ, OMP_NUM_THREADS='1', PYTHONPATH=ROOT)
  for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
    env.pop(k, None)
  cmd = [sys.executable, os.path.join(ROOT, 'tests', '_bench_dry_run.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup',
         str(WARMUP), '--envs-per-gpu', str(ENVS), '--ramp-ms', '1'] + list(extra_args)
  proc = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
  assert proc.returncode == 0, proc.stderr[-2000:]
  lines = [l for l in proc.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, proc.stdout[-2000:]
  return json.loads(lines[0])


def _load(d):
  return {os.path.splitext(f)[0]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _oracle_last_step():
  """The headline's inputs (SURVEY 8d protocol, cluster_s5, anti_aliasing 5) replayed through the oracle: W warm-up steps,
  then K timed ones, the action sets cycled from 0 in both -> the outputs of the last step."""
  from oracle import oracle
  from spriteworld_amd import workloads
  bench = _bench()
  cfg, pool, actions_of_step = workloads.build_protocol_8d('cluster_s5', ENVS, 4, 5, env_offset=0, total_envs=ENVS)
  acts = [actions_of_step(t) for t in range(bench.N_ACTION_SETS)]
  ora = oracle.Engine(cfg, pool)
  out = None
  for k in (WARMUP, STEPS):
    for i in range(k):
      out = ora.step(acts[i % bench.N_ACTION_SETS])
  return out


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
  d = _run(['--dump-outputs', str(tmp_path / 'out')])
  for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
    assert key in d, key
  assert d['steps'] == STEPS and d['warmup'] == WARMUP and d['full'] is False
  assert abs(d['value'] - ENVS * STEPS / (d['ms_per_step'] * STEPS / 1e3)) / d['value'] < 1e-9
  for key in ('verified_envs', 'mismatches', 'extra', 'cpu_baseline'):          # --full only
    assert key not in d, key
  assert all(k['ms'] is None for k in d['roofline']['kernels']) and 'kernel_ms' in d['roofline']
  got = _load(str(tmp_path / 'out'))
  assert sorted(got) == sorted(d['outputs_dumped']) == ['discount', 'discount_is_none', 'obs', 'obs_env_index', 'reward',
                                                       'reward_is_none', 'step_type', 'success']
  assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
  idx = got['obs_env_index'].astype(np.int64)
  assert np.array_equal(idx, np.arange(ENVS))                      # a batch this small: every environment's frame
  _util.check_dump_against(got, _oracle_last_step(), idx)


def test_full_run_checks_and_times_the_kernels_apart_and_dumps_the_same_outputs(tmp_path):
  plain = _run(['--dump-outputs', str(tmp_path / 'plain')])
  full = _run(['--full', '--no-extra', '--no-cpu-baseline', '--dump-outputs', str(tmp_path / 'full')])
  assert full['full'] is True and full['steps'] == STEPS
  assert full['verified_envs'] == ENVS and full['mismatches'] == 0
  assert all(k['ms'] is not None for k in full['roofline']['kernels'])
  a, b = _load(str(tmp_path / 'plain')), _load(str(tmp_path / 'full'))
  assert sorted(a) == sorted(b)
  for name in a:
    assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name], equal_nan=True), name
  assert 'outputs_dumped' in plain


def test_dump_of_a_large_batch_is_a_fixed_sample_within_64_mb():
  torch = pytest.importorskip('torch')
  bench = _bench()

  class Outputs(object):
    def __init__(self, n, shape):
      self.obs_shape = shape
      self.obs = (torch.arange(n) % 251).to(torch.uint8).view((n,) + (1,) * len(shape)).expand((n,) + shape).contiguous()
      self.reward = torch.arange(n, dtype=torch.float64) / 7
      self.discount = torch.ones(n, dtype=torch.float32)
      self.reward[::5] = float('nan')                       # FIRST steps: the reference's None
      self.discount[::5] = float('nan')
      self.step_type = torch.full((n,), 1, dtype=torch.uint8)
      self.success = torch.zeros(n, dtype=torch.uint8)

  for n, shape in ((5000, (64, 64, 3)), (300, (128, 128, 3)), (300000, (8, 8, 3))):
    eng = Outputs(n, shape)
    a, b = bench.outputs_to_dump(eng, n), bench.outputs_to_dump(eng, n)
    assert sum(x.nbytes for x in a.values()) <= 64 * 10**6, (n, shape)
    idx = a['obs_env_index'].astype(np.int64)
    assert len(idx) == min(n, bench.DUMP_OBS_BYTES // (4 * int(np.prod(shape)))) and np.all(np.diff(idx) > 0)
    per_env = slice(None) if n <= bench.DUMP_ALL_ENVS_UP_TO else idx
    assert a['reward'].shape[0] == (n if n <= bench.DUMP_ALL_ENVS_UP_TO else len(idx))
    _util.check_dump_against(a, {k: getattr(eng, k).numpy()[per_env] if k != 'obs' else eng.obs.numpy()
                           for k in ('obs', 'reward', 'discount', 'step_type', 'success')}, idx)
    assert a['reward_is_none'].any() and a['discount_is_none'].any()
    for k in a:
      assert np.array_equal(a[k], b[k]), k                         # the same sample every time
