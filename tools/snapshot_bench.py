"""What snapshots cost (swb_save_state, swb_load_state, swb_copy_pool), and what the step after a load costs.

  save, load   `--calls` back-to-back calls on pre-allocated tensors between ONE pair of device events, divided by the calls;
               `--rounds` such windows, median / min / max.  Bytes moved: each state is read once and written once.
  yardstick    Engine.rollout of M candidates, K = 1, at N / M environments: the fork launch moves the same arrays for the
               same number of states, and one step of the rollout kernel follows it (the two are not separated here: read
               swb_rollout_fork_kernel from a kernel trace of this tool for the launch alone).
  fork         N0 environments forked `--copies` times at the engine level: a second Engine of N0 * copies, copy_pool_from,
               one save, one load; wall clock with a device synchronisation at the end, the creation of the engine apart.
  next step    one rendering step, device events around it, after: a load of every environment / set_positions of every
               environment (both rebuild every list) / a load of one environment in 16 / nothing (an undisturbed still step).
One JSON line per figure.  Run it in three processes and take the median of their medians.

  python tools/snapshot_bench.py [--n 8192] [--fork-n 1024] [--copies 64] [--workload goal_s5] [--calls 20] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def window(fn, calls):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(calls):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / calls


def spread(ts):
  return {'median': round(statistics.median(ts), 5), 'min': round(min(ts), 5), 'max': round(max(ts), 5)}


def still(n):
  return torch.full((n, 4), 0.5, dtype=torch.float64, device='cuda')


def save_and_load(name, n, calls, rounds):
  from spriteworld_amd import _abi, engine, workloads
  cfg, pool, sample = workloads.build(name, n, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  rng = np.random.default_rng(1)
  for _ in range(4):
    eng.step(sample(rng))
  snap = eng.save_state()
  cs, pid = snap.as_struct(), snap.pool_id
  per_state = 16 * eng.S + 6 * 4 + 1
  save = lambda: eng._check(eng.lib.swb_save_state(eng._h, _abi.STATE_LIVE, None, n, C.byref(cs), eng._stream()))
  load = lambda: eng._check(eng.lib.swb_load_state(eng._h, C.byref(cs), n, None, C.c_uint64(pid), None, eng._stream()))
  for what, fn in (('save_state', save), ('load_state', load)):
    for _ in range(3):
      fn()
    ts = [window(fn, calls) for _ in range(rounds)]
    moved = 2 * n * per_state
    print(json.dumps({'what': what, 'workload': name, 'n_envs': n, 'ms': spread(ts), 'bytes_moved': moved,
                      'GB_per_s': round(moved / statistics.median(ts) / 1e6, 1)}), flush=True)
  eng.close()


def yardstick(name, n, m, calls, rounds):
  from spriteworld_amd import engine, workloads
  cfg, pool, sample = workloads.build(name, n // m, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  rng = np.random.default_rng(1)
  for _ in range(4):
    eng.step(sample(rng), render=False)
  acts = torch.as_tensor(np.stack([sample(rng) for _ in range(m)], axis=1)[None]).to(eng.device)
  fn = lambda: eng.rollout(acts)
  for _ in range(3):
    fn()
  ts = [window(fn, calls) for _ in range(rounds)]
  print(json.dumps({'what': 'rollout_K1 (fork launch + one step of the rollout kernel)', 'workload': name, 'n_envs': n // m, 'M': m,
                    'states': n, 'ms': spread(ts)}), flush=True)
  eng.close()


def fork(name, n0, copies, rounds):
  from spriteworld_amd import engine, workloads
  cfg, pool, sample = workloads.build(name, n0, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  rng = np.random.default_rng(1)
  for _ in range(4):
    eng.step(sample(rng))
  big = type(cfg).from_buffer_copy(cfg)
  big.n_envs = n0 * copies
  base, length = np.repeat(pool.pool_base, copies), np.repeat(pool.pool_len, copies)
  slots = torch.arange(n0 * copies, device=eng.device, dtype=torch.int32) // copies
  create, transfer = [], []
  for _ in range(rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    child = engine.Engine(big, None)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    child.copy_pool_from(eng, base, length)
    child.load_state(eng.save_state(), slots)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    create.append((t1 - t0) * 1e3)
    transfer.append((t2 - t1) * 1e3)
    child.step(still(n0 * copies))        # (it steps and renders)
    assert not child.outputs_host()['error'].any()
    child.close()
  print(json.dumps({'what': 'fork', 'workload': name, 'n_envs': n0, 'copies': copies, 'create_engine_ms': spread(create),
                    'copy_pool_save_load_ms': spread(transfer), 'pool_entries': int(pool.n_entries)}), flush=True)
  eng.close()


def next_step(name, n, rounds):
  from spriteworld_amd import engine, workloads
  cfg, pool, sample = workloads.build(name, n, episodes_per_env=2, seed=3)
  cfg.max_episode_length = 1 << 20
  eng = engine.Engine(cfg, pool)
  rng = np.random.default_rng(1)
  for _ in range(4):
    eng.step(sample(rng))
  a = still(n)
  for _ in range(4):
    eng.step(a)                            # every environment still: lists kept, frames copied
  snap = eng.save_state()
  st = eng.state()
  one_in_16 = torch.where(torch.arange(n, device=eng.device) % 16 == 0, torch.arange(n, device=eng.device), -1)

  def timed(prepare):
    ts = []
    for _ in range(rounds):
      eng.step(a)
      eng.step(a)
      prepare()
      ts.append(window(lambda: eng.step(a), 1))
    return spread(ts)

  for what, prepare in (('step after a load of every environment', lambda: eng.load_state(snap)),
                        ('step after set_positions of every environment', lambda: eng.set_positions(st['x'], st['y'])),
                        ('step after a load of one environment in 16', lambda: eng.load_state(snap, one_in_16)),
                        ('undisturbed still step', lambda: None)):
    print(json.dumps({'what': what, 'workload': name, 'n_envs': n, 'ms': timed(prepare)}), flush=True)
  eng.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=8192)
  ap.add_argument('--fork-n', type=int, default=1024)
  ap.add_argument('--copies', type=int, default=64)
  ap.add_argument('--workload', default='goal_s5')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  args = ap.parse_args()
  save_and_load(args.workload, args.n, args.calls, args.rounds)
  save_and_load(args.workload, args.fork_n * args.copies, args.calls, args.rounds)
  yardstick(args.workload, args.n, 8, args.calls, args.rounds)
  yardstick(args.workload, args.fork_n * args.copies, args.copies, args.calls, args.rounds)
  fork(args.workload, args.fork_n, args.copies, args.rounds)
  next_step(args.workload, args.n, args.rounds)


if __name__ == '__main__':
  main()
