"""One swb_rollout against what a user could do without it: a second engine of N * M environments taking K steps.

For each workload, M (candidates per environment) and K (steps per candidate), at N environments:
  rollout   Engine(N).rollout(actions[K, N, M, A])      -- swb_rollout_fork_kernel + swb_rollout_kernel, one call
  baseline  Engine(N * M).step(actions[N * M, A], render=False), K times -- the state phase of the step kernels, K launches
            (where one handle cannot hold N * M environments -- its run lists are limited to 4 GB -- two handles of half as
            many, and so on, stepped one after the other)
            (the baseline is not charged for getting the live state into the second engine: swb_get_state / swb_set_positions
            go through the host and cannot carry step counts, episodes or pool entries at all)
Both are timed the same way: after warm-up, `--calls` back-to-back repetitions between ONE pair of device events, divided by
the repetitions; `--rounds` such windows, alternating the two, of which the median, the fastest and the slowest are reported.
One JSON line per configuration.

  python tools/rollout_bench.py [--n 1024] [--m 16,64] [--k 4,16] [--workloads goal_s5,embodied_s12] [--calls 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

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


def run(name, n, m, ks, calls, rounds, warm_steps=6):
  """One result dict per K in `ks`; the two engines are built once."""
  from spriteworld_amd import _lib, engine, workloads
  rng = np.random.default_rng(1)
  cfg, pool, sample = workloads.build(name, n, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  parts = 1
  while True:                                          # the fewest handles that hold N * M environments between them
    bcfg, bpool, bsample = workloads.build(name, n * m // parts, episodes_per_env=2, seed=3)
    bases = [engine.Engine(bcfg, bpool) for _ in range(parts)]
    try:
      for base in bases:
        base.step(bsample(rng), render=False)
      break
    except _lib.SwbError as e:
      if 'step fewer environments per engine' not in str(e):
        raise
      for base in bases:
        base.close()
      parts *= 2
  for _ in range(warm_steps):                          # all engines a few steps into their episodes
    eng.step(sample(rng), render=False)
    for base in bases:
      base.step(bsample(rng), render=False)
  out = []
  for k in ks:
    out.append(_measure(name, n, m, k, calls, rounds, eng, bases, sample, bsample, rng))
  eng.close()
  for base in bases:
    base.close()
  return out


def _measure(name, n, m, k, calls, rounds, eng, bases, sample, bsample, rng):
  acts = torch.as_tensor(np.stack([np.stack([sample(rng) for _ in range(m)], axis=1) for _ in range(k)], axis=0)).to(eng.device)
  bacts = [torch.as_tensor(bsample(rng)).to(eng.device) for _ in range(k)]

  def rollout():
    eng.rollout(acts)

  def baseline():
    for base in bases:
      for a in bacts:
        base.step(a, render=False)

  for _ in range(3):
    rollout()
    baseline()
  torch.cuda.synchronize()
  t_roll, t_base = [], []
  for r in range(rounds):
    for which in ((rollout, baseline) if r % 2 == 0 else (baseline, rollout)):
      (t_roll if which is rollout else t_base).append(window(which, calls))
  res = eng.rollout(acts)
  err = int(res['error'].any().item()) | int(any(base.outputs_host()['error'].any() for base in bases))
  info = eng.variant()
  f = lambda ts: {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
  return {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'rollout_ms': f(t_roll), 'baseline_ms': f(t_base),
          'baseline_over_rollout': round(statistics.median(t_base) / statistics.median(t_roll), 2),
          'candidate_steps_per_s': round(n * m * k * 1e3 / statistics.median(t_roll), 0),
          'baseline_handles': len(bases), 'baseline_state_kernel': info.get('state_kernel', info['cover_kernel']), 'error': err}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1024)
  ap.add_argument('--m', default='16,64')
  ap.add_argument('--k', default='4,16')
  ap.add_argument('--workloads', default='goal_s5,embodied_s12')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  args = ap.parse_args()
  for name in args.workloads.split(','):
    for m in (int(v) for v in args.m.split(',')):
      for line in run(name, args.n, m, [int(v) for v in args.k.split(',')], args.calls, args.rounds):
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
