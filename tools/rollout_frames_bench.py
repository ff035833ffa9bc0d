"""swb_rollout_frames -- the frames of a rollout's N * M end states, drawn in M chunks of N -- against one swb_render of the
same number of frames.

For each workload and M (candidates per environment), at N environments and K steps per candidate:
  rollout      Engine(N).rollout(actions[K, N, M, A])                          -- for scale
  frames_all   Engine(N).rollout_frames()          -- M render launches of N environments on the rollout's scratch state
  frames_pick  Engine(N).rollout_frames(cand[N])   -- swb_rollout_pick_kernel + one render launch of N environments
  render       Engine(N * M).render()              -- the same number of frames as frames_all in ONE launch (where one handle
               cannot hold N * M environments -- its run lists are limited to 4 GB -- two handles of half as many, and so on,
               one after the other); not charged for getting the candidates' states into that engine, which nothing offers
frames_all / render is what rendering in chunks of N costs.  The calls are timed as a user makes them: rollout_frames
allocates its two output tensors inside the window, render reuses the engine's frame buffer.  All are timed the same way:
after warm-up, `--calls` back-to-back repetitions between ONE pair of device events, divided by the repetitions; `--rounds`
such windows of each, the order rotating, of which the median, the fastest and the slowest are reported.  One JSON line per
configuration.

  python tools/rollout_frames_bench.py [--n 1024] [--m 16,64] [--k 1] [--workloads goal_s5,embodied_s12] [--calls 20] [--rounds 5]
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

from tools.rollout_bench import window  # noqa: E402


def run(name, n, m, k, calls, rounds, warm_steps=6):
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
        base.step(bsample(rng))
      break
    except _lib.SwbError as e:
      if 'step fewer environments per engine' not in str(e):
        raise
      for base in bases:
        base.close()
      parts *= 2
  for _ in range(warm_steps):                          # all engines a few steps into their episodes, run lists trimmed
    eng.step(sample(rng))
    for base in bases:
      base.step(bsample(rng))
  acts = torch.as_tensor(np.stack([np.stack([sample(rng) for _ in range(m)], axis=1) for _ in range(k)], axis=0)).to(eng.device)
  cand = torch.as_tensor(rng.integers(0, m, size=n).astype(np.int32)).to(eng.device)
  eng.rollout(acts)

  def render():
    for base in bases:
      base.render()

  fns = {'rollout': lambda: eng.rollout(acts), 'frames_all': eng.rollout_frames, 'frames_pick': lambda: eng.rollout_frames(cand),
         'render': render}
  for _ in range(3):
    for fn in fns.values():
      fn()
  torch.cuda.synchronize()
  times = {key: [] for key in fns}
  order = list(fns)
  for r in range(rounds):
    for key in order[r % len(order):] + order[:r % len(order)]:
      times[key].append(window(fns[key], calls))
  res = eng.rollout_frames()
  err = int(res['error'].any().item()) | int(eng.rollout_frames(cand)['error'].any().item())
  f = lambda ts: {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
  med = {key: statistics.median(ts) for key, ts in times.items()}
  info = eng.variant()
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k}
  out.update({key + '_ms': f(ts) for key, ts in times.items()})
  out.update({'frames_all_over_render': round(med['frames_all'] / med['render'], 3),
              'frames_pick_over_one_chunk': round(med['frames_pick'] / (med['frames_all'] / m), 3),
              'frames_per_s': round(n * m * 1e3 / med['frames_all'], 0), 'render_handles': len(bases),
              'kernels': '%s + %s' % (info['cover_kernel'], info['kernel']), 'error': err})
  eng.close()
  for base in bases:
    base.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1024)
  ap.add_argument('--m', default='16,64')
  ap.add_argument('--k', type=int, default=1)
  ap.add_argument('--workloads', default='goal_s5,embodied_s12')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  args = ap.parse_args()
  for name in args.workloads.split(','):
    for m in (int(v) for v in args.m.split(',')):
      print(json.dumps(run(name, args.n, m, args.k, args.calls, args.rounds)), flush=True)


if __name__ == '__main__':
  main()
