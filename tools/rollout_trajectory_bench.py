"""swb_rollout_trajectory and swb_rollout_step_frames -- a rollout that keeps the state after every step, and the K frames of a
picked candidate -- against what there was before: swb_rollout, and K rollouts of K' = 1 .. K steps each followed by a picked
swb_rollout_frames.

For each workload, M (candidates per environment) and K (steps per candidate), at N environments:
  rollout       Engine(N).rollout(actions[K, N, M, A])                       -- swb_rollout
  trajectory    Engine(N).rollout(actions, keep_steps=True)                  -- swb_rollout_trajectory; trajectory / rollout is
                what keeping the steps costs
  plan_frames   Engine(N).rollout_frames(cand[N], step='all')                -- swb_rollout_pick_steps_kernel + K render launches,
                after one trajectory rollout made outside the window
  plan          trajectory, then plan_frames                                 -- the K frames of a picked candidate, the new way
  old_way       for K' in 1 .. K: rollout(actions[:K']), rollout_frames(cand) -- the same K frames, the only way there was
  pick_one      Engine(N).rollout_frames(cand[N])                            -- one picked chunk; K x pick_one is what the K render
                launches of plan_frames cost on their own
The calls are timed as a user makes them (the result tensors are allocated inside the window).  All are timed the same way:
after warm-up, `--calls` back-to-back repetitions between ONE pair of device events, divided by the repetitions; `--rounds` such
windows of each, the order rotating, of which the median, the fastest and the slowest are reported.  One JSON line per
configuration.  On a library without swb_rollout_trajectory (SWB_LIBRARY: a build of an older revision) only `rollout`,
`old_way` and `pick_one` are measured.

  python tools/rollout_trajectory_bench.py [--n 1024] [--m 16,64] [--k 4,16] [--workloads goal_s5,embodied_s12] [--calls 20] [--rounds 5]
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


def run(name, n, m, ks, calls, rounds, warm_steps=6):
  """One result dict per K in `ks`; the engine is built once."""
  from spriteworld_amd import engine, workloads
  rng = np.random.default_rng(1)
  cfg, pool, sample = workloads.build(name, n, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  for _ in range(warm_steps):                          # a few steps into the episodes, run lists trimmed
    eng.step(sample(rng))
  keeps = hasattr(eng.lib, 'swb_rollout_trajectory')
  cand = torch.as_tensor(rng.integers(0, m, size=n).astype(np.int32)).to(eng.device)
  info = eng.variant()
  for k in ks:
    acts = torch.as_tensor(np.stack([np.stack([sample(rng) for _ in range(m)], axis=1) for _ in range(k)], axis=0)).to(eng.device)
    prefixes = [acts[:kk].contiguous() for kk in range(1, k + 1)]

    def old_way():
      for a in prefixes:
        eng.rollout(a)
        eng.rollout_frames(cand)

    def plan():
      eng.rollout(acts, keep_steps=True)
      eng.rollout_frames(cand, step='all')

    # name -> (what runs before the window, outside the events; what is timed)
    plain = lambda: eng.rollout(acts)
    fns = {'rollout': (None, plain), 'old_way': (None, old_way), 'pick_one': (plain, lambda: eng.rollout_frames(cand))}
    if keeps:
      keep = lambda: eng.rollout(acts, keep_steps=True)
      fns.update({'trajectory': (None, keep), 'plan': (None, plan), 'plan_frames': (keep, lambda: eng.rollout_frames(cand, step='all'))})
    for _ in range(3):
      for setup, fn in fns.values():
        if setup:
          setup()
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in fns}
    order = list(fns)
    for r in range(rounds):
      for key in order[r % len(order):] + order[:r % len(order)]:
        setup, fn = fns[key]
        if setup:
          setup()
        times[key].append(window(fn, calls))
    err = 0
    if keeps:
      res = eng.rollout(acts, keep_steps=True)
      err = int(res['error'].any().item()) | int(eng.rollout_frames(cand, step='all')['error'].any().item())
    f = lambda ts: {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
    med = {key: statistics.median(ts) for key, ts in times.items()}
    out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'build_id': info['build_id']}
    out.update({key + '_ms': f(ts) for key, ts in times.items()})
    if keeps:
      out.update({'trajectory_over_rollout': round(med['trajectory'] / med['rollout'], 3),
                  'old_way_over_plan': round(med['old_way'] / med['plan'], 2),
                  'plan_frames_over_K_pick_one': round(med['plan_frames'] / (k * med['pick_one']), 3)})
    out.update({'kernels': '%s + %s' % (info['cover_kernel'], info['kernel']), 'error': err})
    yield out
  eng.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1024)
  ap.add_argument('--m', default='16,64')
  ap.add_argument('--k', default='4,16')
  ap.add_argument('--workloads', default='goal_s5,embodied_s12')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  args = ap.parse_args()
  ks = [int(v) for v in args.k.split(',')]
  for name in args.workloads.split(','):
    for m in (int(v) for v in args.m.split(',')):
      for out in run(name, args.n, m, ks, args.calls, args.rounds):
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
