"""What a step costs when only a part of the batch takes part in it (swb_step_masked), and what swb_reset_envs costs.

  fractions    100, 50, 10 and 0 % of the environments active: per fraction 16 seeded Bernoulli masks (device tensors, made
               before the clock starts) taken in turn with 16 seeded action tensors; `--steps` steps between ONE pair of device
               events, divided by the steps; `--rounds` such windows after a warm-up, median / min / max.  The 100 % line passes a
               mask of ones; `unmasked` is the same run through swb_step.
  all_miss     every environment clicks beside every sprite: no list is rebuilt and every frame is copied, as in a 0 %-active
               step -- which also skips the hit tests and the task.  This line needs swb_step only: run the tool with SWB_LIBRARY
               naming an older build of the library to have its figure beside this build's (the masked lines are then left out).
  reset_envs   `--calls` back-to-back swb_reset_envs calls on a mask of every third environment between one pair of events.
One JSON line per figure.  Episodes never time out during the run (max_episode_length is raised), so the fractions are what the
masks say.

  python tools/masked_step_bench.py [--n 8192] [--workload cluster_s5] [--aa 5] [--steps 40] [--rounds 5] [--warmup 10] [--seed 0]
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
  for i in range(calls):
    fn(i)
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / calls


def spread(ts):
  return {'median': round(statistics.median(ts), 5), 'min': round(min(ts), 5), 'max': round(max(ts), 5)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=8192)
  ap.add_argument('--workload', default='cluster_s5')
  ap.add_argument('--aa', type=int, default=5)
  ap.add_argument('--steps', type=int, default=40)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--calls', type=int, default=50)
  ap.add_argument('--seed', type=int, default=0)
  args = ap.parse_args()
  from spriteworld_amd import engine, workloads
  n = args.n
  cfg, pool, sample = workloads.build(args.workload, n, episodes_per_env=4, seed=args.seed, anti_aliasing=args.aa)
  cfg.max_episode_length = 1 << 20
  eng = engine.Engine(cfg, pool)
  masked = hasattr(eng.lib, 'swb_step_masked')
  rng = np.random.default_rng(args.seed + 2000)
  acts = [torch.as_tensor(sample(rng), device=eng.device) for _ in range(16)]
  base = {'workload': args.workload, 'n_envs': n, 'anti_aliasing': args.aa, 'build_id': eng.variant()['build_id'], 'seed': args.seed}

  def timed(step):
    for i in range(args.warmup):
      step(i)
    torch.cuda.synchronize()
    return spread([window(step, args.steps) for _ in range(args.rounds)])

  print(json.dumps(dict(base, what='unmasked', ms=timed(lambda i: eng.step(acts[i % 16])))), flush=True)
  if masked:
    for percent in (100, 50, 10, 0):
      masks = [torch.as_tensor((rng.random(n) < percent / 100.).astype(np.uint8), device=eng.device) for _ in range(16)]
      ms = timed(lambda i: eng.step(acts[i % 16], active=masks[i % 16]))
      print(json.dumps(dict(base, what='active_%d' % percent, active_fraction=round(float(torch.stack(masks).float().mean()), 4), ms=ms)),
            flush=True)
  miss = torch.as_tensor(np.tile([5., 5., 0.5, 0.5], (n, 1)), device=eng.device).to(acts[0].dtype)
  print(json.dumps(dict(base, what='all_miss', ms=timed(lambda i: eng.step(miss)))), flush=True)
  if masked:
    third = torch.as_tensor((np.arange(n) % 3 == 0).astype(np.uint8), device=eng.device)
    for _ in range(3):
      eng.reset_envs(third)
    ts = [window(lambda i: eng.reset_envs(third), args.calls) for _ in range(args.rounds)]
    print(json.dumps(dict(base, what='reset_envs', ms=spread(ts))), flush=True)
  assert not int(eng.error.max().item()), 'error flags'
  eng.close()


if __name__ == '__main__':
  main()
