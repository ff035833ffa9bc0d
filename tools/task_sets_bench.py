"""What a step of a batch that mixes tasks costs (task sets), against what users did before:

  mix          goal_s5 + cluster_s5 + sorting_s4 in ONE handle of `--n` environments: entry k of environment n plays set
               (n + k) mod 3.  Every workload runs with episodes of `--episode` steps (goal_s5's own 20 would leave it a sixth of
               the steps): random clicks rarely end an episode early, so the three residue classes n mod 3 change task together
               and each set holds about a third of the batch at every step.  `share_of_sets` is the mean, over the timed
               windows, of the shares `task_sets()` shows at the end of each.
  alone_<w>    each of the three workloads alone at `--n` environments (the same episode length) in a handle without task sets: the expectation to test
               is that the mix costs no more than the most expensive of them.
  three_handles  three handles of `--n` / 3 environments, one per workload, each on a stream of its own (what
               `EnvironmentGroups` does): a "step" is one step of each.
Per figure `--steps` steps between ONE pair of device events, divided by the steps; `--rounds` such windows after a warm-up,
median / min / max; 16 seeded action tensors taken in turn.  One JSON line per figure.

  python tools/task_sets_bench.py [--n 8192] [--aa 5] [--steps 40] [--rounds 6] [--warmup 10] [--seed 0]
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

NAMES = ('goal_s5', 'cluster_s5', 'sorting_s4')


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
  ap.add_argument('--aa', type=int, default=5)
  ap.add_argument('--steps', type=int, default=40)
  ap.add_argument('--rounds', type=int, default=6)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--episode', type=int, default=50)
  args = ap.parse_args()
  from spriteworld_amd import engine, workloads
  n = args.n

  def timed(step, after_window=None):
    for i in range(args.warmup):
      step(i)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
      ts.append(window(step, args.steps))
      if after_window is not None:
        after_window()
    return spread(ts)

  def actions(sample, device, seed):
    rng = np.random.default_rng(seed)
    return [torch.as_tensor(sample(rng), device=device) for _ in range(16)]

  base = {'n_envs': n, 'anti_aliasing': args.aa, 'seed': args.seed}
  # the mix in one handle
  cfg, sets, pool, sample = workloads.build_task_sets(NAMES, n, episodes_per_env=4, seed=args.seed, anti_aliasing=args.aa,
                                                      max_episode_lengths=(args.episode,) * 3)
  eng = engine.Engine(cfg, pool, task_sets=sets)
  base['build_id'] = eng.variant()['build_id']
  acts = actions(sample, eng.device, args.seed + 2000)
  shares = []
  ms = timed(lambda i: eng.step(acts[i % 16]),
             lambda: shares.append(np.bincount(eng.task_sets().cpu().numpy(), minlength=3) / float(n)))
  print(json.dumps(dict(base, what='mix', ms=ms, share_of_sets=[round(float(v), 3) for v in np.mean(shares, axis=0)])), flush=True)
  assert not int(eng.error.max().item()), 'error flags'
  eng.close()
  # each workload alone
  for g, name in enumerate(NAMES):
    cfg, pool, sample = workloads.build(name, n, episodes_per_env=4, seed=args.seed + g, anti_aliasing=args.aa)
    cfg.max_episode_length = args.episode
    eng = engine.Engine(cfg, pool)
    acts = actions(sample, eng.device, args.seed + 2000)
    print(json.dumps(dict(base, what='alone_' + name, ms=timed(lambda i: eng.step(acts[i % 16])))), flush=True)
    assert not int(eng.error.max().item()), 'error flags'
    eng.close()
  # three handles of a third of the batch, on three streams
  per = n // 3
  streams = [torch.cuda.Stream() for _ in NAMES]
  engines, acts3 = [], []
  for g, name in enumerate(NAMES):
    cfg, pool, sample = workloads.build(name, per, episodes_per_env=4, seed=args.seed + g, anti_aliasing=args.aa)
    cfg.max_episode_length = args.episode
    with torch.cuda.stream(streams[g]):
      engines.append(engine.Engine(cfg, pool))
    acts3.append(actions(sample, engines[g].device, args.seed + 2000))
  torch.cuda.synchronize()

  def step3(i):
    for g, e in enumerate(engines):
      with torch.cuda.stream(streams[g]):
        e.step(acts3[g][i % 16])

  def window3(calls):      # (the events sit on the default stream: it waits for the three, and they for it)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in streams:
      s.wait_stream(torch.cuda.current_stream())
    for i in range(calls):
      step3(i)
    for s in streams:
      torch.cuda.current_stream().wait_stream(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls

  for i in range(args.warmup):
    step3(i)
  torch.cuda.synchronize()
  print(json.dumps(dict(base, what='three_handles', n_envs_each=per, ms=spread([window3(args.steps) for _ in range(args.rounds)]))),
        flush=True)
  for e in engines:
    assert not int(e.error.max().item()), 'error flags'
    e.close()


if __name__ == '__main__':
  main()
