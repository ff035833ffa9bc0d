"""An iterative planner's rollout: candidates drawn from a plan distribution (swb_rollout_guided) against clicks on uniformly
chosen sprites (swb_rollout_sampled, SWB_SAMPLE_ON_SPRITE) of the same build, and the CEM loop built on it.

Default: for each workload at N environments, M candidates of K steps, called on the engine so that the shipped workloads serve:
  sprite        Engine.rollout_sampled(SAMPLE_ON_SPRITE, seed, M, K, positions=True)                  -- the route there was
  guided        Engine.rollout_guided(seed, M, K, cdf, mean, std, positions=True), random weights     -- swb_rollout_guided
  guided_nocdf  ... choice_cdf None (the uniform fallback)
timed as tools/rollout_random_bench.py times its legs: after warm-up, `--calls` back-to-back repetitions between ONE pair of
device events, divided by the repetitions; `--rounds` such windows of each, the order rotating; median, fastest and slowest.
One JSON line per configuration.  SWB_LIBRARY names another build of the library (a register budget to compare).

--cem: one BatchedEnvironment.plan_cem(M, K, iterations=I) against I rollout_random(click='sprite') calls followed by
episode_return().max(1) -- the same number of candidates scored --, timed the same way, one window of `--calls` each per round.
--quality: planning quality at equal budget: the mean over environments of the incumbent's return after I x M guided
candidates (plan_cem) against the best of I * M sprite-click random candidates (one rollout_random of I * M), over `--seeds`.

  python tools/rollout_guided_bench.py [--shapes 1024x64x16,8192x16x8] [--workloads goal_s5,embodied_s12] [--calls 20] [--rounds 5]
  python tools/rollout_guided_bench.py --cem [--iterations 4] ...
  python tools/rollout_guided_bench.py --quality [--shapes 1024x64x16] [--workloads goal_s5] [--iterations 4] [--seeds 4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.rollout_bench import window  # noqa: E402
from tools.rollout_random_bench import started  # noqa: E402


def environment_over(eng):
  """A BatchedEnvironment's planner methods over an engine of a shipped workload (they use the engine, the action seed and the
  environment offset only)."""
  from spriteworld_amd import environment
  env = object.__new__(environment.BatchedEnvironment)
  env._engine, env._num_envs, env._global_env_offset = eng, eng.N, 0  # pylint: disable=protected-access
  env.seed_actions(1)
  return env


def summary(times):
  f = lambda ts: {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
  return {key + '_ms': f(ts) for key, ts in times.items()}


def timed(fns, calls, rounds):
  for _ in range(3):
    for fn in fns.values():
      fn()
  torch.cuda.synchronize()
  times = {key: [] for key in fns}
  order = list(fns)
  for r in range(rounds):
    for key in order[r % len(order):] + order[:r % len(order)]:
      times[key].append(window(fns[key], calls))
  return times


def run(name, n, m, k, calls, rounds):
  from spriteworld_amd import _abi
  cfg, pool, sample, rng, eng = started(name, n)
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  width = 8 if embodied else eng.S
  gen = torch.Generator(device=eng.device).manual_seed(5)
  cdf = torch.rand((k, n, width), dtype=torch.float64, device=eng.device, generator=gen).cumsum(-1)
  mean = std = None
  if not embodied:
    mean = torch.rand((k, n, 2), dtype=torch.float64, device=eng.device, generator=gen)
    std = torch.full((k, n, 2), 0.25, dtype=torch.float64, device=eng.device)
  seed = [0]

  def next_seed():
    seed[0] += 1
    return seed[0]

  fns = {'sprite': lambda: eng.rollout_sampled(_abi.SAMPLE_ON_SPRITE, next_seed(), m, k, positions=True),
         'guided': lambda: eng.rollout_guided(next_seed(), m, k, choice_cdf=cdf, motion_mean=mean, motion_std=std, positions=True),
         'guided_nocdf': lambda: eng.rollout_guided(next_seed(), m, k, motion_mean=mean, motion_std=std, positions=True)}
  times = timed(fns, calls, rounds)
  med = {key: statistics.median(ts) for key, ts in times.items()}
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'build_id': eng.variant()['build_id'], 'library': os.environ.get('SWB_LIBRARY', '')}
  out.update(summary(times))
  out.update({'guided_over_sprite': round(med['guided'] / med['sprite'], 3), 'guided_nocdf_over_sprite': round(med['guided_nocdf'] / med['sprite'], 3)})
  out['error'] = int(fns['guided']()['error'].any().item())
  eng.close()
  return out


def cem(name, n, m, k, iterations, calls, rounds):
  cfg, pool, sample, rng, eng = started(name, n)
  env = environment_over(eng)

  def shooting():
    best = None
    for _ in range(iterations):
      r, actions = env.rollout_random(m, k, click='sprite')
      top = r.episode_return().max(1).values
      best = top if best is None else torch.maximum(best, top)
    return best

  fns = {'plan_cem': lambda: env.plan_cem(m, k, iterations=iterations), 'random_shooting': shooting}
  times = timed(fns, max(calls // iterations, 1), rounds)
  med = {key: statistics.median(ts) for key, ts in times.items()}
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'iterations': iterations, 'build_id': eng.variant()['build_id']}
  out.update(summary(times))
  out['plan_cem_over_random_shooting'] = round(med['plan_cem'] / med['random_shooting'], 3)
  eng.close()
  return out


def quality(name, n, m, k, iterations, seeds):
  cfg, pool, sample, rng, eng = started(name, n)
  env = environment_over(eng)
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'iterations': iterations, 'seeds': seeds, 'build_id': eng.variant()['build_id']}
  guided, per_round, shot = [], [], []
  for s in range(seeds):
    env.seed_actions(100 + s)
    plan = env.plan_cem(m, k, iterations=iterations)
    guided.append(float(plan.episode_return.mean().item()))
    per_round.append([round(float(v), 4) for v in plan.best_per_iteration.mean(0).tolist()])
    env.seed_actions(100 + s)
    r, actions = env.rollout_random(m * iterations, k, click='sprite')
    shot.append(float(r.episode_return().max(1).values.mean().item()))
  out.update({'plan_cem_mean_return': round(statistics.mean(guided), 4), 'plan_cem_min_max_over_seeds': [round(min(guided), 4), round(max(guided), 4)],
              'plan_cem_mean_best_per_iteration': per_round,
              'random_shooting_mean_best_return': round(statistics.mean(shot), 4),
              'random_shooting_min_max_over_seeds': [round(min(shot), 4), round(max(shot), 4)]})
  eng.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='1024x64x16,8192x16x8', help='N x M x K, comma separated')
  ap.add_argument('--workloads', default='goal_s5,embodied_s12')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--cem', action='store_true')
  ap.add_argument('--quality', action='store_true')
  ap.add_argument('--iterations', type=int, default=4)
  ap.add_argument('--seeds', type=int, default=4)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('rollout_guided_bench.py needs a GPU: a timing taken on the CPU says nothing about it')
  for name in args.workloads.split(','):
    for shape in args.shapes.split(','):
      n, m, k = (int(v) for v in shape.split('x'))
      if args.quality:
        line = quality(name, n, m, k, args.iterations, args.seeds)
      elif args.cem:
        line = cem(name, n, m, k, args.iterations, args.calls, args.rounds)
      else:
        line = run(name, n, m, k, args.calls, args.rounds)
      print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
