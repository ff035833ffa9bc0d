"""Reset sampling of generators the legacy device sampler refuses: swb_sample_pool_tree against the host route.

  (a) 65 536 entries of the `hue_filter` and `pos_goal` generators of tests/_sampler_tree_cases.py through swb_sample_pool_tree:
      device events around each of 20 calls (after 3 warm-up calls), the median;
  (b) the same generators through what such generators took before the tree sampler, host `refill_pool()` (init_sprites() per
      episode, lowering, upload): one timed call;
  (c) the cobra-like generator of tests/_sampler_cases.py through the legacy kernel and, wrapped in a TreeSampler, through the
      tree kernel: the same 20-call medians, the calls of the two kernels alternating.

Prints one JSON line.  python tools/sampler_tree_bench.py [--envs 8192] [--episodes-per-env 8] [--no-host]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from spriteworld_amd import action_spaces, device_sampler, environment, sprite_generators
from tests import _sampler_cases
from tests import _sampler_tree_cases as cases


def _median_ms(calls, repeats=20, warmup=3):
  """Median device time of `repeats` rounds, per call of `calls` (alternating inside a round)."""
  times = [[] for _ in calls]
  for r in range(warmup + repeats):
    for i, call in enumerate(calls):
      start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      call()
      end.record()
      end.synchronize()
      if r >= warmup:
        times[i].append(start.elapsed_time(end))
  return [float(np.median(t)) for t in times], [[float(min(t)), float(max(t))] for t in times]


def _env(init, task, rend, n, k, **kwargs):
  return environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend, init_sprites=init,
                                        num_envs=n, episodes_per_env=k, refresh_every=0, check_errors=0, **kwargs)


def _host_generator(case):
  """The generator of a case as a sprite_generators closure (what a config hands the environment)."""
  init, task, rend = cases.CASES[case]()
  if isinstance(init, device_sampler.TreeSampler):
    (dist, lo, hi), = init.groups
    count = lambda: np.random.randint(3, 6)
    assert (lo, hi) == (3, 5)
    init = sprite_generators.generate_sprites(dist, count)
    init = sprite_generators.shuffle(init)
  return init, task, rend


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=8192)
  ap.add_argument('--episodes-per-env', type=int, default=8)
  ap.add_argument('--no-host', action='store_true')
  args = ap.parse_args()
  n, k = args.envs, args.episodes_per_env
  P = n * k
  base, length = np.arange(n, dtype=np.int32) * k, np.full(n, k, np.int32)
  out = {'entries': P, 'device': torch.cuda.get_device_name(0)}
  for case in ('hue_filter', 'pos_goal'):
    gen, task, rend = _host_generator(case)
    env = _env(gen, task, rend, n, k, device_reset='tree', seed=1)
    assert isinstance(env._sampler, device_sampler.TreeSampler)
    eng, spec, seeds = env.engine, env._sampler_spec, iter(range(1, 1000))
    (ms,), (spread,) = _median_ms([lambda: eng.sample_pool_tree(spec, P, base, length, next(seeds))])
    assert eng.sampler_exhausted() == 0
    print(case, 'tree %.3f ms' % ms, file=sys.stderr, flush=True)
    out[case] = {'tree_ms': ms, 'tree_min_max_ms': spread, 'sprites': int(eng.get_pool().n_sprites.sum())}
    env.close()
    if not args.no_host:
      np.random.seed(0)
      env = _env(gen, task, rend, n, 1, device_reset=False, max_sprites=5)      # (the constructor draws a pool too: a small one)
      env._episodes_per_env = k
      torch.cuda.synchronize()
      t = time.time()
      env.refill_pool()
      torch.cuda.synchronize()
      out[case]['host_refill_s'] = time.time() - t
      out[case]['host_over_tree'] = out[case]['host_refill_s'] * 1e3 / ms
      env.close()
  legacy, task, rend = _sampler_cases._cobra_like()
  tree = device_sampler.TreeSampler([(dist, (lo, hi + 1)) for dist, lo, hi, _ in legacy.groups], shuffle=True, seed=7)
  env = _env(legacy, task, rend, n, k)
  eng, seeds = env.engine, iter(range(1, 1000))
  spec_legacy, spec_tree = legacy.lower(task, rend), tree.lower(task, rend)
  (a, b), spreads = _median_ms([lambda: eng.sample_pool(spec_legacy, P, base, length, next(seeds)),
                                lambda: eng.sample_pool_tree(spec_tree, P, base, length, next(seeds))])
  out['cobra_like'] = {'legacy_ms': a, 'tree_ms': b, 'tree_over_legacy': b / a, 'min_max_ms': spreads}
  env.close()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
