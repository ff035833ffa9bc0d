"""The quick-start loop of a random agent, with the actions drawn on the host and on the device.

On the headline scene (cluster_s5 as configs/cobra/clustering.py draws it: 2 + 3 sprites in two hue clusters, 64 x 64,
anti_aliasing 5, SelectMove) as a `BatchedEnvironment`, at each batch size of --envs:
  host     env.step(env.sample_actions())                                  numpy on the host, uploaded by every step
  device   env.step(env.sample_actions(where='device'))                    swb_sample_actions, uniform
  sprite   env.step(env.sample_actions(where='device', click='sprite'))    ... the click inside a randomly chosen sprite
A window is --steps timed steps after --warmup, between host clocks around work that ends in a device synchronise (the host
loop's cost IS host time); --rounds windows per loop, the loops alternating; env-steps/s as median [min, max] over the rounds.
The sampling kernel's own time is taken from one pair of device events around --kernel-calls back-to-back calls.
One JSON line per batch size.  A tree without the device forms (--tree: another checkout of this package, e.g. the parent
commit, built in place) runs the host loop only: alternate the two trees in one session to compare them.

  python tools/random_agent_bench.py [--envs 8192,1024] [--steps 20] [--warmup 5] [--rounds 7] [--tree DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--envs', default='8192,1024')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--kernel-calls', type=int, default=200)
ap.add_argument('--tree', default=None, help='root of the checkout whose spriteworld_amd is measured (default: this one)')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spriteworld_amd import _abi, action_spaces, engine, environment, renderers, sprite_generators, tasks  # noqa: E402
from spriteworld_amd import factor_distributions as distribs  # noqa: E402


def headline_env(n_envs):
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.13]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  clusters = [distribs.Continuous('c0', 0.55, 0.65), distribs.Continuous('c0', 0.27, 0.37)]
  gen = sprite_generators.shuffle(sprite_generators.chain_generators(
      sprite_generators.generate_sprites(distribs.Product(common + [clusters[0]]), num_sprites=2),
      sprite_generators.generate_sprites(distribs.Product(common + [clusters[1]]), num_sprites=3)))
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  return environment.BatchedEnvironment(task=tasks.Clustering(clusters, terminate_bonus=0., reward_range=10.),
                                        action_space=action_spaces.SelectMove(scale=0.25), renderers=rend, init_sprites=gen,
                                        max_episode_length=50, num_envs=n_envs, episodes_per_env=4, seed=3, check_errors=0)


def window(env, draw, steps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    env.step(draw())
  torch.cuda.synchronize()
  return time.perf_counter() - t0


def kernel_ms(env, mode, calls):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(5):
    env.engine.sample_actions(mode, 1)
  torch.cuda.synchronize()
  e0.record()
  for k in range(calls):
    env.engine.sample_actions(mode, k)
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / calls


def run(n_envs):
  env = headline_env(n_envs)
  np.random.seed(0)
  env.reset()
  loops = {'host': lambda: env.sample_actions()}
  on_device = hasattr(engine.Engine, 'sample_actions')
  if on_device:
    env.seed_actions(0)
    loops['device'] = lambda: env.sample_actions(where='device')
    loops['sprite'] = lambda: env.sample_actions(where='device', click='sprite')
  for draw in loops.values():
    window(env, draw, args.warmup)
  rates = {k: [] for k in loops}
  order = list(loops)
  for r in range(args.rounds):
    for k in (order if r % 2 == 0 else order[::-1]):
      window(env, loops[k], args.warmup)
      rates[k].append(n_envs * args.steps / window(env, loops[k], args.steps))
  err = int(env.engine.error.max().item())
  f = lambda v: {'median': round(statistics.median(v)), 'min': round(min(v)), 'max': round(max(v))}
  line = {'tree': os.path.relpath(ROOT), 'build_id': env.engine.variant()['build_id'], 'n_envs': n_envs, 'steps': args.steps,
          'warmup': args.warmup, 'rounds': args.rounds, 'env_steps_per_s': {k: f(v) for k, v in rates.items()}, 'error': err}
  if on_device:
    line['sample_kernel_ms'] = {'uniform': round(kernel_ms(env, _abi.SAMPLE_UNIFORM, args.kernel_calls), 5),
                                'on_sprite': round(kernel_ms(env, _abi.SAMPLE_ON_SPRITE, args.kernel_calls), 5)}
    tries = env.sample_contained_positions().tries
    line['on_sprite_mean_tries'] = round(float(tries.double().mean().item()), 3)
    line['on_sprite_max_tries'] = int(tries.max().item())
  env.close()
  return line


if __name__ == '__main__':
  if not torch.cuda.is_available():
    sys.exit('random_agent_bench.py needs a GPU: a timing taken on the CPU says nothing about it')
  for n in (int(v) for v in args.envs.split(',')):
    print(json.dumps(run(n)), flush=True)
