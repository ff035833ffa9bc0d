"""A random-shooting planner's rollout, with the candidate actions made by torch and drawn in the rollout kernel.

For each workload at N environments, M candidates of K steps (what BatchedEnvironment.rollout / rollout_random run, called on
the engine so that the shipped workloads serve):
  a  torch_rand   torch.rand([N, M, K, 4], float64), permuted to [K, N, M, 4], Engine.rollout(positions=True)  -- the route there
                  was: swb_rollout on a generated tensor (SelectMove / DragAndDrop only: torch.rand draws no Embodied actions)
  b  uniform      Engine.rollout_sampled(SAMPLE_UNIFORM, seed, M, K, positions=True)     -- swb_rollout_sampled
  c  sprite       Engine.rollout_sampled(SAMPLE_ON_SPRITE, ...)                          -- ... every click inside a sprite
  d  premade      Engine.rollout(actions, positions=True) on a tensor made outside the window -- the plain swb_rollout alone
The calls are timed as a user makes them (result tensors allocated inside the window).  All are timed the same way: after
warm-up, `--calls` back-to-back repetitions between ONE pair of device events, divided by the repetitions; `--rounds` such
windows of each, the order rotating, of which the median, the fastest and the slowest are reported.  One JSON line per
configuration.  On a library without swb_rollout_sampled (SWB_LIBRARY: a build of an older revision) only a and d are measured.

--planner: instead of timing, what the two modes give a planner at equal M and K, one JSON line per workload: the share of
non-FIRST candidate steps that moved a sprite (positions after the step differ from those before it; the shipped pools have
no velocities, so only a hit moves anything) and the mean over environments of episode_return().max(1), over `--seeds` calls.

  python tools/rollout_random_bench.py [--shapes 1024x64x16,8192x16x8] [--workloads goal_s5,embodied_s12] [--calls 20] [--rounds 5]
  python tools/rollout_random_bench.py --planner [--shapes 1024x64x16] [--workloads goal_s5] [--seeds 4]
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


def started(name, n, warm_steps=6):
  from spriteworld_amd import engine, workloads
  rng = np.random.default_rng(1)
  cfg, pool, sample = workloads.build(name, n, episodes_per_env=2, seed=3)
  eng = engine.Engine(cfg, pool)
  for _ in range(warm_steps):                          # a few steps into the episodes
    eng.step(sample(rng), render=False)
  return cfg, pool, sample, rng, eng


def run(name, n, m, k, calls, rounds):
  from spriteworld_amd import _abi
  cfg, pool, sample, rng, eng = started(name, n)
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  draws = hasattr(eng.lib, 'swb_rollout_sampled')
  acts = torch.as_tensor(np.stack([np.stack([sample(rng) for _ in range(m)], axis=1) for _ in range(k)], axis=0)).to(eng.device)
  seed = [0]

  def next_seed():
    seed[0] += 1
    return seed[0]

  fns = {'premade': lambda: eng.rollout(acts, positions=True)}
  if not embodied:
    fns['torch_rand'] = lambda: eng.rollout(torch.rand((n, m, k, 4), dtype=torch.float64, device=eng.device).permute(2, 0, 1, 3),
                                            positions=True)
  if draws:
    fns['uniform'] = lambda: eng.rollout_sampled(_abi.SAMPLE_UNIFORM, next_seed(), m, k, positions=True)
    fns['sprite'] = lambda: eng.rollout_sampled(_abi.SAMPLE_ON_SPRITE, next_seed(), m, k, positions=True)
  for _ in range(3):
    for fn in fns.values():
      fn()
  torch.cuda.synchronize()
  times = {key: [] for key in fns}
  order = list(fns)
  for r in range(rounds):
    for key in order[r % len(order):] + order[:r % len(order)]:
      times[key].append(window(fns[key], calls))
  err = int(eng.rollout(acts)['error'].any().item())
  f = lambda ts: {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
  med = {key: statistics.median(ts) for key, ts in times.items()}
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'build_id': eng.variant()['build_id']}
  out.update({key + '_ms': f(ts) for key, ts in times.items()})
  base = 'premade' if embodied else 'torch_rand'
  if draws:
    out.update({'uniform_over_' + base: round(med['uniform'] / med[base], 3), 'sprite_over_' + base: round(med['sprite'] / med[base], 3)})
  out['error'] = err
  eng.close()
  return out


def planner(name, n, m, k, seeds):
  """What the modes give a planner: moved share and best return, accumulated over `seeds` calls of each mode."""
  from spriteworld_amd import _abi, environment
  cfg, pool, sample, rng, eng = started(name, n)
  st = eng.state()
  live = [torch.as_tensor(st[f]).to(eng.device) for f in ('x', 'y')]
  out = {'workload': name, 'n_envs': n, 'M': m, 'K': k, 'seeds': seeds, 'build_id': eng.variant()['build_id'],
         'pool_has_velocities': bool(pool.x_vel.any() or pool.y_vel.any())}
  for label, mode in (('uniform', _abi.SAMPLE_UNIFORM), ('sprite', _abi.SAMPLE_ON_SPRITE)):
    moved = steps = 0
    best = []
    for s in range(seeds):
      res = eng.rollout_sampled(mode, 1000 + s, m, k, positions=True, keep_steps=True)
      xs, ys = res['x_steps'], res['y_steps']                                 # [K, N, M, S] after step k + 1
      before_x = torch.cat([live[0][None, :, None, :].expand(1, n, m, -1), xs[:-1]])
      before_y = torch.cat([live[1][None, :, None, :].expand(1, n, m, -1), ys[:-1]])
      changed = ((xs != before_x) | (ys != before_y)).any(dim=3)
      counted = res['step_type'] != _abi.STEP_FIRST
      moved += int((changed & counted).sum().item())
      steps += int(counted.sum().item())
      per_step = [res[f].permute(1, 2, 0) for f in ('step_type', 'reward', 'discount', 'success')]
      r = environment.Rollout(*(per_step + [res['x'], res['y'], res['n_sprites'], res['error']]))
      best.append(float(r.episode_return().max(1).values.mean().item()))
    out[label] = {'moved_share_of_non_first_steps': round(moved / steps, 4), 'non_first_steps': steps,
                  'mean_best_episode_return': round(statistics.mean(best), 4),
                  'best_return_min_max_over_seeds': [round(min(best), 4), round(max(best), 4)]}
  eng.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='1024x64x16,8192x16x8', help='N x M x K, comma separated')
  ap.add_argument('--workloads', default='goal_s5,embodied_s12')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--planner', action='store_true')
  ap.add_argument('--seeds', type=int, default=4)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('rollout_random_bench.py needs a GPU: a timing taken on the CPU says nothing about it')
  for name in args.workloads.split(','):
    for shape in args.shapes.split(','):
      n, m, k = (int(v) for v in shape.split('x'))
      line = planner(name, n, m, k, args.seeds) if args.planner else run(name, n, m, k, args.calls, args.rounds)
      print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
