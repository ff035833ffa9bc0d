"""Throughput of the many-sprite path (handles of more than 16 sprites: swb_ms_state_kernel + the large-frame render kernels).

Scenes of S sprites (squares, triangles, 30-gon circles and four-pointed stars of scales 0.05 .. 0.1 on a 64x64 image, a
FindGoalPosition task on a third of them, SelectMove actions), every episode holding all S sprites.  For each S, anti_aliasing
and batch size: warm-up steps, then a synchronised window of `--steps` steps timed with one pair of device events; then a
diagnostic run with the engine's own events splits a step into its state kernel and its render kernels.  S = 16 is the same
scene on the tuned path (cover + resample / fill kernels), for comparison.  One JSON line per configuration.

  python tools/many_sprites_bench.py [--steps 20] [--warmup 5] [--n 1024,8192] [--sprites 16,24,40,64] [--aa 1,5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def scene(S, n, aa, episodes_per_env=2, seed=1):
  from spriteworld_amd import action_spaces, lowering, renderers, synthetic, tasks
  rng = np.random.default_rng(seed)
  P = n * episodes_per_env
  task = tasks.FindGoalPosition(filter_distrib=None, terminate_distance=0.1)
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=aa, color_to_rgb=renderers.hsv_to_rgb)}
  labels = [[int(i % 3 == 0)] for i in range(S)]
  pool = synthetic.make_pool(rng, P, S, [(0.0, 1.0)] * S, labels, shape_names=('square', 'triangle', 'circle', 'star_4'),
                             scales=(0.05, 0.1), xy_range=(0.05, 0.95))
  cfg = lowering.lower_config(task, action_spaces.SelectMove(scale=0.25), rend, True, 50, n, S, True)
  pool.assign_round_robin(n, episodes_per_env)

  def sample(r):
    return r.uniform(0.0, 1.0, size=(n, 4))
  return cfg, pool, sample


def gpu_run(S, aa, n, steps, warmup):
  from spriteworld_amd import engine
  cfg, pool, sample = scene(S, n, aa)
  eng = engine.Engine(cfg, pool)
  info = eng.variant()
  rng = np.random.default_rng(3)
  acts = [torch.as_tensor(sample(rng)).to(eng.device) for _ in range(4)]
  for i in range(warmup):
    eng.step(acts[i % 4])
  torch.cuda.synchronize(eng.device)
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for i in range(steps):
    eng.step(acts[i % 4])
  e1.record()
  torch.cuda.synchronize(eng.device)
  ms = e0.elapsed_time(e1) / steps
  eng.timing(True)
  for i in range(min(steps, 10)):
    eng.step(acts[i % 4])
  state, render, launches = eng.kernel_times_ms()
  eng.timing(False)
  err = int(eng.outputs_host()['error'].any())
  eng.close()
  return {'ms_per_step': round(ms, 4), 'env_steps_per_s': round(n * 1e3 / ms, 0),
          'state_ms': round(state / max(launches, 1), 4), 'render_ms': round(render / max(launches, 1), 4),
          'many_sprites': int(info['many_sprites']), 'state_kernel': info.get('state_kernel', info['cover_kernel']),
          'render_kernel': info['kernel'], 'error': err}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--n', default='1024,8192')
  ap.add_argument('--sprites', default='16,24,40,64')
  ap.add_argument('--aa', default='1,5')
  args = ap.parse_args()
  for aa in (int(v) for v in args.aa.split(',')):
    for S in (int(v) for v in args.sprites.split(',')):
      for n in (int(v) for v in args.n.split(',')):
        line = {'sprites': S, 'image': '64x64', 'anti_aliasing': aa, 'n_envs': n}
        line.update(gpu_run(S, aa, n, args.steps, args.warmup))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
