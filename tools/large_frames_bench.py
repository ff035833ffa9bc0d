"""Throughput of the large-frame render path (canvases wider than 640 px, images wider than 256 columns).

For each scene (workloads.build('geom_<S>x<S>'), four sprites of scales 0.1 .. 0.4) and batch size: warm-up steps, then a
synchronised window of `--steps` steps timed with one pair of device events; prints one JSON line with steps per second,
frames per second and milliseconds per step, and the CPU oracle's time per frame on the same scene (one thread).

  python tools/large_frames_bench.py [--steps 20] [--warmup 5] [--n 64,1024] [--scenes 256:10,256:5,512:1,128:8]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def oracle_ms_per_frame(size, aa, frames=4):
  from oracle import oracle
  from spriteworld_amd import workloads
  cfg, pool, sample = workloads.build('geom_%dx%d' % (size, size), frames, episodes_per_env=2, seed=1, anti_aliasing=aa)
  ora = oracle.Engine(cfg, pool)
  rng = np.random.default_rng(3)
  ora.step(sample(rng))
  a = sample(rng)
  t0 = time.perf_counter()
  ora.step(a)
  return (time.perf_counter() - t0) * 1e3 / frames


def gpu_run(size, aa, n, steps, warmup):
  from spriteworld_amd import engine, workloads
  cfg, pool, sample = workloads.build('geom_%dx%d' % (size, size), n, episodes_per_env=2, seed=1, anti_aliasing=aa)
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
  # the split of a step: cover kernel (state phase) / render kernels, from the engine's own events (a diagnostic run)
  eng.timing(True)
  for i in range(min(steps, 10)):
    eng.step(acts[i % 4])
  cover, render, launches = eng.kernel_times_ms()
  eng.timing(False)
  err = int(eng.outputs_host()['error'].any())
  eng.close()
  return {'ms_per_step': round(ms, 4), 'steps_per_s': round(1e3 / ms, 1), 'frames_per_s': round(n * 1e3 / ms, 0),
          'state_phase_ms': round(cover / max(launches, 1), 4), 'render_ms': round(render / max(launches, 1), 4),
          'large_frames': int(info['large_frames']), 'kernel': info['kernel'], 'error': err}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--n', default='64,1024')
  ap.add_argument('--scenes', default='256:10,256:5,512:1,128:8')
  ap.add_argument('--no-oracle', action='store_true')
  args = ap.parse_args()
  ns = [int(v) for v in args.n.split(',')]
  for sc in args.scenes.split(','):
    size, aa = (int(v) for v in sc.split(':'))
    ora_ms = None if args.no_oracle else round(oracle_ms_per_frame(size, aa), 2)
    for n in ns:
      line = {'image': '%dx%d' % (size, size), 'anti_aliasing': aa, 'canvas': aa * size, 'n_envs': n}
      line.update(gpu_run(size, aa, n, args.steps, args.warmup))
      line['oracle_ms_per_frame'] = ora_ms
      if ora_ms:
        line['speedup_vs_oracle_frame'] = round(ora_ms / (1e3 / line['frames_per_s']), 1)
      print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
