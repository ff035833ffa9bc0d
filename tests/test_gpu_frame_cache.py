"""The frame cache on the GPU: the scripts of tests/_frame_cache_cases.py against the oracle at every step, with swb_frame_stats
and swb_list_stats held to what a model of the header word implies."""
import numpy as np
import pytest

from tests import _frame_cache_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def test_never_hit(monkeypatch):
  cases.never_hit(_gpu, monkeypatch, 40)


def test_hit_every_step(monkeypatch):
  cases.hit_every_step(_gpu, monkeypatch, 33)


def test_scripted(monkeypatch):
  cases.scripted(_gpu, monkeypatch, 37)


def test_episode_ends(monkeypatch):
  cases.episode_ends(_gpu, monkeypatch, 33)


def test_caller_scribbles(monkeypatch):
  cases.scripted(_gpu, monkeypatch, 37, what='caller_scribbles', scribble=True)


def test_alternating_buffers(monkeypatch):
  cases.alternating_buffers(_gpu, monkeypatch, 33)


@pytest.mark.parametrize('which', cases.BETWEEN)
def test_calls_between(monkeypatch, which):
  cases.call_between(_gpu, monkeypatch, 33, which)


@pytest.mark.parametrize('which', cases.GEOMETRIES)
def test_geometries(monkeypatch, which):
  cases.geometry(_gpu, monkeypatch, 16 if which == 'band_tasks_8' else 37, which)


def test_switches(monkeypatch):
  cases.switches(_gpu, monkeypatch, 37)


@pytest.mark.parametrize('paint', (False, True))
def test_anti_aliasing_1(monkeypatch, paint):
  cases.anti_aliasing_1(_gpu, monkeypatch, 33, paint)


def test_one_band_at_full_size(monkeypatch):
  """8192 environments take one band by themselves (the headline's geometry): six steps of the headline workload, byte for
  byte against a second handle created with SWB_NO_FRAME_CACHE.  No oracle: the small cases hold the frames to it."""
  import torch
  from spriteworld_amd import engine, workloads
  monkeypatch.setenv('SWB_LIST_STATS', '1')
  cfg, pool, sample = workloads.build('cluster_s5', 8192, episodes_per_env=2, seed=1, anti_aliasing=5)
  a = engine.Engine(cfg, pool)
  monkeypatch.setenv('SWB_NO_FRAME_CACHE', '1')
  b = engine.Engine(cfg, pool)
  assert a.variant()['n_bands'] == 1 and a.variant()['frame_cache_bytes'] == 8192 * 64 * 64 * 3 and b.variant()['frame_cache_bytes'] == 0
  rng = np.random.default_rng(5)
  for t in range(6):
    act = torch.as_tensor(sample(rng), device=a.device)
    a.obs.fill_(0xA5)
    a.step(act)
    b.step(act)
    assert torch.equal(a.obs, b.obs), t
    assert torch.equal(a.reward.nan_to_num(), b.reward.nan_to_num()) and not bool(a.error.any())
  copied, filled, resampled = a.frame_stats()
  assert copied > 0 and filled > 0 and copied + filled + resampled == 6 * 8192
  assert copied + filled == a.list_stats()[0]            # every kept list was filled from or copied
  assert b.frame_stats() == (0, 0, 6 * 8192) and b.list_stats() == a.list_stats()
  a.close()
  b.close()
