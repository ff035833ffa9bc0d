"""The UNMODIFIED reference and the HIP engine in ONE process on the GPU node (the direct leg of the parity chain).

Everywhere else parity is transitive (reference -> oracle / golden in the build container; oracle / golden -> HIP on the
GPU box).  Here the reference's own `Environment` (`/root/reference/spriteworld/environment.py:88-108`; on the GPU box the
sourceless bytecode of exactly those modules under `oracle/_ref`, see oracle/stage_ref.py) is stepped beside
`spriteworld_amd.engine.Engine` -- the C ABI, the HIP kernels -- on the same lowered episodes and the same actions, for
every shipped config in both modes: step types, rewards, success and sprite positions bit-exact, frames +-0 (north_star
allows +-1 LSB).  The body is `tests/_reference_cases.side_by_side`, which
`tests/test_oracle_vs_reference.py` runs with the oracle and `tests/test_emulated_kernel.py` with the emulated library.
"""
import numpy as np
import pytest

from oracle import ref_harness
from tests import _parity
from tests import _reference_cases
from tests._reference_cases import CONFIGS, fresh_episodes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_harness.reference_available(),
                                 reason='neither /root/reference nor oracle/_ref (python oracle/stage_ref.py) present')]


def _engine(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def test_third_party_libraries_of_the_reference_import_here():
  """The arithmetic the reference delegates must be the versions the oracle was pinned against."""
  v = ref_harness.third_party_versions()
  assert not any(str(x).startswith('missing') for x in v.values()), v
  print('reference runs as', ref_harness.reference_kind(), 'from', ref_harness.REFERENCE_ROOT, v)


@pytest.mark.parametrize('module,mode', CONFIGS)
def test_hip_engine_equals_reference_environment(module, mode):
  _reference_cases.side_by_side(_engine, module, mode, seed=21, n_eps=30, n_steps=250)


def test_hip_engine_equals_reference_on_a_batch_of_reference_environments():
  """N = 48 reference environments (the headline scene's generators, np.random.seed(1000 + i) as SURVEY 8d prescribes)
  beside ONE batched engine launch per step."""
  ref_harness.load_reference()
  from spriteworld import environment, sprite_generators, tasks
  from spriteworld import factor_distributions as distribs
  from spriteworld import renderers as ref_renderers
  from spriteworld.configs.cobra import common
  from spriteworld_amd import engine, lowering
  N, EPS, STEPS = 48, 6, 60
  clusters = [distribs.Continuous('c0', 0.55, 0.65), distribs.Continuous('c0', 0.27, 0.37)]
  other = distribs.Product([
      distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
      distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.13]),
      distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)])
  gens = [sprite_generators.generate_sprites(distribs.Product((other, c0)), num_sprites=n) for c0, n in zip(clusters, (2, 3))]
  gen = sprite_generators.shuffle(sprite_generators.chain_generators(*gens))
  task = tasks.Clustering(clusters, terminate_bonus=0., reward_range=10.)
  aspace, rends = common.action_space(), common.renderers()
  per_env, envs = [], []
  for i in range(N):
    np.random.seed(1000 + i)
    eps = [gen() for _ in range(EPS)]
    per_env.append(eps)
    it = fresh_episodes(eps)
    envs.append(environment.Environment(task=task, action_space=aspace, init_sprites=(lambda it=it: next(it)),
                                        renderers=dict(rends, success=ref_renderers.Success()), max_episode_length=12))
  flat = [e for eps in per_env for e in eps]
  cfg = lowering.lower_config(task, aspace, rends, True, 12, N, 5, pos_is_f32=True)
  pool = lowering.lower_episodes(flat, task, rends, max_sprites=5)
  pool.pool_base = np.arange(N, dtype=np.int32) * EPS
  pool.pool_len = np.full(N, EPS, np.int32)
  eng = engine.Engine(cfg, pool)
  from spriteworld_amd import _abi
  dropped = set()        # environments in which the reference raised: compared no further (the others go on to the last step)
  for t in range(STEPS):
    acts = np.random.RandomState(2000 + t).uniform(size=(N, 4))
    eng.step(acts)
    out = eng.outputs_host()
    st = eng.state()
    for i, env in enumerate(envs):
      if i in dropped:
        continue
      try:
        ts = env.step(acts[i])
      except ZeroDivisionError:      # tasks.py:215 1. / 0. (collapsed clusters): the engine flags exactly that environment
        assert out['error'][i] & _abi.ENV_ERR_DB_ZERO, (t, i)
        dropped.add(i)
        continue
      assert not out['error'][i], (t, i)
      assert int(ts.step_type) == int(out['step_type'][i]), (t, i)
      r = np.nan if ts.reward is None else float(ts.reward)
      assert (np.isnan(r) and np.isnan(out['reward'][i])) or _parity.bits(r) == _parity.bits(out['reward'][i]), (t, i)
      assert np.array_equal(ts.observation['image'], out['obs'][i]), (t, i)
      pos = np.array([s.position for s in env._sprites], dtype=np.float64).reshape(-1, 2)
      assert np.array_equal(pos[:, 0], st['x'][i, :5]) and np.array_equal(pos[:, 1], st['y'][i, :5]), (t, i)
  assert len(dropped) < N // 4, sorted(dropped)
  eng.close()
