"""Pure-Python restatement of swb_rollout_sampled's draws (rollout_drawer<true>, spriteworld_amd/csrc/swb_sampler.hip.inc).

Test infrastructure.  The Philox function is tests/_sampler_model.py's, the bounding-box arithmetic and the containment test
are tests/_random_agent_model.py's (`contained_from_uniforms`, `oracle_sprites`: geometry and containment from the oracle);
what is added here is the fourth counter word (1 + candidate) and a stream that outlives a step -- one per virtual
environment for the K steps of a rollout -- and the walk that feeds it: an oracle.Engine per candidate, stepped with the
actions drawn so far.
"""
import numpy as np

from spriteworld_amd import _abi
from tests import _random_agent_model
from tests import _sampler_model

M32 = _sampler_model.M32


class CandidateStream(object):
  """Philox4x32-10, key = seed, counter = (entry lo, block, entry hi, 1 + candidate)."""

  def __init__(self, seed, entry, candidate):
    self.key = (seed & M32, (seed >> 32) & M32)
    self.entry, self.entry_hi, self.word3, self.block, self.buf = entry & M32, (entry >> 32) & M32, (1 + candidate) & M32, 0, []

  def u32(self):
    if not self.buf:
      self.buf = list(_sampler_model.philox4x32_10((self.entry, self.block, self.entry_hi, self.word3), self.key))
      self.block += 1
    return self.buf.pop(0)

  def uniform(self):
    a, b = self.u32() >> 5, self.u32() >> 6
    return (a * 67108864.0 + b) / 9007199254740992.0


def _uniforms(stream):
  while True:
    yield stream.uniform()


def draw_step(rng, mode, cfg, sprites):
  """One step's draw of one virtual environment from its running stream, in swb_sample_actions' order for the mode:
  (actions, sprite, tries); sprite / tries are None in the uniform mode.  sprites: tests/_random_agent_model.oracle_sprites."""
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  sprite = tries = None
  head = None
  if mode == _abi.SAMPLE_ON_SPRITE:
    n = len(sprites)
    if n == 0:
      sprite, tries, head = -1, 0, (rng.uniform(), rng.uniform())
    else:
      sprite = rng.u32() % n
      s = sprites[sprite]
      head, tries = _random_agent_model.contained_from_uniforms(s['pos'], s['path'], s['contains'], _uniforms(rng))
  elif not embodied:
    head = (rng.uniform(), rng.uniform())
  if embodied:
    actions = np.array([rng.u32() % 2, rng.u32() % 4], np.int32)
  else:
    actions = np.array([head[0], head[1], rng.uniform(), rng.uniform()], np.float64)
    if cfg.action_is_f32:
      actions = actions.astype(np.float32)
  return actions, sprite, tries


def rollout(cfg, pool, live, seed, first_env, mode, n_cand, n_steps, reset_after_live=False):
  """The model's rollout: (drawn, want).  drawn: actions [K, N, M, A] in the handle's action dtype, sprite, tries i32[K, N, M]
  (-9 in the uniform mode), pos_x, pos_y f64[K, N, M, S] -- the positions every draw was taken on -- and shape_of, (k, n, m) ->
  (shape, scale, angle) of the chosen sprite.  want: the oracle's
  outputs stepped with those actions, as tests/_rollout_cases.reference returns them, plus per-step x_steps, y_steps
  [K, N, M, S] and n_sprites_steps [K, N, M]."""
  from oracle import oracle
  n, s = cfg.n_envs, cfg.max_sprites
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  width = 2 if embodied else 4
  a_dtype = np.int32 if embodied else (np.float32 if cfg.action_is_f32 else np.float64)
  drawn = {'actions': np.zeros((n_steps, n, n_cand, width), a_dtype), 'sprite': np.full((n_steps, n, n_cand), -9, np.int32),
           'tries': np.full((n_steps, n, n_cand), -9, np.int32), 'pos_x': np.zeros((n_steps, n, n_cand, s)),
           'pos_y': np.zeros((n_steps, n, n_cand, s)), 'shape_of': {}}
  want = {'reward': np.zeros((n_steps, n, n_cand)), 'discount': np.zeros((n_steps, n, n_cand), np.float32),
          'step_type': np.zeros((n_steps, n, n_cand), np.uint8), 'success': np.zeros((n_steps, n, n_cand), np.uint8),
          'error': np.zeros((n, n_cand), np.uint8), 'x': np.zeros((n, n_cand, s)), 'y': np.zeros((n, n_cand, s)),
          'n_sprites': np.zeros((n, n_cand), np.int32), 'x_steps': np.zeros((n_steps, n, n_cand, s)),
          'y_steps': np.zeros((n_steps, n, n_cand, s)), 'n_sprites_steps': np.zeros((n_steps, n, n_cand), np.int32)}
  for m in range(n_cand):
    ora = oracle.Engine(cfg, pool)
    for a in live:
      ora.step(a, render=False)
    if reset_after_live:
      ora.reset_all()
    streams = [CandidateStream(seed, first_env + e, m) for e in range(n)]

    def draw(e, k, st):
      sprites = None
      if mode == _abi.SAMPLE_ON_SPRITE:
        sprites = _random_agent_model.oracle_sprites(ora, e, int(st['n_sprites'][e]), st['x'], st['y'])
      act, sprite, tries = draw_step(streams[e], mode, cfg, sprites)
      drawn['actions'][k, e, m] = act
      drawn['pos_x'][k, e, m], drawn['pos_y'][k, e, m] = st['x'][e], st['y'][e]
      if sprite is not None:
        drawn['sprite'][k, e, m], drawn['tries'][k, e, m] = sprite, tries
        if sprite >= 0:
          sp = ora.get_sprite(e, sprite)
          drawn['shape_of'][(k, e, m)] = (sp['shape'], sp['scale'], sp['angle'])

    st = ora.state()
    for k in range(n_steps):
      resets = st['reset_next'] != 0
      for e in np.flatnonzero(~resets):         # a running episode: the step acts on the sprites as they are
        draw(int(e), k, st)
      out = ora.step(drawn['actions'][k, :, m], render=False)
      st = ora.state()
      for e in np.flatnonzero(resets):          # a FIRST step: the fresh episode's sprites, which the step did not move
        assert out['step_type'][e] == _abi.STEP_FIRST
        draw(int(e), k, st)
      for f in ('reward', 'discount', 'step_type', 'success'):
        want[f][k, :, m] = out[f]
      want['error'][:, m] |= out['error']
      want['x_steps'][k, :, m], want['y_steps'][k, :, m], want['n_sprites_steps'][k, :, m] = st['x'], st['y'], st['n_sprites']
    want['x'][:, m], want['y'][:, m], want['n_sprites'][:, m] = st['x'], st['y'], st['n_sprites']
  return drawn, want
