"""Task sets on the emulated kernel (tests/emu, CPU): the scripts of tests/_task_sets_cases.py against one oracle per set at
every step.  A handful of environments each."""
import pytest

from tests import _task_sets_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def _error():
  from tests import _emu_engine
  return _emu_engine.EmuError


@pytest.mark.parametrize('which', sorted(cases.SCENES))
def test_against_the_oracles(monkeypatch, which):
  cases.against_the_oracles(_emu, monkeypatch, which, gpu=False)


def test_with_a_live_setter(monkeypatch):
  cases.with_setter(_emu, monkeypatch, gpu=False)


def test_with_an_active_mask(monkeypatch):
  cases.with_mask(_emu, monkeypatch, gpu=False)


def test_null_steps_reuse_task_records(monkeypatch):
  cases.null_steps_reuse_records(_emu, monkeypatch, gpu=False)


def test_one_set_equal_to_the_config_is_the_handle_without_sets(monkeypatch):
  cases.one_set_equals_no_sets(_emu, monkeypatch, gpu=False)


def test_reassignment_in_the_middle_of_episodes(monkeypatch):
  cases.reassignment(_emu, monkeypatch, gpu=False, emu_error=_error())


def test_snapshot_loaded_into_other_environments(monkeypatch):
  cases.snapshots(_emu, monkeypatch, gpu=False)


def test_fork(monkeypatch):
  cases.fork(_emu, monkeypatch, gpu=False)


def test_refusals(monkeypatch):
  cases.refusals(_emu, monkeypatch, _error())


def test_swb_task_set_layout_matches_the_header(tmp_path):
  import ctypes
  import os
  import subprocess
  from spriteworld_amd import _abi
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  fields = [f for f, _ in _abi.SwbTaskSet._fields_]
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swb.h"\nint main(void) {\n'
                 '  printf("%zu %d\\n", sizeof(swb_task_set), SWB_MAX_TASK_SETS);\n' +
                 ''.join('  printf("%%zu\\n", offsetof(swb_task_set, %s));\n' % f for f in fields) + '  return 0;\n}\n')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbTaskSet), _abi.SWB_MAX_TASK_SETS] + [getattr(_abi.SwbTaskSet, f).offset for f in fields]
  assert ctypes.sizeof(_abi.SwbTaskSet) == 32


def test_merged_configs_split_back_into_the_workloads_own():
  """The oracle's per-set configurations (cases.split) are, byte for byte, what workloads.build gives for each workload alone --
  the expectation does not lean on the merge it checks."""
  import numpy as np
  from spriteworld_amd import lowering, workloads
  names, lengths = ('goal_s5', 'cluster_s5', 'sorting_s4'), (6, 9, 12)
  cfg, sets, pool, _ = workloads.build_task_sets(names, 5, 4, seed=0, anti_aliasing=5, max_episode_lengths=lengths)
  assert [(s.first_task, s.n_tasks, s.is_meta, s.max_episode_length) for s in sets] == [(0, 1, 0, 6), (1, 1, 0, 9), (2, 4, 1, 12)]
  assert pool.task_set.reshape(5, 4).tolist() == [[(n + k) % 3 for k in range(4)] for n in range(5)]
  for g, (c, pg) in enumerate(cases.split(cfg, sets, pool)):
    own_cfg, own_pool, _ = workloads.build(names[g], 5, 4, g, 5)
    own_cfg.max_episode_length, own_cfg.max_sprites = lengths[g], 5
    assert bytes(c) == bytes(own_cfg), names[g]
    mine = np.flatnonzero(pool.task_set == g)
    S = own_pool.max_sprites
    assert np.array_equal(pg.x[:, :S], own_pool.x[mine]) and np.array_equal(pg.label[:, :, :S], own_pool.label[mine])
    assert (pg.label[:, :, S:] == 0).all() and np.array_equal(pg.n_sprites, own_pool.n_sprites[mine])
  with pytest.raises(lowering.LoweringError, match='image_h'):
    workloads.build_task_sets(('goal_s5', 'embodied_s12'), 4)
  with pytest.raises(lowering.LoweringError, match='sub-tasks'):
    workloads.build_task_sets(('sorting_s4', 'sorting_s4', 'goal_s5'), 4)
  assert lowering.task_set_assignment('per_env', 4, 3, 3).tolist() == [[0] * 3, [1] * 3, [2] * 3, [0] * 3]
  with pytest.raises(lowering.LoweringError):
    lowering.task_set_assignment(np.full((4, 3), 3), 4, 3, 3)
