"""The general device sampler (swb_sample_pool_tree) on the host emulation of the kernel source (tests/emu): the bodies of
tests/_sampler_tree_cases.py, which tests/test_gpu_sampler_tree.py runs on the GPU, and the malformed programs the C ABI refuses
before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from spriteworld_amd import _abi
from spriteworld_amd import environment

from tests import _emu_engine
from tests import _sampler_tree_cases as cases


@pytest.fixture(autouse=True)
def _emulated_engine(monkeypatch):
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)


@pytest.mark.parametrize('case', sorted(cases.CASES))
def test_emulated_tree_sampler_equals_the_python_model(case):
  assert sorted(cases.CASES) == ['edge_f32', 'exhaust', 'hue_clusters', 'hue_filter', 'meta_swap', 'mixture', 'nested', 'pos_goal']
  if case == 'exhaust':
    cases.pool_matches_the_model_case(case, num_envs=4, episodes_per_env=2)      # P = 8
  else:
    cases.pool_matches_the_model_case(case)


def test_emulated_tree_sampler_second_block_and_high_entry_word():
  cases.odd_sizes_case()


def test_emulated_tree_sampler_shards_reproduce_the_whole_job():
  cases.shards_case()


def test_emulated_tree_sampler_refresh_keeps_the_live_entries():
  cases.refresh_case()


@pytest.mark.parametrize('case,click', [('hue_filter', 'uniform'), ('pos_goal', 'sprite'), ('meta_swap', 'sprite')])
def test_emulated_environment_on_a_tree_sampled_pool_steps_like_the_oracle(case, click):
  cases.parity_case(case, click, seed=3)


def test_emulated_setter_on_a_tree_sampled_keyed_handle_keeps_the_cell_labels():
  cases.setter_keeps_cell_labels_case()


# ---- malformed programs, through the raw ABI
def _handle_and_spec():
  env, _, _, _ = cases.make_env('nested', num_envs=4)
  spec = _abi.SwbTreeSampler.from_buffer_copy(env._sampler_spec)
  return env, spec


def _refused(env, spec, message):
  base, length = np.zeros(4, np.int32), np.full(4, 12, np.int32)
  lib = _emu_engine.lib()
  rc = lib.swb_sample_pool_tree(env.engine._h, C.byref(spec), 12, base.ctypes.data, length.ctypes.data, C.c_uint64(1), C.c_uint64(0), None)
  assert rc == -1 and message in lib.swb_last_error().decode(), lib.swb_last_error().decode()


def test_emulated_tree_sampler_refuses_malformed_programs():
  env, spec = _handle_and_spec()
  tests_at = [i for i in range(spec.n_ops) if spec.ops[i].kind == _abi.OP_TEST]
  assert len(tests_at) == 4
  jump = _abi.SwbTreeOp(_abi.OP_JUMP, 0, 0, 0)
  # a jump out of range
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.ops[tests_at[0]] = jump
  bad.ops[tests_at[0]].a = spec.n_ops + 1
  _refused(env, bad, 'outside the program')
  # a backward JUMP
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.ops[tests_at[0]] = jump
  _refused(env, bad, 'backward JUMP')
  # a TEST that retries outside its group's program
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.ops[tests_at[0]].c = tests_at[0] + 1
  _refused(env, bad, 'TEST retries at')
  # a predicate 33 deep: 33 leaves, then 32 ANDs
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  first = bad.n_pred_nodes
  for k in range(33):
    bad.pred_nodes[first + k].op, bad.pred_nodes[first + k].leaf = _abi.PRED_LEAF, 0
  for k in range(32):
    bad.pred_nodes[first + 33 + k].op = _abi.PRED_AND
  bad.n_pred_nodes = first + 65
  bad.preds[bad.n_preds].first, bad.preds[bad.n_preds].n = first, 65
  bad.n_preds += 1
  _refused(env, bad, 'stack deeper than 32')
  # ... and 32 deep is taken
  ok = _abi.SwbTreeSampler.from_buffer_copy(bad)
  for k in range(63):
    ok.pred_nodes[first + k].op = _abi.PRED_LEAF if k < 32 else _abi.PRED_AND
  ok.n_pred_nodes = first + 63
  ok.preds[ok.n_preds - 1].n = 63
  base, length = np.zeros(4, np.int32), np.full(4, 12, np.int32)
  _emu_engine.check(_emu_engine.lib().swb_sample_pool_tree(env.engine._h, C.byref(ok), 12, base.ctypes.data, length.ctypes.data,
                                                          C.c_uint64(1), C.c_uint64(0), None))
  # other indices and kinds
  for field, value, message in (('n_tasks', 2, 'labels 2 tasks'), ('max_tries', 0, 'max_tries'), ('n_leaves', 65, 'at most 64 leaves')):
    bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
    setattr(bad, field, value)
    _refused(env, bad, message)
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.ops[0].a = bad.n_leaves
  _refused(env, bad, 'bad leaf index')
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  x_leaf = [i for i in range(bad.n_leaves) if bad.leaves[i].factor == 0][0]
  bad.leaves[x_leaf].kind = _abi.FACTOR_UNIFORM_INT
  _refused(env, bad, 'x and y must be float32 Continuous factors')
  hue = [i for i in range(spec.n_ops) if spec.ops[i].kind == _abi.OP_DRAW and spec.leaves[spec.ops[i].a].factor == _abi.FACTOR_ORDER.index('c0')][0]
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.leaves[bad.ops[hue].a].kind = _abi.FACTOR_UNIFORM_INT
  _refused(env, bad, 'hsv colours must be float factors')
  bad = _abi.SwbTreeSampler.from_buffer_copy(spec)
  bad.leaves[bad.ops[hue].a].factor = _abi.FACTOR_ORDER.index('angle')          # a float32 angle
  _refused(env, bad, 'angle must be Discrete or integer degrees within [0, 360]')
  env.close()
