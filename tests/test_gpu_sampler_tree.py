"""The general device sampler (swb_sample_pool_tree) on the GPU: every array of the pool bit for bit against the Python model
of tests/_sampler_tree_model.py, and environments on tree-sampled pools against the oracle.  The bodies are in
tests/_sampler_tree_cases.py; tests/test_emulated_sampler_tree.py runs them on the host emulation of the kernel."""
import pytest

from tests import _sampler_tree_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', sorted(cases.CASES))
def test_tree_sampler_equals_the_python_model(case):
  if case == 'exhaust':
    cases.pool_matches_the_model_case(case, num_envs=4, episodes_per_env=2)      # P = 8
  else:
    cases.pool_matches_the_model_case(case)


def test_tree_sampler_second_block_and_high_entry_word():
  cases.odd_sizes_case()


def test_tree_sampler_shards_reproduce_the_whole_job():
  cases.shards_case()


def test_tree_sampler_refresh_keeps_the_live_entries():
  cases.refresh_case()


@pytest.mark.parametrize('case,click', [('hue_filter', 'uniform'), ('pos_goal', 'sprite'), ('meta_swap', 'sprite')])
def test_environment_on_a_tree_sampled_pool_steps_like_the_oracle(case, click):
  cases.parity_case(case, click, seed=3)      # (the seed the emulated suite checks: a sprite changes cell inside an episode)


def test_setter_on_a_tree_sampled_keyed_handle_keeps_the_cell_labels():
  cases.setter_keeps_cell_labels_case()
