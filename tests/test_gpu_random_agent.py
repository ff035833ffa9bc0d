"""GPU: swb_sample_actions (swb_sample_actions_kernel) against the Python model of tests/_random_agent_model.py and the CPU
oracle -- the cases of tests/_random_agent_cases.py, which tests/test_emulated_random_agent.py runs on the emulated library.
Actions, contained positions, sprites and tries bit-exact; the handle untouched."""
import pytest

from tests import _random_agent_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('name', cases.MODEL)
def test_gpu_sampled_actions_equal_the_model(name):
  cases.model_case(_gpu, name)


def test_gpu_sixty_four_vertex_shape_circle_and_star_are_drawn_on():
  cases.shapes_64_coverage_case(_gpu)


def test_gpu_sampled_positions_follow_setter_overrides():
  cases.setters_case(_gpu)


def test_gpu_sampling_leaves_the_handle_untouched():
  cases.read_only_case(_gpu)


def test_gpu_sampled_clicks_are_contained_and_move_a_sprite():
  cases.containment_case(_gpu)


def test_gpu_sample_actions_refusals():
  cases.refusals_case(_gpu)


def test_gpu_sample_actions_python_surface():
  cases.surface_case()


def test_gpu_shards_draw_their_part_of_the_batch_streams():
  cases.offsets_case()


def test_gpu_environment_groups_draw_different_streams():
  cases.groups_case()
