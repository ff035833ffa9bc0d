"""dm_env conformance of the N = 1 `Environment`, re-expressing dm_env.test_utils.EnvironmentTestMixin
as the reference uses it (reference: tests/environment_test.py:30-51): reset / step protocol on fresh
environments, and every time step of a longer action sequence conforms to reward_spec(),
discount_spec() and observation_spec() (a dict of specs, as the reference's assertValidObservation
override handles); sampled actions conform to action_spec().  The bodies are in tests/_surface_cases.py."""
import pytest

from tests import _surface_cases as cases
from tests._surface_cases import _reference_test_env, _rendered_env

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('make', [_reference_test_env, _rendered_env])
def test_reset_and_step_protocol_on_fresh_environments(make):
  cases.reset_and_step_protocol_case(make)


@pytest.mark.parametrize('make', [_reference_test_env, _rendered_env])
def test_longer_action_sequence_conforms_to_the_specs(make):
  cases.longer_action_sequence_case(make)


def test_specs_are_specs():
  cases.specs_are_specs_case()
