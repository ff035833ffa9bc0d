"""The speculative copies of the cover launch on the GPU: tests/_spec_copy_cases.py under both placements of the copy workgroups,
64 environments.  On the device a copy workgroup may read either value of its environment's word: frames and the parent's counts
are exact all the same, swb_spec_copy_stats lies between the two extremes."""
import pytest

from tests import _masked_step_cases as masked
from tests import _spec_copy_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_scripted_two_buffers(monkeypatch, order):
  cases.scripted(_gpu, monkeypatch, 64, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_thirteen_environments(monkeypatch, order):
  cases.scripted(_gpu, monkeypatch, 13, order, False, steps=10)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_stale_cache(monkeypatch, order):
  cases.stale_cache(_gpu, monkeypatch, 64, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', cases.GEOMETRIES)
def test_geometries(monkeypatch, which, order):
  cases.geometry(_gpu, monkeypatch, 64, which, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', ('never', 'always'))
def test_split_bands(monkeypatch, which, order):
  cases.split_bands(_gpu, monkeypatch, 64, which, order)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', cases.BETWEEN)
def test_calls_between(monkeypatch, which, order):
  cases.call_between(_gpu, monkeypatch, 64, which, order)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_state_view(monkeypatch, order):
  cases.state_view(_gpu, monkeypatch, 64, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_load_state_between(monkeypatch, order):
  cases.load_state_between(_gpu, monkeypatch, 64, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_masked_steps_at_every_word(monkeypatch, order):
  cases.masked_words(_gpu, monkeypatch, 64, order, False)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_reset_envs_and_masked_steps(monkeypatch, order):
  from spriteworld_amd import _lib
  cases.under(monkeypatch, order)
  masked.reset_envs(_gpu, monkeypatch, 66, _lib.SwbError)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', ('no_frame_cache', 'anti_aliasing_1'))
def test_absent(monkeypatch, which, order):
  cases.absent(_gpu, monkeypatch, 64, which, order)
