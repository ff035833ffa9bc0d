"""GPU: snapshots (swb_state_save_kernel, swb_state_load_kernel, swb_copy_pool) against the CPU oracle -- the cases of
tests/_snapshot_cases.py, which tests/test_emulated_snapshot.py runs on the emulated library.  A loaded environment continues
bit for bit as its source would have, frames +-0; only the loaded environments' run lists are built again."""
import pytest

from tests import _snapshot_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('name,aa,expect', cases.ROUND_TRIP, ids=['%s-aa%d' % (n, a) for n, a, _ in cases.ROUND_TRIP])
def test_gpu_snapshot_round_trip(name, aa, expect):
  cases.round_trip_case(_gpu, name, aa, expect)


def test_gpu_snapshot_permuted_and_partial_load():
  cases.permuted_case(_gpu)


def test_gpu_snapshot_load_drops_only_the_loaded_lists(monkeypatch):
  cases.stale_list_case(_gpu, monkeypatch)


def test_gpu_snapshot_rollout_end_states():
  cases.rollout_end_case(_gpu)


def test_gpu_snapshot_fork():
  cases.fork_case()


def test_gpu_snapshot_copy_pool_between_unlike_handles():
  cases.unlike_handles_case(_gpu)


def test_gpu_snapshot_pool_identity_and_host_round_trip():
  cases.pool_identity_case(_gpu)


def test_gpu_snapshot_is_refused_after_a_pool_refresh():
  cases.refresh_refuses_case()


def test_gpu_snapshot_guards():
  cases.guards_case(_gpu)
