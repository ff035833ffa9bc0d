"""Every family of Pillow tables swb_upload_resample accepts, on the GPU: the cases of tests/_resample_tables_cases.py -- frames
+-0 against numpy's two integer passes over the oracle's canvases, everything else through tests/_parity.py.  The engine's own
tables keep six output rows in flight at every image size and anti_aliasing: these are the only launches of
swb_resample_kernel<8> (seven and eight rows in flight) in the suite, and of swb_resample_kernel<6> on anything but them."""
import pytest

from tests import _resample_tables_cases as cases

pytestmark = pytest.mark.gpu

N_ENVS = 24


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
@pytest.mark.parametrize('fam', cases.FAMILIES, ids=cases.family_id)
def test_families(fam, geometry):
  rows, vs = cases.families(_gpu, geometry, fam, fam, N_ENVS)
  assert vs == (8 if rows in (7, 8) else 6)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
def test_seven_rows_in_flight_run_the_eight_slot_build(geometry):
  assert cases.families(_gpu, geometry, ('lanczos', 0.9), ('lanczos', 0.9), 11, steps=4) == (7, 8)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
def test_eight_rows_in_flight_run_the_eight_slot_build(geometry):
  assert cases.families(_gpu, geometry, ('lanczos', 0.82), ('lanczos', 0.82), 11, steps=4) == (8, 8)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
@pytest.mark.parametrize('fam_h,fam_v', cases.MIXED, ids=('h_lanczos_box0.82_v_bicubic', 'h_bicubic_v_lanczos_box0.82'))
def test_mixed_axes(fam_h, fam_v, geometry):
  assert cases.families(_gpu, geometry, fam_h, fam_v, N_ENVS)[1] == (8 if fam_v[0] == 'lanczos' else 6)


@pytest.mark.parametrize('geometry', ('64x64_aa5', '128x32_aa2'))
@pytest.mark.parametrize('band_tasks', (0, 1))
@pytest.mark.parametrize('n_bands', (1, 4, 8))
def test_bands_with_eight_rows_in_flight(monkeypatch, n_bands, band_tasks, geometry):
  cases.bands(_gpu, monkeypatch, geometry, n_bands, band_tasks, N_ENVS)


@pytest.mark.parametrize('which', ('never_hit', 'scripted'))
def test_kept_lists_and_frame_cache(monkeypatch, which):
  cases.kept_lists_and_frame_cache(_gpu, monkeypatch, 23, which)


@pytest.mark.parametrize('which', sorted(cases.LARGE))
@pytest.mark.parametrize('fam', cases.FAMILIES + (cases.rt.TOO_MANY,), ids=cases.family_id)
def test_large_paths(monkeypatch, fam, which):
  cases.large_paths(_gpu, monkeypatch, which, fam, 12)


def test_refusals():
  cases.refusals(_gpu, 8)
