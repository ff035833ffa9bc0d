"""Every family of Pillow tables swb_upload_resample accepts, on the emulated kernels (tests/emu, CPU): the cases of
tests/_resample_tables_cases.py -- frames +-0 against numpy's two integer passes over the oracle's canvases, everything else
through tests/_parity.py.  A handful of environments each; tests/test_gpu_resample_tables.py is the twin on the hardware."""
import pytest

from tests import _resample_tables_cases as cases

N_ENVS = 6


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
@pytest.mark.parametrize('fam', cases.FAMILIES, ids=cases.family_id)
def test_families(fam, geometry):
  rows, vs = cases.families(_emu, geometry, fam, fam, N_ENVS)
  assert vs == (8 if rows in (7, 8) else 6)


@pytest.mark.parametrize('geometry', sorted(cases.GEOMETRIES))
@pytest.mark.parametrize('fam_h,fam_v', cases.MIXED, ids=('h_lanczos_box0.82_v_bicubic', 'h_bicubic_v_lanczos_box0.82'))
def test_mixed_axes(fam_h, fam_v, geometry):
  assert cases.families(_emu, geometry, fam_h, fam_v, N_ENVS)[1] == (8 if fam_v[0] == 'lanczos' else 6)


@pytest.mark.parametrize('geometry', ('64x64_aa5', '128x32_aa2'))
@pytest.mark.parametrize('band_tasks', (0, 1))
@pytest.mark.parametrize('n_bands', (1, 4, 8))
def test_bands_with_eight_rows_in_flight(monkeypatch, n_bands, band_tasks, geometry):
  cases.bands(_emu, monkeypatch, geometry, n_bands, band_tasks, 16 if band_tasks else N_ENVS)


@pytest.mark.parametrize('which', ('never_hit', 'scripted'))
def test_kept_lists_and_frame_cache(monkeypatch, which):
  cases.kept_lists_and_frame_cache(_emu, monkeypatch, 7, which)


@pytest.mark.parametrize('which', sorted(cases.LARGE))
@pytest.mark.parametrize('fam', cases.FAMILIES + (cases.rt.TOO_MANY,), ids=cases.family_id)
def test_large_paths(monkeypatch, fam, which):
  cases.large_paths(_emu, monkeypatch, which, fam, N_ENVS)


def test_refusals():
  cases.refusals(_emu, N_ENVS)
