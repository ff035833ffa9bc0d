"""Split bands on the emulated kernel (tests/emu, CPU): the scripts of tests/_split_bands_cases.py against the oracle at every
step, with swb_list_stats, swb_frame_stats and swb_split_stats held to the model of the header word and the decision word."""
import pytest

from tests import _split_bands_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('which', ('always', 'never', 'half'))
@pytest.mark.parametrize('bands', (4, 8))
def test_thresholds(monkeypatch, bands, which):
  assert cases.thresholds(_emu, monkeypatch, 16, bands, which) == bands


def test_all_reset_while_the_word_says_split(monkeypatch):
  cases.all_reset(_emu, monkeypatch, 16, 4)


def test_two_column_groups(monkeypatch):
  cases.two_column_groups(_emu, monkeypatch, 8, 4)


def test_band_placement_cannot_honour_eight(monkeypatch):
  cases.cannot_honour(_emu, monkeypatch, 16)


@pytest.mark.parametrize('which', ('always', 'never'))
def test_eight_rows_in_flight(monkeypatch, which):
  cases.eight_rows_in_flight(_emu, monkeypatch, 16, 4, which)


@pytest.mark.parametrize('which', cases.BETWEEN)
def test_calls_between(monkeypatch, which):
  cases.call_between(_emu, monkeypatch, 16, which)


@pytest.mark.parametrize('which', ('anti_aliasing_1', 'no_frame_cache', 'bands_set', 'small_batch'))
def test_mode_absent(monkeypatch, which):
  cases.mode_absent(_emu, monkeypatch, 16, which)
