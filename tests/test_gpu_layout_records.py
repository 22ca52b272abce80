"""layout_record_cases.py on a real MI355X, through sage_gs.Renderer: splat records stored at layout positions and gathered through the
inverse permutation, held bit for bit against the same arrays uploaded in the caller's order (the cases test_emu_layout_records.py runs
under the emulator)."""
import pytest

pytestmark = pytest.mark.gpu

import layout_record_cases as lc
from test_gpu_upload import UploadDriver


@pytest.fixture(scope="module")
def drv():
    d = UploadDriver()
    yield d
    d.close()


def test_ties_against_the_layout(drv):
    lc.case_ties_against_the_layout(drv)


def test_export_by_index(drv):
    lc.case_export_by_index(drv)


def test_every_gather_site(drv):
    lc.case_every_gather_site(drv)


def test_deep_tile_gather(drv):
    lc.case_deep_tile_gather(drv)


def test_group_path(drv):
    lc.case_group_path(drv)
