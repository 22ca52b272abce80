"""The scene upload — Z-order sort, Morton keys, chunk bounds — under the wave64 emulator: upload_cases' checks on the product's own
kernel source (csrc/sgs_kernels.h k_mean_bounds ... k_chunk_bounds, driven by layout_scene in csrc/sgs_api.hip).  The same cases run on
the GPU in test_gpu_upload.py, and on seeded faults in test_emu_upload_mutants.py."""
import pytest

import emu_harness
import upload_cases as uc


@pytest.fixture(scope="module")
def drv():
    d = emu_harness.EmuRenderer(record_capacity=1 << 22)
    yield d
    d.close()


@pytest.mark.parametrize("name", list(uc.CASES))
def test_upload(drv, name):
    uc.CASES[name](drv)
