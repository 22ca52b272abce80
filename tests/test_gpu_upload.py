"""The scene upload on a real MI355X: the Z-order permutation (SGS_BUF_SCENE_PERM) and the per-chunk bounds (SGS_BUF_CHUNK_BOUNDS) of
upload_cases' scenes, through sage_gs.Renderer, against tests/upload_ref.py — the cases test_emu_upload.py runs under the emulator, up to
131 073 Gaussians (k_mean_bounds' grid-stride loop).  The real-coordinate cases (random_cloud, signed_zeros, non_finite_means,
finite_outlier, compressed, effect) rest on a correctly rounded fp32 division in k_morton_keys; the lattice cases do not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import upload_cases as uc
from test_gpu_parity import GpuDriver


class UploadDriver(GpuDriver):
    def upload_compressed(self, chunks, packed, sh, deg, sh_decode=None):
        if self.scene is not None:
            self.scene.free()
        self.scene = self.r.upload_compressed(chunks, packed, sh, deg, sh_decode=sh_decode)

    def debug(self, what, dtype):
        return self.r.debug_buffer(what, dtype)

    def scene_geom(self):
        from sage_gs import _capi
        return self.r.debug_buffer(_capi.BUF_SCENE_GEOM, np.float32).reshape(-1, 11)


@pytest.fixture(scope="module")
def drv():
    d = UploadDriver()
    yield d
    d.close()


@pytest.mark.parametrize("name", list(uc.CASES))
def test_upload(drv, name):
    uc.CASES[name](drv)
