"""The host side of the diffraction PSF (CPU): argument checks that come before any GPU call, the PSF object's own
host-side sums, and the ABI entries."""
import os
import re

import numpy as np
import pytest

from pyrayt_amd.frame import PSF, DeviceFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_frame(wavelengths=(0.633,)):
    n = len(wavelengths)
    rows = np.zeros((15, 2 * n))
    rows[0] = [0] * n + [1] * n
    rows[2] = list(wavelengths) * 2
    rows[4] = list(range(n)) * 2
    rows[5] = [1] * n + [2] * n
    return DeviceFrame(rows, [n, n])


def test_psf_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    with pytest.raises(TypeError, match="world_unit_um"):
        frame.psf(2)
    for bad in (0, -1000, float("nan"), "mm"):
        with pytest.raises(ValueError, match="world_unit_um"):
            frame.psf(2, world_unit_um=bad)
    for bad in (0, 1025, (64,), (64, 0), 12.5, (64, 2000), True):
        with pytest.raises(ValueError, match="pixels"):
            frame.psf(2, world_unit_um=1000, pixels=bad)
    for bad in (0, -1e-3, float("inf"), (1e-3, 0), (1e-3, 1e-3, 1e-3)):
        with pytest.raises(ValueError, match="pixel_size"):
            frame.psf(2, world_unit_um=1000, pixel_size=bad)
    with pytest.raises(ValueError, match="centre"):
        frame.psf(2, world_unit_um=1000, centre=(0.0, float("nan")))
    with pytest.raises(ValueError, match="weights"):
        frame.psf(2, world_unit_um=1000, weights="brightness")
    with pytest.raises(NotImplementedError):
        frame.psf(2, world_unit_um=1000, group=object())
    with pytest.raises(ValueError, match="where"):
        frame.where(generation=1).psf(2, world_unit_um=1000)
    recorded = host_frame()
    recorded.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        recorded.psf(2, world_unit_um=1000)


def test_psf_refuses_more_than_sixteen_wavelengths():
    many = host_frame(tuple(0.4 + 0.01 * k for k in range(17)))
    with pytest.raises(ValueError, match="16 distinct wavelengths"):
        many.psf(2, world_unit_um=1000)
    with pytest.raises(ValueError, match="16 distinct wavelengths"):
        many.psf(None, world_unit_um=1000)
    bad = host_frame((0.5, float("nan")))
    with pytest.raises(ValueError, match="wavelength"):
        bad.psf(2, world_unit_um=1000)
    with pytest.raises(ValueError, match="no row"):
        host_frame().psf(7, world_unit_um=1000)


def test_psf_object_sums_on_the_host():
    nx, ny = 5, 3
    image = np.zeros((1, 2, nx, ny))
    image[0, 0, 2, 1] = 0.75
    image[0, 1, 2, 1] = 0.25
    image[0, 0, 4, 1] = 0.5
    record = np.array([[[10, 1, 10.0, 1.0], [5, 0, 5.0, 0.5]]])
    psf = PSF(image, np.array([0.8]), record, [0.5, 0.6], 1000.0, (nx, ny), (0.1, 0.2), (1.0, 0.0), np.array([10.0]),
              None)
    np.testing.assert_allclose(psf.u, [0.8, 0.9, 1.0, 1.1, 1.2])
    np.testing.assert_allclose(psf.v, [-0.2, 0.0, 0.2])
    assert psf.image.shape == (1, nx, ny) and psf.image[0, 2, 1] == 1.0
    assert psf.peak[0] == 1.0 and tuple(psf.peak_uv[0]) == (1.0, 0.0)
    assert psf.n_rays[0] == 15 and psf.n_missed[0] == 1
    # (P is (u, v) = (0, 0); the window is centred on (1, 0))
    np.testing.assert_allclose(psf.encircled_energy([0.05, 1.05], about="reference"), [[0.0, 2 / 3]])
    np.testing.assert_allclose(psf.encircled_energy(0.05, about="peak"), [2 / 3])
    with pytest.raises(ValueError, match="about"):
        psf.encircled_energy(0.1, about="centroid")
    table = psf.to_pandas()
    assert list(table.columns) == ["strehl", "peak", "peak_u", "peak_v", "f_number", "n_rays", "n_missed"]


def test_abi_entries_are_declared():
    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prt.h")).read(), flags=re.S)
    for name in ("prt_frame_psf_workspace_bytes", "prt_frame_psf"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert engine.PRT_VERSION == 240


def test_library_checks_psf_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_psf_workspace_bytes(1000, 2, 3) > 1000 * 64
    assert lib.prt_frame_psf_workspace_bytes(1000, 2, 17) == -1
    buf = np.zeros(64)
    lam = np.array([0.5, 0.6] + [0.7 + 0.01 * k for k in range(17)])
    centre = np.zeros(2)
    p = buf.ctypes.data

    def call(n_w=2, nx=8, ny=8, du=1e-3, unit=1000.0, n_groups=1, wavelengths=lam):
        return lib.prt_frame_psf(0, p, 4, 4, 1.0, float("nan"), float(n_groups > 1), n_groups, p, p, p, -1, wavelengths.ctypes.data,
                                 n_w, unit, nx, ny, du, du, centre.ctypes.data, p, p, p, p, None)

    for kwargs, message in ((dict(n_w=17), "16 distinct"), (dict(nx=0), "1..1024"), (dict(ny=1025), "1..1024"),
                            (dict(du=0.0), "du, dv"), (dict(unit=0.0), "world_unit_um"),
                            (dict(wavelengths=np.array([0.5, 0.5])), "distinct"),
                            (dict(nx=1024, ny=1024, n_groups=4, n_w=16), "slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
