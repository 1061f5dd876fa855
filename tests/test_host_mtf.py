"""The host side of the geometric MTF (CPU): argument checks that come before any GPU call, the MTF object's table and
best focus, the closed-form diffraction MTF, the MTF of a PSF image, the ABI entries and the kernels' resources."""
import os
import re

import numpy as np
import pytest

from pyrayt_amd.frame import MTF, PSF, DeviceFrame, diffraction_mtf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_frame():
    rows = np.zeros((15, 4))
    rows[0] = [0, 0, 1, 1]
    rows[4] = [0, 1, 0, 1]
    rows[5] = [1, 1, 2, 2]
    rows[12] = 1.0
    return DeviceFrame(rows, [2, 2])


def test_mtf_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    for bad in ([-1.0], [float("nan")], [float("inf")], np.zeros(4097), [], [[1.0, 2.0]], "fine"):
        with pytest.raises(ValueError, match="frequencies"):
            frame.mtf(2, bad)
    for bad in (np.zeros(17), [float("nan")], [], "tangential"):
        with pytest.raises(ValueError, match="azimuths"):
            frame.mtf(2, [10.0], azimuths=bad)
    for bad in (np.zeros(257), [float("inf")], []):
        with pytest.raises(ValueError, match="focus"):
            frame.mtf(2, [10.0], focus=bad)
    with pytest.raises(ValueError, match="weights"):
        frame.mtf(2, [10.0], weights="brightness")
    with pytest.raises(ValueError, match="reference"):
        frame.mtf(2, [10.0], reference="chief ray")
    with pytest.raises(ValueError, match="axis"):
        frame.mtf(2, [10.0], axis=(0.0, 0.0, 0.0))
    with pytest.raises(NotImplementedError):
        frame.mtf(2, [10.0], group=object())
    narrow = DeviceFrame(np.zeros((15, 2)), [2], columns=(10, 11))
    with pytest.raises(ValueError, match="without the column"):
        narrow.mtf(None, [10.0])


def test_mtf_object_table_and_best_focus():
    focus = np.linspace(-1.0, 1.0, 21)
    peak = 0.1234
    merit = 0.9 - 0.5 * (focus - peak) ** 2  # (a parabola: recovered exactly from three samples)
    otf = np.empty((2, len(focus), 2, 3), dtype=complex)
    otf[0] = merit[:, None, None] * np.exp(0.3j)
    otf[1] = np.nan
    otf[0, :, :, 0] = 1.0
    record = np.array([[0.0, 1.0, 2.0, 5.0, 10, 1], [np.nan] * 3 + [0.0, 0, 0]])
    mtf = MTF(otf, record, [0.0, 10.0, 20.0], [0.0, 90.0], focus)
    assert mtf.mtf.shape == (2, 21, 2, 3) and np.allclose(mtf.ptf[0, :, :, 1:], 0.3)
    assert list(mtf.n_rays) == [10, 0] and list(mtf.n_missed) == [1, 0] and mtf.centre.shape == (2, 3)
    best = mtf.best_focus(frequency=10.0)
    assert abs(best[0] - peak) <= 1e-12 and np.isnan(best[1])
    assert abs(mtf.best_focus(frequency=20.0, azimuths=[90.0])[0] - peak) <= 1e-12
    assert abs(mtf.best_focus()[0] - peak) <= 1e-12  # (frequency 0 is flat: it moves the mean, not its peak)
    # a peak at an end of the scan is not refined
    edge = MTF(np.linspace(0.1, 0.9, 5)[None, :, None, None] + 0j, record[:1], [10.0], [0.0], np.arange(5.0))
    assert edge.best_focus()[0] == 4.0
    with pytest.raises(ValueError, match="frequency"):
        mtf.best_focus(frequency=15.0)
    table = mtf.to_pandas()
    assert list(table.columns) == ["source_id", "focus", "azimuth", "frequency", "mtf", "ptf"]
    assert table.shape == (2 * 21 * 2 * 3, 6)
    row = table.iloc[21 * 2 * 3 - 1]
    assert (row["source_id"], row["focus"], row["azimuth"], row["frequency"]) == (0, 1.0, 90.0, 20.0)


def test_diffraction_mtf_matches_a_pupil_autocorrelation():
    lam_um, f_number, unit = 0.55, 8.0, 1000.0
    cutoff = 1.0 / (lam_um / unit * f_number)
    # the incoherent OTF is the pupil's autocorrelation: a disk of radius 1 shifted by 2 nu / cutoff of its radius
    n = 801
    x = np.linspace(-1.0, 1.0, n)
    xx, yy = np.meshgrid(x, x, indexing="ij")
    pupil = (xx ** 2 + yy ** 2 <= 1.0).astype(float)
    area = pupil.sum()
    nu = np.array([0.0, 0.1, 0.25, 0.5, 0.75, 0.9]) * cutoff
    numeric = []
    for v in nu:
        shift = int(round(2 * v / cutoff / (x[1] - x[0])))
        numeric.append((pupil[shift:] * pupil[:n - shift]).sum() / area)
    closed = diffraction_mtf(nu, lam_um, f_number, unit)
    assert np.abs(closed - np.array(numeric)).max() <= 5e-3
    assert closed[0] == 1.0
    assert np.all(diffraction_mtf([cutoff, 1.5 * cutoff], lam_um, f_number, unit) == 0.0)
    with pytest.raises(ValueError, match="f_number"):
        diffraction_mtf([1.0], lam_um, 0.0, unit)


def test_psf_mtf_of_a_gaussian_image():
    sigma, step, side = 0.01, 0.001, 161
    u = (np.arange(side) - (side - 1) / 2) * step
    image = np.exp(-(u[:, None] ** 2 + u[None, :] ** 2) / (2 * sigma ** 2))[None, None]
    record = np.array([[[100, 2, 1.0, 1.0]]])
    psf = PSF(image, np.array([1.0]), record, [0.55], 1000.0, (side, side), (step, step), (0.0, 0.0), np.array([8.0]),
              None)
    nu = np.linspace(0.0, 40.0, 9)
    mtf = psf.mtf(nu, azimuths=(0.0, 30.0, 90.0))
    assert mtf.otf.shape == (1, 1, 3, 9) and mtf.n_rays[0] == 100 and mtf.n_missed[0] == 2
    want = np.exp(-2 * np.pi ** 2 * sigma ** 2 * nu ** 2)
    assert np.abs(mtf.mtf[0, 0] - want).max() <= 1e-6
    assert np.abs(mtf.ptf[0, 0]).max() <= 1e-9


def test_abi_entries_are_declared():
    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prt.h")).read(), flags=re.S)
    for name in ("prt_frame_mtf_workspace_bytes", "prt_frame_mtf"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert engine.PRT_VERSION == 240


def test_library_checks_mtf_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_mtf_workspace_bytes(1000, 2, 128, 2, 1) > 1000 * 100
    for args in ((1000, 2, 4097, 2, 1), (1000, 2, 128, 17, 1), (1000, 2, 128, 2, 257), (1000, 0, 128, 2, 1)):
        assert lib.prt_frame_mtf_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    nu, theta, focus = np.array([0.0, 10.0]), np.array([0.0, 90.0]), np.array([0.0])

    def call(frequencies=nu, n_f=2, azimuths=theta, n_a=2, planes=focus, n_p=1, weight=1, n_groups=1, axes=axes):
        return lib.prt_frame_mtf(0, p, 4, 4, 1.0, float("nan"), float(n_groups > 1), n_groups, None, axes.ctypes.data,
                                 weight, frequencies.ctypes.data, n_f, azimuths.ctypes.data, n_a, planes.ctypes.data,
                                 n_p, p, p, p, None)

    big = np.zeros(4097)
    for kwargs, message in ((dict(frequencies=np.array([-1.0, 1.0])), "frequencies finite and >= 0"),
                            (dict(frequencies=np.array([np.nan, 1.0])), "frequencies finite and >= 0"),
                            (dict(frequencies=big, n_f=4097), "1 to 4096 frequencies"),
                            (dict(n_a=17, azimuths=np.zeros(17)), "1 to 16 azimuths"),
                            (dict(azimuths=np.array([0.0, np.inf])), "azimuths finite"),
                            (dict(n_p=257, planes=np.zeros(257)), "1 to 256 focus shifts"),
                            (dict(planes=np.array([np.nan])), "focus shifts finite"),
                            (dict(weight=15), "weight_column"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(n_groups=2, frequencies=np.zeros(4096), n_f=4096, azimuths=np.zeros(16), n_a=16,
                                  planes=np.zeros(256), n_p=256), "slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_mtf_kernels_use_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    found = mod.kernel_resources(engine.LIB_PATH)
    # (the staging pass's scan over the waves is k_sort_offsets of prt_sort.hpp; k_mtf_centre stands once for MtfRaw and
    # once for the aberrations' AbRaw)
    kernels = {name: res for name, res in found.items() if "k_mtf_" in name}
    assert len(kernels) == 9 and sum("k_mtf_centre" in name for name in kernels) == 2, sorted(kernels)
    sort = {name: res for name, res in found.items() if "k_sort_" in name}
    assert len(sort) == 3 and all(any(f"k_sort_{k}" in name for name in sort) for k in ("positions", "offsets", "starts")), sorted(sort)
    kernels.update(sort)
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
