"""The host side of the ray-aberration curves (CPU): argument checks that come before any GPU call, the RayAberrations
object's table, fans, zonal curve, RMS radius and closed-form best focus on hand-made sums, the ABI entries and the
kernels' resources."""
import os
import re

import numpy as np
import pytest

from pyrayt_amd.frame import DeviceFrame, RayAberrations, zernike_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_frame():
    rows = np.zeros((15, 4))
    rows[0] = [0, 0, 1, 1]
    rows[4] = [0, 1, 0, 1]
    rows[5] = [1, 1, 2, 2]
    rows[12] = 1.0
    return DeviceFrame(rows, [2, 2])


def test_ray_aberration_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    with pytest.raises(ValueError, match="pupil"):
        frame.ray_aberrations(2, pupil="angle")
    for bad in ("chief ray", "centre"):
        with pytest.raises(ValueError, match="reference"):
            frame.ray_aberrations(2, reference=bad)
    for bad in (0, 37, 2.5, True, "21"):
        with pytest.raises(ValueError, match="zernike"):
            frame.ray_aberrations(2, zernike=bad)
    for bad in (-1, 1025, 0.5, "many"):
        with pytest.raises(ValueError, match="zones"):
            frame.ray_aberrations(2, zones=bad)
    with pytest.raises(ValueError, match="axis"):
        frame.ray_aberrations(2, axis=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="weights"):
        frame.ray_aberrations(2, weights="brightness")
    with pytest.raises(ValueError, match="pupil_radius"):
        frame.ray_aberrations(2, pupil_radius=-1.0)
    with pytest.raises(ValueError, match="launch_origin"):
        frame.ray_aberrations(2, launch_origin=(0.0, float("nan"), 0.0))
    with pytest.raises(NotImplementedError):
        frame.ray_aberrations(2, group=object())
    narrow = DeviceFrame(np.zeros((15, 2)), [2], columns=(0, 4, 5, 9, 10, 11))
    with pytest.raises(ValueError, match="without the column"):
        narrow.ray_aberrations(None)
    with pytest.raises(KeyError, match="without the column"):
        narrow.launch_index()
    # the join needs the whole frame
    with pytest.raises(ValueError, match="where"):
        frame.where(surface=2).ray_aberrations(2)
    with pytest.raises(ValueError, match="select"):
        frame.select(np.array([True, False, True, False])).launch_index()
    with pytest.raises(ValueError, match="generation"):
        frame.generation(1).launch()
    recorded = host_frame()
    recorded.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        recorded.ray_aberrations(2)


def hand_made(n=400, terms=6, n_zones=4, shift=0.3, seed=5):
    """One group whose eps = -shift * s exactly (a perfect focus at delta = shift), with the device's sums restated."""
    rng = np.random.default_rng(seed)
    r, t = np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
    p = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    s = 0.05 * p                      # (slopes linear in the pupil: a defocused, otherwise perfect beam)
    eps = -shift * s
    w = 1.0 + rng.random(n)
    la = 10.0 + 0.5 * r * r
    la[::7] = np.nan
    rho = 2.0
    z = zernike_basis(terms, r, t).T  # (n, terms)
    upper = np.triu_indices(terms)
    targets = np.stack([eps[:, 0], eps[:, 1], s[:, 0], s[:, 1]], 1)
    normal = np.concatenate([((z * w[:, None]).T @ z)[upper], ((z * w[:, None]).T @ targets).T.reshape(-1), [w.sum()]])
    record = np.zeros(16)
    record[0:3], record[3], record[4], record[5], record[6], record[7] = (1.0, 2.0, 3.0), rho, n, 2, np.isfinite(la).sum(), 17
    record[8] = w.sum()
    record[9:11], record[11:13] = (w[:, None] * eps).sum(0), (w[:, None] * s).sum(0)
    record[13], record[14], record[15] = (w * (eps ** 2).sum(1)).sum(), (w * (eps * s).sum(1)).sum(), (w * (s ** 2).sum(1)).sum()
    zone = np.minimum(np.floor(r * n_zones), n_zones - 1).astype(int)
    zones = np.zeros((n_zones, 6))
    ok = np.isfinite(la)
    for k in range(n_zones):
        m, mf = zone == k, (zone == k) & ok
        zones[k] = [m.sum(), w[mf].sum(), (w * la)[mf].sum(), (w * la * la)[mf].sum(), (w * (eps ** 2).sum(1))[m].sum(), mf.sum()]
    rays = np.concatenate([p, eps, s, la[:, None]], 1)
    obj = RayAberrations(rays, np.arange(n) + 100, record[None], normal[None], zones[None], terms)
    return obj, dict(p=p, s=s, eps=eps, w=w, la=la, rho=rho, zone=zone, shift=shift)


def test_best_focus_and_rms_radius_in_closed_form():
    obj, d = hand_made()
    assert abs(obj.best_focus()[0] - d["shift"]) <= 1e-12
    assert obj.rms_radius(d["shift"])[0] <= 1e-9 * obj.rms_radius(0.0)[0]
    # against the definition at another plane: the weighted RMS of eps + delta s about its own centroid
    delta = -0.11
    x = d["eps"] + delta * d["s"]
    mean = (d["w"][:, None] * x).sum(0) / d["w"].sum()
    want = np.sqrt((d["w"] * ((x - mean) ** 2).sum(1)).sum() / d["w"].sum())
    assert abs(obj.rms_radius(delta)[0] - want) <= 1e-12 * want
    assert list(obj.n_rays) == [400] and list(obj.n_missed) == [2] and list(obj.chief_row) == [17]
    assert obj.centre.tolist() == [[1.0, 2.0, 3.0]] and obj.pupil_radius[0] == 2.0
    # a group without rays: NaN, not an error
    empty = RayAberrations(np.zeros((0, 7)), np.zeros(0, dtype=np.int64), np.zeros((1, 16)), np.zeros((1, 6 * 7 // 2 + 25)),
                           np.zeros((1, 4, 6)), 6)
    assert np.isnan(empty.best_focus()[0]) and np.isnan(empty.rms_radius()[0]) and empty.rank[0] == 0


def test_fans_reproduce_the_fitted_polynomial():
    obj, d = hand_made()
    assert obj.rank[0] == 6 and obj.coefficients.shape == (1, 4, 6)
    assert np.all(obj.residual[0] <= 1e-7)   # (the square root of a difference of two sums that agree to rounding)
    for azimuth in (0.0, 90.0, 30.0):
        t, along, across = obj.fan(azimuth, samples=33)
        assert t[0] == -1.0 and t[-1] == 1.0 and along.shape == (1, 33)
        # eps = -shift * 0.05 p: along the diameter -0.015 t, nothing across it
        np.testing.assert_allclose(along[0], -d["shift"] * 0.05 * t, atol=1e-12)
        np.testing.assert_allclose(across[0], 0.0, atol=1e-12)
        _, at_focus, _ = obj.fan(azimuth, samples=33, focus=d["shift"])
        np.testing.assert_allclose(at_focus[0], 0.0, atol=1e-12)


def test_longitudinal_curve_and_table():
    obj, d = hand_made()
    curve = obj.longitudinal_curve()
    np.testing.assert_allclose(curve["radius"][0], (np.arange(4) + 0.5) / 4 * d["rho"])
    ok = np.isfinite(d["la"])
    for k in range(4):
        m = (d["zone"] == k) & ok
        mean = np.average(d["la"][m], weights=d["w"][m])
        assert abs(curve["mean"][0, k] - mean) <= 1e-12 * abs(mean)
        std = np.sqrt(np.average((d["la"][m] - mean) ** 2, weights=d["w"][m]))
        assert abs(curve["std"][0, k] - std) <= 1e-6 * std + 1e-12
        assert curve["count"][0, k] == m.sum() and curve["rays"][0, k] == (d["zone"] == k).sum()
    table = obj.to_pandas()
    assert list(table.columns) == ["row", "source_id", "radius", "h2", "p1", "p2", "eps1", "eps2", "s1", "s2", "focus"]
    assert len(table) == 400 and table["row"].iloc[0] == 100
    np.testing.assert_allclose(table["radius"], d["p"][:, 0] * d["rho"])
    np.testing.assert_array_equal(table["focus"], d["la"])


def test_abi_entries_are_declared():
    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prt.h")).read(), flags=re.S)
    for name in ("prt_frame_launch_index", "prt_frame_ray_aberrations_workspace_bytes", "prt_frame_ray_aberrations"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name


def test_library_checks_ray_aberration_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_ray_aberrations_workspace_bytes(1000, 2, 21, 64) > 1000 * 90
    for args in ((1000, 2, 0, 64), (1000, 2, 37, 64), (1000, 2, 21, 1025), (1000, 2, 21, -1), (1000, 0, 21, 64),
                 (-1, 2, 21, 64), (1000, 1 << 20, 21, 1024)):
        assert lib.prt_frame_ray_aberrations_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    origin = np.zeros(3)

    def call(n_groups=1, reference=None, mode=0, axes=axes, pupil=0, origin=origin, radius=0.0, terms=21, zones=4,
             weight=1):
        return lib.prt_frame_ray_aberrations(0, p, 4, 4, p, 1.0, float("nan"), float(n_groups > 1), n_groups, reference,
                                             mode, axes.ctypes.data, pupil, origin.ctypes.data, radius, terms, zones,
                                             weight, 4, p, p, p, p, p, p, None)

    for kwargs, message in ((dict(terms=0), "1 to 36 terms"), (dict(terms=37), "1 to 36 terms"),
                            (dict(zones=1025), "zones: 0 to 1024"), (dict(zones=-1), "zones: 0 to 1024"),
                            (dict(weight=15), "weight_column"), (dict(pupil=2), "pupil_mode"),
                            (dict(mode=3), "reference_mode"), (dict(mode=1), "reference_mode"),
                            (dict(reference=p, mode=0), "reference_mode"),
                            (dict(radius=float("nan")), "pupil_radius"), (dict(radius=-1.0), "pupil_radius"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(origin=np.full(3, np.inf)), "launch_origin"),
                            (dict(n_groups=1 << 20, zones=1024), "count cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
    # the join
    for args, message in (((0, p, 4, 4, 5, 0.0, 8, p, None), "bad buffers"),
                          ((0, p, 4, 4, 2, 0.0, 0, p, None), "n_ids"),
                          ((0, p, 4, 4, 2, float("nan"), 8, p, None), "id0 finite")):
        assert lib.prt_frame_launch_index(*args) == -1, args
        assert message in lib.prt_last_error().decode(), (args, lib.prt_last_error())


def test_aberration_kernels_use_no_scratch():
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
    # (the pass's scans are k_sort_positions / k_sort_offsets of prt_sort.hpp, its centre sums k_mtf_centre<AbRaw>)
    kernels = {name: res for name, res in found.items() if "k_aberration_" in name}
    assert len(kernels) == 9, sorted(kernels)
    shared = {name: res for name, res in found.items() if "k_sort_" in name or ("k_mtf_centre" in name and "AbRaw" in name)}
    assert len(shared) == 4, sorted(shared)
    kernels.update(shared)
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
