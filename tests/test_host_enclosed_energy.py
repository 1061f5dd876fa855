"""The host side of the enclosed energy (CPU): argument checks that come before any GPU call, the ABI entries, the
library's own refusals, the EnclosedEnergy object's table and best focus, the kernels' resources, and the numpy
restatement the GPU tests compare against (tests/energy_reference.py) on closed forms."""
import os
import re

import numpy as np
import pytest

import energy_reference as ref
from pyrayt_amd.frame import DeviceFrame, EnclosedEnergy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_frame():
    rows = np.zeros((15, 4))
    rows[0] = [0, 0, 1, 1]
    rows[4] = [0, 1, 0, 1]
    rows[5] = [1, 1, 2, 2]
    rows[12] = 1.0
    return DeviceFrame(rows, [2, 2])


def test_enclosed_energy_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    for bad in ([-1.0], [float("nan")], [float("inf")], np.arange(4097.0), [], [[1.0, 2.0]], "wide", [1.0, 1.0],
                [2.0, 1.0]):
        with pytest.raises(ValueError, match="radii"):
            frame.enclosed_energy(2, bad)
    for bad in ([0.0], [1.5], [-0.1], [float("nan")], np.full(17, 0.5), [], "half"):
        with pytest.raises(ValueError, match="fractions"):
            frame.enclosed_energy(2, [1.0], fractions=bad)
    with pytest.raises(ValueError, match="radii"):
        frame.enclosed_energy(2, None, fractions=None)
    for bad in ("round", 0, None):
        with pytest.raises(ValueError, match="shape"):
            frame.enclosed_energy(2, [1.0], shape=bad)
    for bad in (np.zeros(257), [float("inf")], []):
        with pytest.raises(ValueError, match="focus"):
            frame.enclosed_energy(2, [1.0], focus=bad)
    with pytest.raises(ValueError, match="weights"):
        frame.enclosed_energy(2, [1.0], weights="brightness")
    with pytest.raises(ValueError, match="reference"):
        frame.enclosed_energy(2, [1.0], reference="chief ray")
    with pytest.raises(ValueError, match="axis"):
        frame.enclosed_energy(2, [1.0], axis=(0.0, 0.0, 0.0))
    with pytest.raises(NotImplementedError):
        frame.enclosed_energy(2, [1.0], group=object())
    narrow = DeviceFrame(np.zeros((15, 2)), [2], columns=(10, 11))
    with pytest.raises(ValueError, match="without the column"):
        narrow.enclosed_energy(None, [1.0])


def test_abi_entries_are_declared_and_bound():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_energy_workspace_bytes", "prt_frame_energy"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    from pyrayt_amd.frame import _ENERGY_SHAPES

    for name, value in re.findall(r"#define PRT_ENERGY_([A-Z_0-9]+) (\d+)", header):
        assert _ENERGY_SHAPES[name.lower()] == int(value), name
    assert len(_ENERGY_SHAPES) == 4
    assert engine.PRT_VERSION == 240 and "#define PRT_VERSION 240" in header
    if os.path.exists(engine.LIB_PATH):
        lib = engine.library()
        assert lib.prt_frame_energy.argtypes is not None and len(lib.prt_frame_energy.argtypes) == 24
        assert len(lib.prt_frame_energy_workspace_bytes.argtypes) == 5


def test_library_checks_energy_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_energy_workspace_bytes(1000, 2, 64, 3, 41) > 1000 * 100
    assert lib.prt_frame_energy_workspace_bytes(1000, 2, 0, 3, 1) > 0
    assert lib.prt_frame_energy_workspace_bytes(1000, 2, 64, 0, 1) > 0
    for args in ((1000, 2, 4097, 3, 1), (1000, 2, 64, 17, 1), (1000, 2, 64, 3, 257), (1000, 2, 64, 3, 0),
                 (1000, 0, 64, 3, 1), (1000, 2, 0, 0, 1), (-1, 2, 64, 3, 1), (1000, 2, -1, 3, 1), (1000, 2, 64, -1, 1),
                 (1000, 64, 4096, 3, 256), (1000, 8, 64, 16, 256)):  # (the last two: the 256 MiB slab caps)
        assert lib.prt_frame_energy_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    edges, phi, focus = np.array([0.5, 1.0]), np.array([0.5, 0.9]), np.array([0.0])

    def call(radii=edges, n_r=2, fractions=phi, n_f=2, planes=focus, n_p=1, weight=1, n_groups=1, axes=axes, shape=0,
             energy=p, radius=p):
        return lib.prt_frame_energy(0, p, 4, 4, 1.0, float("nan"), float(n_groups > 1), n_groups, None,
                                    axes.ctypes.data, weight, shape, 1, radii.ctypes.data, n_r, fractions.ctypes.data,
                                    n_f, planes.ctypes.data, n_p, energy, radius, p, p, None)

    for kwargs, message in ((dict(radii=np.array([1.0, 1.0])), "strictly ascending"),
                            (dict(radii=np.array([2.0, 1.0])), "strictly ascending"),
                            (dict(radii=np.array([-1.0, 1.0])), "radii finite, >= 0"),
                            (dict(radii=np.array([1.0, np.inf])), "radii finite, >= 0"),
                            (dict(radii=np.array([np.nan, 1.0])), "radii finite, >= 0"),
                            (dict(radii=np.arange(4097.0), n_r=4097), "0 to 4096 radii"),
                            (dict(energy=None), "0 to 4096 radii"),
                            (dict(fractions=np.array([0.0, 0.5])), "fractions in (0, 1]"),
                            (dict(fractions=np.array([0.5, 1.5])), "fractions in (0, 1]"),
                            (dict(fractions=np.array([np.nan, 0.5])), "fractions in (0, 1]"),
                            (dict(fractions=np.full(17, 0.5), n_f=17), "0 to 16 fractions"),
                            (dict(radius=None), "0 to 16 fractions"),
                            (dict(n_r=0, n_f=0), "not neither"),
                            (dict(n_p=257, planes=np.zeros(257)), "1 to 256 focus shifts"),
                            (dict(n_p=0), "1 to 256 focus shifts"),
                            (dict(planes=np.array([np.nan])), "focus shifts finite"),
                            (dict(shape=4), "shape"),
                            (dict(shape=-1), "shape"),
                            (dict(weight=15), "weight_column"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(n_groups=0), "bad buffers"),
                            (dict(n_groups=64, radii=np.arange(4096.0), n_r=4096, planes=np.zeros(256), n_p=256),
                             "n_radii * 8 bytes above the 256 MiB slab cap"),
                            (dict(n_groups=8, fractions=np.full(16, 0.5), n_f=16, planes=np.zeros(256), n_p=256),
                             "16 KiB above the 256 MiB slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_enclosed_energy_object_table_and_best_focus():
    focus = np.linspace(-1.0, 1.0, 21)
    valley = 0.1234
    curve = 0.2 + 0.5 * (focus - valley) ** 2  # (a parabola: recovered exactly from three samples)
    radius = np.empty((2, len(focus), 3))
    radius[0] = curve[:, None] * np.array([1.0, 2.0, 3.0])
    radius[1] = np.nan
    energy = np.zeros((2, len(focus), 4))
    energy[0] = np.linspace(0.25, 1.0, 4)
    energy[1] = np.nan
    record = np.array([[0.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4, 5.0, 10, 1], [np.nan] * 7 + [0.0, 0, 0]])
    ee = EnclosedEnergy(energy, radius, record, [0.1, 0.2, 0.3, 0.4], [0.5, 0.8, 0.9], focus, "circle")
    assert list(ee.n_rays) == [10, 0] and list(ee.n_missed) == [1, 0] and ee.centre.shape == (2, 3)
    assert ee.sum_weights[0] == 5.0 and ee.centroid_shift.shape == (2, 2, 2)
    assert np.array_equal(ee.centroid_shift[0], [[0.1, 0.2], [0.3, 0.4]])
    best = ee.best_focus(0.8)
    assert abs(best[0] - valley) <= 1e-12 and np.isnan(best[1])
    assert abs(ee.best_focus()[0] - valley) <= 1e-12
    # a minimum at an end of the scan is not refined
    edge = EnclosedEnergy(np.zeros((1, 5, 0)), np.linspace(0.9, 0.1, 5)[None, :, None], record[:1], [], [0.8],
                          np.arange(5.0))
    assert edge.best_focus(0.8)[0] == 4.0
    with pytest.raises(ValueError, match="fraction"):
        ee.best_focus(0.7)
    table = ee.to_pandas()
    assert list(table.columns) == ["source_id", "focus", "quantity", "radius", "energy"]
    assert table.shape == (2 * 21 * (4 + 3), 5)
    row = table.iloc[21 * 4 - 1]
    assert (row["source_id"], row["focus"], row["quantity"], row["radius"], row["energy"]) == (0, 1.0, "energy", 0.4, 1.0)
    row = table.iloc[2 * 21 * 4 + 1]
    assert (row["source_id"], row["focus"], row["quantity"], row["energy"]) == (0, -1.0, "radius", 0.8)
    assert row["radius"] == radius[0, 0, 1]


def test_energy_kernels_use_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_energy_" in name}
    for wanted in ("centre", "record", "scale", "curve", "finish", "begin", "select", "digit"):
        assert any("k_energy_" + wanted in name for name in kernels), (wanted, sorted(kernels))
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
        assert res["group_segment_fixed_size"] <= 64 * 1024, (name, res)  # (two workgroups fit a CU's 160 KiB)


# ---- the numpy restatement against closed forms -------------------------------------------------------------------------
def test_integer_weights_are_a_power_of_two_scaling():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 4097, 100_000):
        w = 50 + 50 * rng.random(n)
        q = ref.integer_weights(w)
        bits = int(n).bit_length()
        assert q.dtype == np.uint64 and int(q.max()) < 2 ** (62 - bits) and int(q.max()) >= 2 ** (61 - bits)
        assert int(q.sum(dtype=np.uint64)) < 2 ** 62
        scale = 2.0 ** (61 - bits - int(np.floor(np.log2(w.max()))))  # (w_max 2^-(61 - B) is one unit of q)
        assert np.all(q.astype(float) <= w * scale) and np.all(w * scale - q.astype(float) < 1.0 + 1e-9 * w * scale)
    assert np.all(ref.integer_weights(np.zeros(5)) == 0) and len(ref.integer_weights(np.zeros(0))) == 0
    # a weight below w_max 2^-(61 - B) counts nothing
    assert list(ref.integer_weights([1.0, 2.0 ** -60, 2.0 ** -57])) == [2 ** 59, 0, 4]


def test_restatement_on_a_vogel_disk_and_a_square_lattice():
    n, a = 10_000, 0.37
    p, r = ref.vogel_disk(n, a)
    s, w = np.zeros((n, 2)), np.ones(n)
    radii = ref.clear_radii(r, 50)
    fractions = np.array([0.1, 0.5, 0.8, 0.9, 1.0])
    energy, radius, margin = ref.enclosed(p, s, w, radii, fractions, follow_centroid=False)
    assert margin > 1e-9
    assert np.abs(energy[0] - (radii / a) ** 2).max() <= 1.0 / n
    want = a * np.sqrt((np.ceil(fractions * n) - 0.5) / n)
    np.testing.assert_allclose(radius[0], want, rtol=1e-12)
    assert radius[0, -1] == np.sqrt((p * p).sum(1)).max()  # (phi = 1: the largest distance, a ray's own)
    # a uniform lattice on the square of half-width a: ensquared EE(h) = (h / a)^2 to within the cells a boundary cuts
    side = 100
    grid = (np.arange(side) + 0.5) / side * 2 * a - a
    lattice = np.stack(np.meshgrid(grid, grid, indexing="ij"), -1).reshape(-1, 2)
    half = ref.clear_radii(np.abs(lattice).max(1), 20)
    energy, radius, margin = ref.enclosed(lattice, np.zeros_like(lattice), np.ones(len(lattice)), half, [0.25, 1.0],
                                          shape="square", follow_centroid=False)
    assert margin > 1e-9
    # the rays inside h are a (2k)^2 block of cells of width 2a / side: |EE - (h/a)^2| <= 4 (h/a) / side + 4 / side^2
    assert np.all(np.abs(energy[0] - (half / a) ** 2) <= 4 * (half / a) / side + 4 / side ** 2)
    np.testing.assert_allclose(radius[0], [grid[74], grid[99]], rtol=1e-12)  # (ceil(0.25 N) rays: the 50 x 50 block)
    # slits see one coordinate each
    e1, r1, _ = ref.enclosed(lattice, np.zeros_like(lattice), np.ones(len(lattice)), [a / 2 + 1e-4], [0.5],
                             shape="slit_e2", follow_centroid=False)
    assert e1[0, 0] == 0.5 and abs(r1[0, 0] - grid[74]) <= 1e-12 * grid[74]


def test_restatement_through_focus_ties_and_extremes():
    # a perfect cone converging at delta0: the radius is |delta - delta0| times the slope quantile
    n, delta0 = 4001, 0.25
    _, slope = ref.vogel_disk(n, 0.1)
    t = np.arange(n) * 2.399963229728653
    s = np.stack([slope * np.cos(t), slope * np.sin(t)], 1)
    p = -delta0 * s
    focus = np.array([0.0, 0.125, 0.25, 0.5])
    _, radius, _ = ref.enclosed(p, s, np.ones(n), (), [0.8], focus, follow_centroid=False)
    quantile = np.sort(np.hypot(s[:, 0], s[:, 1]))[int(np.ceil(0.8 * n)) - 1]
    np.testing.assert_allclose(radius[:, 0], np.abs(focus - delta0) * quantile, rtol=1e-12, atol=1e-18)
    # many equal distances: the radius lands on the ring for every fraction
    ring = np.stack([np.full(64, 3.0), np.zeros(64)], 1)
    ring[::2] *= -1
    _, radius, _ = ref.enclosed(ring, np.zeros_like(ring), np.arange(1.0, 65.0), (), [0.01, 0.5, 1.0],
                                follow_centroid=False)
    assert np.all(radius == 3.0)
    # an overflowing distance is +inf: outside every radius, last in the order
    far = np.array([[1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [1e300, 1e300]])
    energy, radius, _ = ref.enclosed(far, np.zeros_like(far), np.ones(4), [2.5, 1e308], [0.5, 0.75, 1.0],
                                     follow_centroid=False)
    assert list(energy[0]) == [0.5, 0.75] and list(radius[0]) == [2.0, 3.0, np.inf]
    # no weight: NaN
    energy, radius, _ = ref.enclosed(far, np.zeros_like(far), np.zeros(4), [2.5], [0.5])
    assert np.all(np.isnan(energy)) and np.all(np.isnan(radius))
