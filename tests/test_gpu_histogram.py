"""Histograms of the result frame on the device (DeviceFrame.histogram / histogram2d, RayTracer.trace_histogram)
against numpy on the reference's own frames (tests/golden/scene_*.npz) and on synthetic frames built to sit on the
bin rule's edges.  Counts are compared exactly, with no tolerance; intensity-weighted sums too (every source emits
intensity 100); other weights at 1e-12 relative."""
import os
import socket

import numpy as np
import pytest

import helpers
import scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}


def device_frame(golden):
    from pyrayt_amd.frame import DeviceFrame

    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(np.asarray(golden, dtype=np.float64).T)).to("cuda:0"))


def values(rows, name):
    if name == "axis_intercept":
        with np.errstate(all="ignore"):
            return rows[:, IX["x0"]] - rows[:, IX["x_tilt"]] * rows[:, IX["y0"]] / rows[:, IX["y_tilt"]]
    return rows[:, IX[name]]


def finite_range(v):
    f = v[np.isfinite(v)]
    return (float(f.min()), float(f.max())) if f.size else (0.0, 1.0)


def reference(frame, names, bins, range_, weights=None, density=False, surface=None, generation=None,
              rays_per_source=None, n_groups=None):
    """numpy on the selected rows (the automatic range over their finite values), per group."""
    sel = frame
    if surface is not None:
        sel = sel[sel[:, IX["surface"]] == surface]
    if generation == "last":
        generation = frame[:, 0].max() if len(frame) else 0
    if generation is not None:
        sel = sel[sel[:, IX["generation"]] == generation]
    vals = [values(sel, name) for name in names]
    if range_ is None:
        range_ = [None] * len(names) if len(names) == 2 else None
    if len(names) == 1:
        if range_ is None and np.ndim(bins) == 0:
            range_ = finite_range(vals[0])
    else:
        range_ = list(range_)
        try:  # (np.histogram2d's reading of `bins`)
            count = len(bins)
        except TypeError:
            count = 1
        per_axis = list(bins) if count == 2 else [bins, bins]
        for axis in (0, 1):
            if range_[axis] is None and np.ndim(per_axis[axis]) == 0:
                range_[axis] = finite_range(vals[axis])
    groups = np.floor(sel[:, IX["id"]] / rays_per_source) if rays_per_source else np.zeros(len(sel))
    out = []
    for g in range(n_groups or 1):
        m = groups == g
        w = None if weights is None else sel[m, IX[weights]]
        if len(names) == 1:
            h, *edges = np.histogram(vals[0][m], bins=bins, range=range_, weights=w, density=density)
        else:
            h, *edges = np.histogram2d(vals[0][m], vals[1][m], bins=bins, range=range_, weights=w, density=density)
        out.append(h)
    hist = np.stack(out) if rays_per_source else out[0]
    return hist, edges


def check(frame, device, names, bins=10, range_=None, weights=None, exact=True, **select):
    args = dict(bins=bins, range=range_, weights=weights, **select)
    try:
        want, want_edges = reference(frame, names, bins, range_, weights, **select)
    except ValueError as error:  # (e.g. too many bins for a tiny range): the same error, from the same numpy
        with pytest.raises(ValueError, match=str(error)):
            device.histogram(names[0], **args) if len(names) == 1 else device.histogram2d(names[0], names[1], **args)
        return None
    got = device.histogram(names[0], **args) if len(names) == 1 else device.histogram2d(names[0], names[1], **args)
    hist, edges = got[0], got[1:]
    assert hist.dtype == np.float64 and hist.shape == want.shape, (hist.shape, want.shape)
    for e, w in zip(edges, want_edges):
        assert np.array_equal(e, w)
    if exact:
        assert np.array_equal(hist, want), (names, bins, range_, weights, select, np.abs(hist - want).max())
    else:
        assert np.allclose(hist, want, rtol=1e-12, atol=0), (names, weights, select)
    return hist


FIXTURES = ["config2", "config3", "config4", "mirrors_and_stops", "adv_prism"]


@pytest.mark.parametrize("name", FIXTURES)
def test_histograms_of_the_reference_frames(name):
    fx = helpers.load(f"scene_{name}.npz")
    frame = fx["frame"]
    device = device_frame(frame)
    last = frame[:, 0].max()
    imager = float(frame[frame[:, 0] == last][-1, IX["surface"]])
    rps = 256 if name == "config4" else 512
    n_groups = int(frame[:, IX["id"]].max() // rps) + 1
    for surface in (None, imager):
        for generation in (None, 1.0, "last"):
            select = dict(surface=surface, generation=generation)
            for names in (("y1",), ("y1", "z1"), ("x0",), ("axis_intercept",), ("z1", "axis_intercept")):
                check(frame, device, names, 10, None, **select)
                explicit = [finite_range(values(frame, q)) for q in names]
                check(frame, device, names, 17, explicit[0] if len(names) == 1 else explicit, **select)
            check(frame, device, ("y1",), 7, None, rays_per_source=rps, n_groups=n_groups, **select)
            check(frame, device, ("y1", "z1"), (5, 9), None, rays_per_source=rps, n_groups=n_groups, **select)
            check(frame, device, ("y1", "z1"), 12, None, weights="intensity", **select)
            check(frame, device, ("y1", "z1"), 12, None, weights="wavelength", exact=False, **select)
            check(frame, device, ("y1",), 12, None, weights="wavelength", exact=False, rays_per_source=rps,
                  n_groups=n_groups, **select)
    # explicit, uneven edges (with a repeated one) and density
    y = values(frame, "y1")
    lo, hi = finite_range(y)
    uneven = np.unique(np.concatenate([[lo - 0.1], np.quantile(y, [0.1, 0.3, 0.31, 0.8]), [hi]]))
    uneven = np.insert(uneven, 2, uneven[2])
    check(frame, device, ("y1",), uneven, None)
    check(frame, device, ("y1", "z1"), [uneven, np.linspace(-0.5, 0.5, 6)], None, surface=imager)
    for names in (("y1",), ("y1", "z1")):
        check(frame, device, names, 8, None, density=True, exact=False)
        check(frame, device, names, 8, None, weights="intensity", density=True, exact=False)


def test_the_axis_intercept_skips_rays_parallel_to_the_axis():
    frame = helpers.load("scene_config2.npz")["frame"].copy()
    frame[::7, IX["y_tilt"]] = 0.0          # rays parallel to the axis: 0 / 0 or +-inf, no intercept
    frame[::14, IX["y0"]] = 0.0
    device = device_frame(frame)
    hist, _ = device.histogram("axis_intercept", bins=10)
    assert hist.sum() == np.isfinite(values(frame, "axis_intercept")).sum() < len(frame)
    check(frame, device, ("axis_intercept",), 10, None)
    check(frame, device, ("y1", "axis_intercept"), 6, None, weights="intensity")


def synthetic(columns, n=None):
    """A (R, 15) frame: the given columns, the rest zeros (id = row number unless given)."""
    n = n or len(next(iter(columns.values())))
    rows = np.zeros((n, 15))
    rows[:, IX["id"]] = np.arange(n)
    for name, v in columns.items():
        rows[:, IX[name]] = v
    return rows


def test_values_on_every_edge_and_one_ulp_either_side():
    for edges in (np.linspace(-1.0, 1.0, 17), np.linspace(0.1, 0.7, 7), np.array([-2.0, -0.3, 0.0, 0.0, 1e-9, 4.0])):
        special = np.array([edges[0] - 1, edges[-1] + 1, np.nan, np.inf, -np.inf, edges[-1], edges[-1]])
        v = np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf), special])
        w = np.concatenate([edges[::-1], special[::-1], edges, edges])[:len(v)]
        frame = synthetic({"y1": v, "z1": w, "intensity": np.arange(len(v)) % 7})
        device = device_frame(frame)
        check(frame, device, ("y1",), edges, None)
        check(frame, device, ("y1", "z1"), [edges, edges], None, weights="intensity")
        if np.allclose(np.diff(edges), np.diff(edges)[0]):  # the arithmetic guess, corrected against the edges
            check(frame, device, ("y1",), len(edges) - 1, (edges[0], edges[-1]))
            check(frame, device, ("y1", "z1"), len(edges) - 1, [(edges[0], edges[-1])] * 2, weights="intensity")
        # the automatic range over the finite values: numpy raises for NaN / inf without a range (the divergence)
        with pytest.raises(ValueError):
            np.histogram(v, bins=4)
        hist, got_edges = device.histogram("y1", bins=4)
        assert np.array_equal(got_edges, np.histogram_bin_edges(v[np.isfinite(v)], bins=4))
        assert np.array_equal(hist, np.histogram(v[np.isfinite(v)], bins=4)[0])


def test_empty_selections_and_a_single_value():
    frame = synthetic({"y1": np.linspace(0, 1, 100), "z1": np.full(100, 2.5), "surface": np.full(100, 3.0)})
    device = device_frame(frame)
    hist, edges = device.histogram("y1", bins=5, surface=7)
    assert np.array_equal(hist, np.zeros(5)) and np.array_equal(edges, np.linspace(0, 1, 6))
    hist, xedges, yedges = device.histogram2d("y1", "z1", bins=3, surface=7, range=((0, 1), None))
    assert not hist.any() and np.array_equal(yedges, np.linspace(0, 1, 4))
    empty = device_frame(np.zeros((0, 15)))
    hist, edges = empty.histogram("y1", bins=4)
    assert np.array_equal(hist, np.zeros(4)) and np.array_equal(edges, np.histogram(np.empty(0), bins=4)[1])
    hist, edges = device.histogram("z1", bins=4)  # one distinct value: (v - 0.5, v + 0.5)
    want = np.histogram(np.full(100, 2.5), bins=4)
    assert np.array_equal(hist, want[0]) and np.array_equal(edges, want[1])


def test_groups_and_ids_beyond_them():
    rng = np.random.default_rng(5)
    n = 50_000
    frame = synthetic({"y1": rng.normal(size=n), "z1": rng.normal(size=n), "intensity": np.full(n, 100.0),
                       "id": rng.integers(-30, 1300, n).astype(float)})
    device = device_frame(frame)
    for n_groups in (1, 5, 13, 20):
        check(frame, device, ("y1",), 33, (-2, 2), rays_per_source=100, n_groups=n_groups)
        check(frame, device, ("y1", "z1"), 19, None, weights="intensity", rays_per_source=100, n_groups=n_groups)
    hist, _ = device.histogram("y1", bins=4, range=(-10, 10), rays_per_source=100)  # default: highest id // rps + 1
    assert hist.shape == (13, 4) and hist.sum() == ((frame[:, IX["id"]] >= 0)).sum()


def test_more_bins_than_one_window():
    rng = np.random.default_rng(9)
    n = 1_000_000
    frame = synthetic({"y1": rng.uniform(-1, 1, n), "z1": rng.normal(0, 0.4, n), "intensity": np.full(n, 100.0),
                       "id": rng.integers(0, 4 * 250_000, n).astype(float)})
    device = device_frame(frame)
    check(frame, device, ("y1", "z1"), 1024, [(-1, 1), (-1, 1)], rays_per_source=250_000, n_groups=4)
    for nx in (32767, 32768, 32769, 65535, 65536, 65537):  # around the counts-only windows (32-bit and 16-bit tallies)
        check(frame, device, ("y1",), nx, (-1, 1))
    for nx in (10921, 10922, 10923):      # around the window with weight sums
        check(frame, device, ("y1",), nx, (-1, 1), weights="intensity")
    check(frame, device, ("y1", "z1"), 300, None, weights="intensity", rays_per_source=250_000, n_groups=4)


def test_the_same_call_twice_gives_the_same_bits():
    rng = np.random.default_rng(1)
    n = 1_000_000
    frame = synthetic({"y1": rng.normal(0, 0.01, n), "z1": rng.normal(0, 0.01, n), "intensity": np.full(n, 100.0)})
    device = device_frame(frame)
    for weights in (None, "intensity"):
        a = device.histogram2d("y1", "z1", bins=256, weights=weights)[0]
        b = device.histogram2d("y1", "z1", bins=256, weights=weights)[0]
        assert np.array_equal(a, b) and a.sum() == n * (100 if weights else 1)


def test_a_frame_recorded_with_a_column_list_needs_its_columns():
    from pyrayt_amd.frame import DeviceFrame

    frame = synthetic({"y1": np.linspace(0, 1, 10)})
    device = DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)).to("cuda:0"), None, (IX["y1"], IX["z1"]))
    assert device.histogram("y1", bins=2)[0].sum() == 10
    with pytest.raises(KeyError):
        device.histogram("y1", bins=2, weights="intensity")
    with pytest.raises(KeyError):
        device.histogram("axis_intercept", bins=2)
    with pytest.raises(KeyError):
        device.histogram2d("y1", "z1", bins=2, surface=3)


# ---- RayTracer.trace_histogram ---------------------------------------------------------------------------------------
def test_trace_histogram_at_a_million_rays():
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=1_000_000)
    whole = tracer.trace().to_numpy(dtype=float)
    rows = whole[whole[:, IX["surface"]] == det.get_id()]
    y, z = rows[:, IX["y1"]], rows[:, IX["z1"]]
    box = ((-0.5, 0.5), (-0.5, 0.5))
    hist, ye, ze = tracer.trace_histogram("y1", "z1", surface=det, bins=256, range=box, weights="intensity")
    want = np.histogram2d(y, z, bins=256, range=box, weights=rows[:, IX["intensity"]])
    assert np.array_equal(hist, want[0]) and np.array_equal(ye, want[1]) and hist.sum() > 0
    hist, ye, ze = tracer.trace_histogram("y1", "z1", surface=det, bins=256)
    want = np.histogram2d(y, z, bins=256)
    assert np.array_equal(hist, want[0]) and np.array_equal(ye, want[1]) and np.array_equal(ze, want[2])
    hist, edges = tracer.trace_histogram("y1", surface=det)   # cell 19
    assert np.array_equal(hist, np.histogram(y, bins=10)[0])
    again = tracer.trace().to_numpy(dtype=float)
    assert np.array_equal(again, whole, equal_nan=True)
    # an active record_only() setting survives the call
    tracer.record_only(det, columns=("y1", "z1"))
    spot = tracer.trace().to_numpy(dtype=float)
    tracer.trace_histogram("z1", surface=lens, bins=5, generation="last")
    assert tracer._record_surfaces == (det.get_id(),) and tracer._record_columns == ("y1", "z1")
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), spot)


class PresetSource:
    """A user's own source: the fixture's rays, from the host."""

    wavelength = 0.633

    def __init__(self, rays):
        self._rays = rays

    def generate_rays(self, n):
        from pyrayt_amd import RaySet

        return self._rays.copy().view(RaySet)


def fixture_tracer(name, *args):
    import pyrayt_amd as pyrayt
    from pyrayt_amd.g3d.objects import CountedObject

    fx = helpers.load(f"scene_{name}.npz")
    CountedObject.reset_ids()
    parts, rays = scenes.SCENES[name](scenes.product_api(), *args)
    assert np.array_equal(rays, fx["rays0"])
    tracer = pyrayt.RayTracer(PresetSource(rays), parts, rays_per_source=rays.shape[1],
                              generation_limit=int(fx["generation_limit"]))
    return tracer, fx["frame"]


def test_trace_histogram_of_a_multi_source_scene():
    tracer, frame = fixture_tracer("config4", 256)   # one LineOfRays per wavelength: 8 x 256 rays
    imager = 5
    hist, _, _ = tracer.trace_histogram("y1", "z1", surface=imager, bins=(6, 4), rays_per_source=256, n_groups=8,
                                        weights="intensity")
    want, _ = reference(frame, ("y1", "z1"), (6, 4), None, "intensity", surface=imager, rays_per_source=256,
                        n_groups=8)
    assert hist.shape == (8, 6, 4) and np.array_equal(hist, want) and hist.sum() > 0
    hist, _ = tracer.trace_histogram("wavelength", surface=imager, bins=8, rays_per_source=True)
    assert hist.shape == (1, 8)
    assert np.array_equal(hist[0], reference(frame, ("wavelength",), 8, None, surface=imager)[0])


def test_trace_histogram_on_the_stepwise_path():
    tracer, frame = fixture_tracer("custom_retro", 10)   # a user-defined Material.trace(): the plan is applied afterwards
    for surface in (1, 2, None):
        sel = frame if surface is None else frame[frame[:, IX["surface"]] == surface]
        hist, _ = tracer.trace_histogram("y1", surface=surface, bins=4)
        assert np.array_equal(hist, np.histogram(values(sel, "y1"), bins=4)[0])
        hist, _, _ = tracer.trace_histogram("y1", "z1", surface=surface, bins=3, generation="last")
        last = sel[sel[:, 0] == sel[:, 0].max()]
        assert np.array_equal(hist, np.histogram2d(last[:, IX["y1"]], last[:, IX["z1"]], bins=3)[0])


@pytest.mark.parametrize("name,args,surface", [("config2", (2048,), 1), ("adv_stop", (), None),
                                               ("mirrors_and_stops", (4096,), None)])
def test_last_generation_of_a_surface(name, args, surface):
    """"last" is the highest generation in which a row of the surface was recorded -- the notebook's
    imager_rays.generation.max() -- which comes before the frame's last generation here."""
    tracer, frame = fixture_tracer(name, *args)
    if surface is None:  # a stop: the surface whose last hit is earliest
        ids = np.unique(frame[:, IX["surface"]])
        surface = min(ids, key=lambda s: frame[frame[:, IX["surface"]] == s, 0].max())
    sel = frame[frame[:, IX["surface"]] == surface]
    assert len(sel) and sel[:, 0].max() < frame[:, 0].max()
    last = sel[sel[:, 0] == sel[:, 0].max()]
    hist, ye, ze = tracer.trace_histogram("y1", "z1", surface=float(surface), bins=5, generation="last")
    want = np.histogram2d(last[:, IX["y1"]], last[:, IX["z1"]], bins=5)
    assert np.array_equal(hist, want[0]) and np.array_equal(ye, want[1]) and np.array_equal(ze, want[2])
    hist, _ = tracer.trace_histogram("y1", surface=float(surface), bins=5, range=(-1, 1), generation=1)
    gen1 = sel[sel[:, 0] == 1]
    assert np.array_equal(hist, np.histogram(gen1[:, IX["y1"]], bins=5, range=(-1, 1))[0])


# ---- a frame sharded over ranks ---------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, name, result_dir):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        frame = helpers.load(f"scene_{name}.npz")["frame"]
        ids = frame[:, IX["id"]]
        half = (ids.max() + 1) // 2
        mine = frame[(ids < half) if rank == 0 else (ids >= half)]
        device = device_frame(mine)
        group = dist.group.WORLD
        h2, xe, ye = device.histogram2d("y1", "z1", bins=32, weights="intensity", group=group)
        h1, e1 = device.histogram("axis_intercept", bins=16, rays_per_source=512, group=group, generation="last")
        np.savez(os.path.join(result_dir, f"rank_{rank}.npz"), h2=h2, xe=xe, ye=ye, h1=h1, e1=e1)
    finally:
        dist.destroy_process_group()


def test_a_sharded_frame_gives_the_histogram_of_the_whole(tmp_path):
    import torch.multiprocessing as mp

    name = "mirrors_and_stops"
    mp.start_processes(_shard_worker, args=(2, _free_port(), name, str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    device = device_frame(helpers.load(f"scene_{name}.npz")["frame"])
    h2, xe, ye = device.histogram2d("y1", "z1", bins=32, weights="intensity")
    h1, e1 = device.histogram("axis_intercept", bins=16, rays_per_source=512, generation="last")
    for rank in range(2):
        got = np.load(tmp_path / f"rank_{rank}.npz")
        for key, want in (("h2", h2), ("xe", xe), ("ye", ye), ("h1", h1), ("e1", e1)):
            assert np.array_equal(got[key], want), (rank, key)
