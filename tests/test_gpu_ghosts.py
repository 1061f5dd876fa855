"""Ghost rays on the device (DeviceFrame.ghosts, RayTracer.trace_ghosts): the bits of the numpy restatement
(tests/ghost_reference.py) on GPU traces of three scenes, on synthetic frames at every size where the pass takes another
path, under permuted rows, and end to end against the C oracle's trace of the reference's children."""
import numpy as np
import pytest

import fresnel_reference as fref
import ghost_reference as ref
import ghost_scenes as gs
import helpers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = fref.IX
X = np.array([1.0, 0.0, 0.0])
COUNTERS = ("n_spawned", "n_dropped", "n_dark", "n_invalid", "n_open")
# csrc: kFresnelBlock = PRT_BLOCK = 256 (four waves of 64), kWfRowsPerWave = 1024 and kWfMaxWaves = 2048 (sort_plan),
# kSortScanBlock = 512 (the scans' threads: one wave's counts each up to there), kGhostCountBytes = 64 MiB of
# (wave, bucket) counts of 8 bytes
WAVE, BLOCK, ROWS_PER_WAVE, MAX_WAVES, SCAN, COUNT_BYTES = 64, 256, 1024, 2048, 512, 64 << 20


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else [0]
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def agree(got, want, what):
    """Rays, parent_row, keys, counts, stride and counters: the reference's, bit for bit."""
    assert tuple(getattr(got, name) for name in COUNTERS) == tuple(want[name] for name in COUNTERS), what
    assert got.counts.tolist() == want["counts"].tolist(), what
    assert (got.stride, got.n_groups) == (want["stride"], want["n_groups"]), what
    assert got.keys.tolist() == want["keys"].tolist() and got.bucket.tolist() == want["bucket"].tolist(), what
    assert got.parent_row.cpu().numpy().tolist() == want["parent_row"].tolist(), what
    helpers.assert_same_bits(got.rays.cpu().numpy(), want["rays"], what)


def both(device, surfaces, fresnel_options=None, **options):
    """(device result, reference on the downloaded frame and transmittance)."""
    fresnel = device.fresnel(**(fresnel_options or {}))
    got = device.ghosts(fresnel, surfaces, **options)
    reference = dict(options)
    reference["rays_per_group"] = reference.pop("rays_per_source", None)
    want = ref.ghosts(device.rows.cpu().numpy().T, fresnel.transmittance.cpu().numpy(), surfaces, **reference)
    return got, want


# ---- GPU traces of three scenes ---------------------------------------------------------------------------------------------
def traced(parts, rays, limit=10):
    from pyrayt_amd.engine import DeviceScene
    from pyrayt_amd.frame import DeviceFrame
    from pyrayt_amd.scene import SceneSnapshot

    scene = DeviceScene(SceneSnapshot(parts))
    rows, counts = scene.trace(torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0"), limit)
    return DeviceFrame(rows, counts)


SCENES = {"lens": lambda: gs.lens(257), "stopped_lens": lambda: gs.stopped_lens(300), "prism": lambda: gs.prism(40)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_children_of_a_traced_frame_are_the_references(name):
    from pyrayt_amd.materials import Coating

    parts, rays, det = SCENES[name]()
    glass = gs.refracting(parts)
    device = traced(parts, rays)
    per_group = rays.shape[1] // (4 if name == "prism" else 1)
    groups = dict(rays_per_source=per_group, n_groups=rays.shape[1] // per_group)
    got, want = both(device, glass, **groups)
    agree(got, want, name)
    assert got.n_spawned > 100 and got.n_invalid == 0 and got.n_groups >= 2
    if name == "lens":
        assert got.n_spawned == 2 * 257 and got.n_open == 0
    if name == "prism":
        assert len(set(got.rays[10].cpu().tolist())) == 4 and got.n_groups >= 4
    met = [s for s in glass if bool((device["surface"] == s).any())]  # (the glass surfaces the rays meet)
    for label, fresnel_options in (("polarised", dict(polarization=(0.3, 1.0, -0.2))), ("lossless", dict(lossless=met[:1])),
                                   ("coated", dict(coatings={tuple(met): Coating.quarter_wave(1.38, 0.55)}))):
        other, wanted = both(device, glass, fresnel_options, **groups)
        agree(other, wanted, f"{name}, {label}")
        assert not torch.equal(other.rays[9], got.rays[9]) or label == "polarised"
    weak = float(got.rays[9].median())
    agree(*both(device, glass[::-1], min_intensity=weak, ray_offset=1e-3, **groups), f"{name}, threshold")
    again = device.ghosts(device.fresnel(), glass, **groups)
    assert torch.equal(again.rays.view(torch.int64), got.rays.view(torch.int64)) and torch.equal(again.parent_row, got.parent_row)


# ---- synthetic frames at the partition edges ---------------------------------------------------------------------------------
def plates(n_rows, children=None, groups=1, n_surfaces=2, id0=0, seed=11):
    """A whole frame of exactly n_rows rows: rays through a plate (surfaces 1, 2, then 3), three rows each as far as
    they go; interfaces beyond the first `children` (in frame order, None: all) lie on surface 9, which is not listed.
    With n_surfaces > 2 the faces' ids cycle through 1 .. n_surfaces."""
    rng = np.random.default_rng(seed + n_rows)
    n0 = -(-n_rows // 3)
    n1 = -(-(n_rows - n0) // 2)
    n2 = n_rows - n0 - n1
    theta, azimuth = rng.uniform(0.05, 1.2, n0), rng.uniform(0, 2 * np.pi, n0)
    index = rng.choice([1.46, 1.5, 1.8], n0)
    u = np.stack([np.cos(theta), np.sin(theta) * np.cos(azimuth), np.sin(theta) * np.sin(azimuth)])
    sin_t = np.sin(theta) / index
    inside = np.stack([np.sqrt(1 - sin_t ** 2), u[1] / index, u[2] / index])
    frame = np.zeros((n_rows, 15))
    start = 0
    for g, (count, direction, medium) in enumerate(((n0, u, np.ones(n0)), (n1, inside, index), (n2, u, np.ones(n0)))):
        block = slice(start, start + count)
        frame[block, IX["generation"]], frame[block, IX["id"]] = g, id0 + np.arange(count)
        frame[block, IX["intensity"]] = rng.uniform(50.0, 100.0, count)
        frame[block, IX["wavelength"]], frame[block, IX["index"]] = 0.633, medium[:count]
        frame[block, IX["surface"]] = (g + np.arange(count)) % n_surfaces + 1 if n_surfaces > 2 else g + 1
        frame[block, 9:12], frame[block, 12:15] = rng.normal(size=(count, 3)), direction[:, :count].T
        start += count
    if children is not None:
        followed = np.concatenate([np.arange(n1), n0 + np.arange(n2)])  # (rows with a successor, in frame order)
        frame[followed[children:], IX["surface"]] = 9
    return frame


def grouping(frame, groups):
    n0 = int((frame[:, 0] == 0).sum())
    per_group = max(1, -(-n0 // groups))
    return dict(rays_per_source=per_group, n_groups=groups) if groups > 1 else {}


ROW_COUNTS = sorted({1, 2, 3, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK - 1, 3 * BLOCK, 3 * BLOCK + 1,
                     ROWS_PER_WAVE - 1, ROWS_PER_WAVE, ROWS_PER_WAVE + 1, 4 * ROWS_PER_WAVE, 4 * ROWS_PER_WAVE + 1})
BIG_ROW_COUNTS = [SCAN * ROWS_PER_WAVE - 1, SCAN * ROWS_PER_WAVE + 1, MAX_WAVES * ROWS_PER_WAVE, MAX_WAVES * ROWS_PER_WAVE + 1]


@pytest.mark.parametrize("n_rows", ROW_COUNTS + BIG_ROW_COUNTS)
def test_row_counts_on_either_side_of_the_blocks_and_of_the_sort_plan(n_rows):
    frame = plates(n_rows)
    device = device_frame(frame)
    got, want = both(device, [1, 2], **grouping(frame, 3))
    agree(got, want, f"{n_rows} rows")
    assert got.n_spawned == int((frame[:, 0] > 0).sum())
    second = device.ghosts(device.fresnel(), [1, 2], **grouping(frame, 3))
    assert torch.equal(second.rays.view(torch.int64), got.rays.view(torch.int64)) and torch.equal(second.parent_row, got.parent_row)


@pytest.mark.parametrize("children", [0, 1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_child_counts_on_either_side_of_a_wave_and_a_block(children):
    frame = plates(3 * BLOCK + 5, children=children)
    got, want = both(device_frame(frame), [2, 1], **grouping(frame, 2))
    agree(got, want, f"{children} children")
    assert len(got) == children and got.rays.shape == (13, children)


def test_an_empty_frame_one_bucket_many_buckets_and_the_last_bucket():
    from pyrayt_amd.frame import DeviceFrame

    empty = DeviceFrame(torch.zeros((15, 0), dtype=torch.float64, device="cuda:0"), [0])
    got = empty.ghosts(empty.fresnel(), [1, 2])
    assert len(got) == 0 and got.n_groups == 0 and got.stride == 0 and got.keys.shape == (0, 2) and got.n_open == 0
    frame = plates(2000)
    agree(*both(device_frame(frame), [2]), "one bucket")
    wide = plates(5000, n_surfaces=64)
    got, want = both(device_frame(wide), list(range(1, 65)), **grouping(wide, 5))
    agree(got, want, "64 surfaces x 5 groups")
    assert got.n_groups > 200
    last = plates(1500, id0=0)
    last[:, IX["id"]] += 4000  # (every ray in the last of five groups of 1000)
    got, want = both(device_frame(last), [7, 2], rays_per_source=1000, n_groups=5)
    agree(got, want, "the last bucket")
    assert got.bucket.tolist() == [9] and got.keys.tolist() == [[4, 2]]


def test_more_buckets_than_the_counts_cap_gives_every_wave():
    """65472 buckets of 8 bytes: 64 MiB hold 128 waves' counts, and 131073 rows would have 129 waves."""
    n_surfaces, n_groups = 64, 1023
    waves = COUNT_BYTES // (n_surfaces * n_groups * 8)
    assert waves == 128
    frame = plates(waves * ROWS_PER_WAVE + 1, n_surfaces=64)
    n0 = int((frame[:, 0] == 0).sum())
    got, want = both(device_frame(frame), list(range(1, 65)), rays_per_source=-(-n0 // n_groups), n_groups=n_groups)
    agree(got, want, "the counts' cap")
    assert got.n_groups > 30000


def test_rows_permuted_inside_a_generation_give_the_same_children():
    frame = plates(3001, seed=4)
    rng = np.random.default_rng(3)
    counts = np.bincount(frame[:, 0].astype(int))
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = np.concatenate([starts[g] + rng.permutation(counts[g]) for g in range(len(counts))])  # new row -> old row
    options = dict(rays_per_source=334, n_groups=3)
    first, shuffled = device_frame(frame), device_frame(frame[order])
    a, b = first.ghosts(first.fresnel(), [1, 2], **options), shuffled.ghosts(shuffled.fresnel(), [1, 2], **options)
    agree(b, ref.ghosts(frame[order], shuffled.fresnel().transmittance.cpu().numpy(), [1, 2], rays_per_group=334, n_groups=3),
          "shuffled")

    def children(result, rows):
        payload = result.rays.cpu().numpy()
        parents = rows[result.parent_row.cpu().numpy()]
        lines = np.concatenate([parents[:, [IX["id"], IX["surface"]]], payload[:12].T], axis=1)
        return lines[np.lexsort(lines.T.view(np.int64)[::-1])], np.floor(payload[12] / result.stride)

    (lines_a, groups_a), (lines_b, groups_b) = children(a, frame), children(b, frame[order])
    assert np.array_equal(lines_a.view(np.int64), lines_b.view(np.int64)) and len(lines_a) == a.n_spawned > 1500
    assert a.counts.tolist() == b.counts.tolist() and sorted(groups_a) == sorted(groups_b)
    assert not torch.equal(a.parent_row, b.parent_row)


def test_frames_the_definitions_refuse_leave_nothing_behind():
    frame = plates(600)
    device = device_frame(frame)
    bad = frame.copy()
    bad[5, IX["id"]] = bad[6, IX["id"]]
    with pytest.raises(ValueError, match="repeats within a generation"):
        both(device_frame(bad), [1, 2])
    with pytest.raises(ValueError, match="not below n_groups"):
        device.ghosts(device.fresnel(), [1, 2], rays_per_source=10, n_groups=3)
    with pytest.raises(ValueError, match="this very frame"):
        device.ghosts(device_frame(frame).fresnel(), [1, 2])
    agree(*both(device, [1, 2]), "after the refusals")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def lens_tracer(n, housing=True):
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-2)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    parts = [lens, det] + ([pyrayt.ghosts.housing(gs.HOUSING)] if housing else [])
    return pyrayt.RayTracer(src, parts, rays_per_source=n), lens, det, parts


def oracle_children(analysis, parts, k, surfaces, **options):
    """The reference's children of order k from the device's frame and transmittance of order k - 1, and the C oracle's
    trace of them."""
    from oracle import c_oracle

    before = analysis.orders[k - 1]
    stride, groups = analysis._grouping(k - 1)
    want = ref.ghosts(before.frame.rows.cpu().numpy().T, before.fresnel.transmittance.cpu().numpy(), surfaces,
                      rays_per_group=stride, n_groups=groups, **options)
    frame, _ = c_oracle.trace(gs.flat(parts), want["rays"], 10)
    return want, frame


def detector_energy(order, det):
    """The longdouble sum of intensity * transmittance (one product a row, as apply() forms it) on the detector."""
    frame = order.frame.rows.cpu().numpy().T
    on = frame[:, IX["surface"]] == det.get_id()
    return ref.energy(frame[on, IX["intensity"]] * order.fresnel.transmittance.cpu().numpy()[on]), int(on.sum())


def test_trace_ghosts_end_to_end_against_the_oracle():
    from pyrayt_amd.materials import Coating

    tracer, lens, det, parts = lens_tracer(500)
    glass = gs.refracting(parts)
    plain = tracer.trace().to_numpy(dtype=float)
    kept, settings = tracer.device_frame, tracer.record_only(det)._record_surfaces
    analysis = tracer.trace_ghosts(det, order=2)
    assert tracer.device_frame is kept and tracer._record_surfaces == settings
    assert len(analysis.orders) == 3 and [len(o.frame) for o in analysis.orders] == [1500, 1500, 1000]
    for k in (1, 2):
        want, frame = oracle_children(analysis, parts, k, glass)
        agree(analysis.orders[k].ghosts, want, f"order {k}")
        helpers.assert_frames_identical(analysis.orders[k].frame.rows.cpu().numpy().T, frame, f"the frame of order {k}")
    front, back = int(plain[0, IX["surface"]]), int(plain[500, IX["surface"]])
    table = analysis.table()
    assert len(table) == 1 and table.loc[0, "surfaces"] == (back, front) and table.loc[0, "order"] == 2
    assert table.loc[0, "source"] == 0 and table.loc[0, "rays"] == 500 and analysis.path(2, 0) == ((back, front), 0)
    energy, rays = detector_energy(analysis.orders[2], det)
    signal, _ = detector_energy(analysis.orders[0], det)
    print(f"ghost (back, front): {table.loc[0, 'energy']!r} against {energy!r}; share {table.loc[0, 'share']:.3e}")
    assert rays == 500 and np.isclose(table.loc[0, "energy"], float(energy), rtol=1e-12, atol=1e-12)  # (test_gpu_frame.py's bar)
    assert np.isclose(table.loc[0, "share"], float(energy / signal), rtol=1e-12, atol=0.0) and 1e-4 < table.loc[0, "share"] < 5e-3
    image, y_edges, z_edges = analysis.image(bins=8, range=((-0.5, 0.5), (-0.5, 0.5)))
    assert image.shape == (8, 8) and np.isclose(image.sum(), float(energy), rtol=1e-12)
    applied = analysis.frame(2)
    assert applied.rows_per_generation == analysis.orders[2].frame.rows_per_generation
    # a quarter-wave layer of MgF2 on the lens: less ghost, and still its own reference's
    quarter = Coating.quarter_wave(1.38, 0.55)
    coated = tracer.trace_ghosts(det, order=2, fresnel=dict(coatings={lens: quarter}))
    for k in (1, 2):
        want, frame = oracle_children(coated, parts, k, glass)
        agree(coated.orders[k].ghosts, want, f"coated, order {k}")
        helpers.assert_frames_identical(coated.orders[k].frame.rows.cpu().numpy().T, frame, f"coated, the frame of order {k}")
    coated_table = coated.table()
    coated_energy, _ = detector_energy(coated.orders[2], det)
    assert len(coated_table) == 1 and coated_table.loc[0, "surfaces"] == (back, front)
    assert np.isclose(coated_table.loc[0, "energy"], float(coated_energy), rtol=1e-12, atol=1e-12)
    assert coated_table.loc[0, "energy"] < 0.5 * table.loc[0, "energy"]
    # a threshold relative to the launch intensity: the second reflection carries 4 % of 4 %
    few = tracer.trace_ghosts(det, order=2, min_share=0.01)
    assert len(few.orders) == 2 and few.orders[1].ghosts.n_dropped == 0 and len(few.table()) == 0
    tracer.record_only()
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), plain, equal_nan=True)


def test_strict_needs_the_housing():
    tracer, lens, det, parts = lens_tracer(64, housing=False)
    with pytest.raises(ValueError, match=r"housing\(radius\)"):
        tracer.trace_ghosts(det, order=2)
    loose = tracer.trace_ghosts(det, order=2, strict=False)
    assert len(loose.orders) == 2 and len(loose.table()) == 0  # (order 1 ends unseen on the front surface: no order 2)
    assert loose.orders[1].ghosts.n_open == 0 and len(loose.orders[1].frame) == 64
