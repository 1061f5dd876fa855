"""Scattered rays on the device (DeviceFrame.scatter, RayTracer.trace_scatter): the bits of the numpy restatement
(tests/scatter_reference.py) on GPU traces of three scenes in both modes, on synthetic frames at every size where the pass
takes another path, under permuted rows and other numbers of children, the fates, end to end against the C oracle's trace
of the reference's children, and the closed forms of the Lambertian plate under the 5-standard-error rule."""
import numpy as np
import pytest

import fresnel_reference as fref
import ghost_scenes as gs
import helpers
import scatter_reference as ref
import scatter_scenes as ss

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = fref.IX
# csrc: kFresnelBlock = PRT_BLOCK = 256 (four waves of 64), kWfRowsPerWave = 1024 and kWfMaxWaves = 2048 (sort_plan, over
# items), kSortScanBlock = 512 (the scans' threads), kGhostCountBytes = 64 MiB of (wave, bucket) counts of 8 bytes
WAVE, BLOCK, ROWS_PER_WAVE, MAX_WAVES, SCAN, COUNT_BYTES = 64, 256, 1024, 2048, 512, 64 << 20


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else [0]
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def agree(got, want, what):
    """Rays, parent_row, child, keys, counts, stride and counters: the reference's, bit for bit."""
    assert tuple(getattr(got, name) for name in ref.COUNTERS) == tuple(want[name] for name in ref.COUNTERS), what
    assert got.counts.tolist() == want["counts"].tolist(), what
    assert (got.stride, got.n_groups) == (want["stride"], want["n_groups"]), what
    assert got.keys.tolist() == want["keys"].tolist() and got.bucket.tolist() == want["bucket"].tolist(), what
    assert np.array_equal(got.parent_row.cpu().numpy(), want["parent_row"]), what
    assert np.array_equal(got.child.cpu().numpy(), want["child"]) and got.child.dtype == torch.int32, what
    helpers.assert_same_bits(got.rays.cpu().numpy(), want["rays"], what)


def both(device, parts, ids, numbers, toward=None, **options):
    """(device result, reference on the downloaded frame)."""
    models, table_values = ss.tables()
    given, order, order_numbers = ss.product_models(list(ids), list(numbers), models)
    got = device.scatter(given, parts, toward=None if toward is None else toward[0], **options)
    reference = dict(options)
    reference["rays_per_group"] = reference.pop("rays_per_source", None)
    want = ss.reference(device.rows.cpu().numpy().T, parts, order, order_numbers, table_values,
                        target=None if toward is None else toward[1], **reference)
    assert list(got.surfaces) == order
    return got, want


# ---- GPU traces of three scenes ---------------------------------------------------------------------------------------------
def traced(parts, rays, limit=10):
    from pyrayt_amd.engine import DeviceScene
    from pyrayt_amd.frame import DeviceFrame
    from pyrayt_amd.scene import SceneSnapshot

    scene = DeviceScene(SceneSnapshot(parts))
    rows, counts = scene.trace(torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0"), limit)
    return DeviceFrame(rows, counts)


SCENES = {"stopped_lens": (lambda: ss.stopped_lens(300), ((-3.0, 0.5, 0.0), (1.0, 0.0, 0.0), 1.0)),
          "prism": (lambda: ss.prism(40), ((3.0, 0.0, 0.0), (-1.0, 0.2, 0.0), 1.0)),
          "two_mirrors": (lambda: ss.two_mirrors(48), ((0.0, 2.0, 0.5), (0.0, 1.0, 0.0), 0.8))}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_children_of_a_traced_frame_are_the_references(name):
    build, disk = SCENES[name]
    parts, rays, _ = build()
    device = traced(parts, rays)
    frame = device.rows.cpu().numpy().T
    ids, numbers = ss.split_models(frame, parts)
    assert len(ids) >= 2 and set(numbers) == {0, 1}
    per_group = rays.shape[1] // (4 if name == "prism" else 3)
    groups = dict(rays_per_source=per_group, n_groups=-(-rays.shape[1] // per_group))
    for toward in (None, ss.target_for(*disk)):
        mode = "hemisphere" if toward is None else "disk"
        got, want = both(device, parts, ids, numbers, toward, rays_per_hit=3, seed=7, **groups)
        agree(got, want, f"{name}, {mode}")
        assert got.n_spawned > 100 and got.n_rejected > 50 and got.n_groups >= 2
        assert got.n_invalid == 0 and (toward is not None or got.n_below == 0)
        weak = float(got.rays[9].median())
        other, wanted = both(device, parts, ids[::-1], numbers[::-1], toward, rays_per_hit=3, seed=2 ** 63 + 5,
                             min_intensity=weak, ray_offset=1e-3, **groups)
        agree(other, wanted, f"{name}, {mode}, threshold and second seed")
        assert other.n_dropped > 0 and not np.array_equal(other.counts, got.counts)
        again = repeated(device, got, parts, **groups)
        assert torch.equal(again.rays.view(torch.int64), got.rays.view(torch.int64))
        assert torch.equal(again.parent_row, got.parent_row) and torch.equal(again.child, got.child)
    if name == "prism":
        assert len(set(got.rays[10].cpu().tolist())) == 4
    if name == "two_mirrors":
        assert len(set(device["generation"][got.parent_row].cpu().tolist())) == 10  # (a row of every generation spawns)


def repeated(device, result, parts, **groups):
    """The call that gave `result`, once more (default threshold and offset)."""
    return device.scatter(dict(zip(result.surfaces, result.models)), parts, toward=result.toward,
                          rays_per_hit=result.rays_per_hit, seed=result.seed, **groups)


# ---- synthetic frames at the partition edges ---------------------------------------------------------------------------------
def walls():
    """A tilted plane, a sphere and a cylinder (absorbers): (parts, ids)."""
    a = gs.api()
    black = a.materials.absorber
    parts = [a.cg.XYPlane(3, 3, material=black).rotate_y(40).move(0.3, -0.2, 1.0), a.cg.Sphere(1.5, material=black).move_x(2),
             a.cg.Cylinder(0.7, -1, 1, material=black).rotate_x(30)]
    return parts, [int(part.get_id()) for part in parts]


def landings(n_rows, ids, unlisted=4, seed=11, generations=3):
    """A frame of exactly n_rows rows that land on the surfaces `ids` in turn, every `unlisted`-th row (0: none) on
    surface 9999, which no call lists; random landing points, directions and intensities, ids 0 .. n_rows - 1."""
    rng = np.random.default_rng(seed + n_rows)
    frame = np.zeros((n_rows, 15))
    frame[:, IX["generation"]] = np.sort(rng.integers(0, generations, n_rows))
    frame[:, IX["id"]] = np.arange(n_rows)
    frame[:, IX["intensity"]] = rng.uniform(50.0, 100.0, n_rows)
    frame[:, IX["wavelength"]], frame[:, IX["index"]] = rng.choice([0.45, 0.633], n_rows), rng.choice([1.0, 1.5], n_rows)
    frame[:, IX["surface"]] = np.asarray(ids, dtype=float)[np.arange(n_rows) % len(ids)]
    if unlisted:
        frame[unlisted - 1::unlisted, IX["surface"]] = 9999
    frame[:, 9:12], frame[:, 12:15] = rng.normal(size=(n_rows, 3)), rng.normal(size=(n_rows, 3))
    return frame


def grouping(n_rows, groups):
    return dict(rays_per_source=max(1, -(-n_rows // groups)), n_groups=groups) if groups > 1 else {}


DISK = ((0.5, 0.3, 4.0), (0.1, -0.2, -1.0), 1.2)
# (rows, children a hit): items on either side of a wave, of a workgroup, of a wave's run of the sort, of the scan's 512
# runs, and of the most waves the sort plans
ITEM_COUNTS = [(1, 1), (63, 1), (64, 1), (65, 1), (9, 7), (1, 64), (13, 5), (255, 1), (256, 1), (257, 1), (17, 15), (4, 64),
               (ROWS_PER_WAVE - 1, 1), (ROWS_PER_WAVE, 1), (ROWS_PER_WAVE + 1, 1), (16, 64), (205, 5), (4 * ROWS_PER_WAVE + 1, 1)]
BIG_ITEM_COUNTS = [(SCAN * ROWS_PER_WAVE - 1, 1), (8192, 64), (174763, 3), (MAX_WAVES * ROWS_PER_WAVE // 64, 64), (MAX_WAVES * ROWS_PER_WAVE // 64 + 1, 64)]
assert [r * n for r, n in BIG_ITEM_COUNTS[:3]] == [SCAN * ROWS_PER_WAVE - 1, SCAN * ROWS_PER_WAVE, SCAN * ROWS_PER_WAVE + 1]
assert BIG_ITEM_COUNTS[-1] == (32769, 64)


@pytest.mark.parametrize("n_rows, rays_per_hit", ITEM_COUNTS + BIG_ITEM_COUNTS)
def test_item_counts_on_either_side_of_the_blocks_and_of_the_sort_plan(n_rows, rays_per_hit):
    parts, ids = walls()
    frame = landings(n_rows, ids, unlisted=0 if n_rows < 4 else 4)
    device = device_frame(frame)
    toward = ss.target_for(*DISK) if n_rows % 2 else None
    got, want = both(device, parts, ids, [0, 1, 1], toward, rays_per_hit=rays_per_hit, seed=n_rows, **grouping(n_rows, 3))
    agree(got, want, f"{n_rows} rows x {rays_per_hit}")
    listed = int((frame[:, IX["surface"]] != 9999).sum())
    assert sum(getattr(got, name) for name in ref.COUNTERS) == listed * rays_per_hit
    if n_rows * rays_per_hit > 100:
        assert 0.6 * listed * rays_per_hit < got.n_spawned + got.n_below < 0.95 * listed * rays_per_hit


@pytest.mark.parametrize("buckets", [1, SCAN - 1, SCAN, SCAN + 1])
def test_bucket_counts_on_either_side_of_the_scans_threads(buckets):
    parts, ids = walls()
    frame = landings(3000, ids[:1], unlisted=3)
    got, want = both(device_frame(frame), parts, ids[:1], [1], None, rays_per_hit=2, seed=1, **grouping(3000, buckets))
    agree(got, want, f"{buckets} buckets")
    assert got.n_groups >= min(buckets, 400)


def test_more_buckets_than_the_counts_cap_gives_every_wave():
    """65535 buckets of 8 bytes: 64 MiB hold 128 waves' counts, and 131073 items would have 129 waves."""
    parts, ids = walls()
    n_groups = 65535 // 3
    waves = COUNT_BYTES // (3 * n_groups * 8)
    assert waves == 128 and 3 * n_groups == 65535
    n_rows = waves * ROWS_PER_WAVE + 1
    frame = landings(n_rows, ids, unlisted=0)
    got, want = both(device_frame(frame), parts, ids, [0, 1, 0], ss.target_for(*DISK), rays_per_hit=1, seed=3,
                     **grouping(n_rows, n_groups))
    agree(got, want, "the counts' cap")
    assert got.n_groups > 30000


def test_no_listed_row_an_empty_frame_and_the_last_bucket():
    from pyrayt_amd.frame import DeviceFrame

    parts, ids = walls()
    models, _ = ss.tables()
    frame = landings(700, [9999], unlisted=0)
    got, want = both(device_frame(frame), parts, ids, [0, 1, 1], None, rays_per_hit=4)
    agree(got, want, "no listed row")
    assert len(got) == 0 and got.n_groups == 0 and got.stride == 0 and got.keys.shape == (0, 2)
    assert all(getattr(got, name) == 0 for name in ref.COUNTERS) and len(got.trace(_scene(parts), generation_limit=5)) == 0
    empty = DeviceFrame(torch.zeros((15, 0), dtype=torch.float64, device="cuda:0"), [0])
    none = empty.scatter({ids[0]: models[0]}, parts, rays_per_hit=64)
    assert len(none) == 0 and none.rays.shape == (13, 0) and none.child.shape == (0,) and none.n_rejected == 0
    last = landings(1500, ids[1:2], unlisted=0)
    last[:, IX["id"]] += 4000  # (every ray in the last of five groups of 1100)
    got, want = both(device_frame(last), parts, [ids[2], ids[1]], [0, 1], None, rays_per_hit=2, rays_per_source=1100, n_groups=5)
    agree(got, want, "the last bucket")
    assert got.bucket.tolist() == [7, 9] or got.bucket.tolist() == [9]


def _scene(parts):
    from pyrayt_amd.engine import DeviceScene
    from pyrayt_amd.scene import SceneSnapshot

    return DeviceScene(SceneSnapshot(parts))


# ---- invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["hemisphere", "disk"])
def test_rows_permuted_give_the_same_set_of_children(mode):
    parts, ids = walls()
    frame = landings(3001, ids, seed=4)
    rng = np.random.default_rng(3)
    counts = np.bincount(frame[:, 0].astype(int))
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = np.concatenate([starts[g] + rng.permutation(counts[g]) for g in range(len(counts))])  # new row -> old row
    toward = ss.target_for(*DISK) if mode == "disk" else None
    options = dict(rays_per_hit=4, seed=21, rays_per_source=1001, n_groups=3)
    a, wanted = both(device_frame(frame), parts, ids, [0, 1, 1], toward, **options)
    agree(a, wanted, "in frame order")
    b, want = both(device_frame(frame[order]), parts, ids, [0, 1, 1], toward, **options)
    agree(b, want, "shuffled")

    def children(result, rows):
        """The children sorted by (parent ray id, generation, child), their ids apart."""
        payload = result.rays.cpu().numpy()
        parents = rows[result.parent_row.cpu().numpy()]
        keys = np.stack([parents[:, IX["id"]], parents[:, IX["generation"]], result.child.cpu().numpy().astype(float)])
        lines = np.concatenate([keys, payload[:12]]).T
        return lines[np.lexsort(keys[::-1])]

    lines_a, lines_b = children(a, frame), children(b, frame[order])
    # (2251 listed rows x 4 children, pi / 4 of them inside the unit disk: about 7000 over the hemisphere; the target disk
    # stands in front of about half of the random normals, and the rest are below the horizon)
    assert np.array_equal(lines_a.view(np.int64), lines_b.view(np.int64)) and len(lines_a) == a.n_spawned > 2000
    assert a.counts.tolist() == b.counts.tolist() and not torch.equal(a.parent_row, b.parent_row)


@pytest.mark.parametrize("mode", ["hemisphere", "disk"])
def test_a_childs_direction_does_not_depend_on_the_number_of_children(mode):
    parts, ids = walls()
    frame = landings(2000, ids, seed=5)
    device = device_frame(frame)
    toward = ss.target_for(*DISK) if mode == "disk" else None
    one, want = both(device, parts, ids, [0, 1, 1], toward, rays_per_hit=1, seed=8)
    agree(one, want, "one child")
    four, want = both(device, parts, ids, [0, 1, 1], toward, rays_per_hit=4, seed=8)
    agree(four, want, "four children")
    first = (four.child == 0).cpu().numpy()
    # (the same surfaces are listed in both calls and there is one group: child 0 of every row in the same order)
    assert np.array_equal(four.parent_row.cpu().numpy()[first], one.parent_row.cpu().numpy())
    assert first.sum() > 400  # (1500 listed rows, pi / 4 of the samples accepted; the disk is seen by about half of them)
    rays_one, rays_four = one.rays.cpu().numpy(), four.rays.cpu().numpy()[:, first]
    assert np.array_equal(rays_four[:9].view(np.int64), rays_one[:9].view(np.int64))
    assert np.array_equal((4.0 * rays_four[9]).view(np.int64), rays_one[9].view(np.int64))
    again = repeated(device, four, parts)
    assert torch.equal(again.rays.view(torch.int64), four.rays.view(torch.int64)) and torch.equal(again.child, four.child)


# ---- fates ---------------------------------------------------------------------------------------------------------------------
def test_fates_on_the_device():
    from pyrayt_amd.scatter import Scatter, Target

    a = gs.api()
    black = a.materials.absorber
    plane = a.cg.XYPlane(3, 3, material=black)  # z = 0, normal +z
    box = a.cg.Cuboid((-1, -1, -1), (1, 1, 1), material=black)
    parts = [plane, box]
    sid, cube = int(plane.get_id()), ss.surface_ids(box)[0]
    table = ref.table_of(ss.prims_of(parts))
    frame = landings(900, [sid], unlisted=0)
    frame[:, 9:12] *= (1, 1, 0)
    frame[:, 14] = -np.abs(frame[:, 14])  # (the rays come from above)
    device = device_frame(frame)
    wall = Scatter.lambertian(0.3)
    accepted = device.scatter({plane: wall}, parts, rays_per_hit=2).n_spawned
    behind = device.scatter({plane: wall}, parts, toward=Target.disk((0, 0, -5), (0, 0, 1), 0.5), rays_per_hit=2)
    assert behind.n_below == accepted > 1000 and behind.n_spawned == 0 and behind.n_rejected == 1800 - accepted
    dark = device.scatter({plane: Scatter.lambertian(0.0)}, parts, rays_per_hit=2)
    assert dark.n_dark == accepted and dark.n_spawned == 0 and len(dark) == 0
    inside = frame.copy()
    inside[:, IX["surface"]], inside[:, 9:12] = cube, inside[:, 9:12] * 0.1  # (points on no face of the cube)
    for toward in (None, Target.disk((0, 0, 5), (0, 0, 1), 0.5)):
        edge = device_frame(inside).scatter({cube: wall}, parts, toward=toward, rays_per_hit=2)
        want = ref.scatter(inside, table, [cube], [0], wall.table[None], target=None if toward is None else toward.packed(),
                           rays_per_hit=2)
        assert edge.n_invalid == want["n_invalid"] == accepted and edge.n_spawned == 0
    still = frame.copy()
    still[:10, 12:15] = 0.0  # (rows without a direction)
    assert device_frame(still).scatter({plane: wall}, parts, rays_per_hit=2).n_invalid == \
        ref.scatter(still, table, [sid], [0], wall.table[None], rays_per_hit=2)["n_invalid"] > 0
    with pytest.raises(ValueError, match="not below n_groups"):
        device.scatter({plane: wall}, parts, rays_per_source=10, n_groups=3)
    bad = frame.copy()
    bad[5, IX["id"]] = 2.5
    with pytest.raises(ValueError, match="not an integer"):
        device_frame(bad).scatter({plane: wall}, parts)
    after = device.scatter({plane: wall}, parts, rays_per_hit=2)
    agree(after, ref.scatter(frame, table, [sid], [0], wall.table[None], rays_per_hit=2), "after the refusals")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def lens_tracer(n):
    """A singlet and its detector in a barrel, a closed black cylinder, lit 20 degrees off the axis: the beam goes
    through the lens and ends on the barrel's wall next to the detector (examples/stray_light.py)."""
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=3).rotate_z(20).move(-0.9, -0.33, 0)
    det = pyrayt.components.baffle((1, 1)).move_x(2)
    barrel = pyrayt.g3d.Cylinder(0.6, -3.0, 3.0, material=pyrayt.materials.absorber).rotate_y(90)
    parts = [lens, det, barrel]
    return pyrayt.RayTracer(src, parts, rays_per_source=n), lens, det, barrel, parts


def test_trace_scatter_end_to_end_against_the_oracle():
    from oracle import c_oracle
    from pyrayt_amd.scatter import Scatter, Target

    tracer, lens, det, barrel, parts = lens_tracer(500)
    polish, paint = Scatter.harvey(*ss.HARVEY), Scatter.lambertian(ss.LAMBERT)
    models = {lens: polish, barrel: paint}
    plain = tracer.trace().to_numpy(dtype=float)
    kept, settings = tracer.device_frame, tracer.record_only(det)._record_surfaces
    toward = Target.disk((2.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.5 * np.sqrt(2))  # (the detector's circumscribed circle)
    analysis = tracer.trace_scatter(det, models, toward=toward, rays_per_hit=2, seed=5)
    assert tracer.device_frame is kept and tracer._record_surfaces == settings
    rays = analysis.rays
    frame = analysis.frame.rows.cpu().numpy().T
    helpers.assert_frames_identical(frame, plain, "the signal's frame")
    wall = int(barrel.get_id())
    assert int((plain[:, IX["surface"]] == wall).sum()) == 500 and not (plain[:, IX["surface"]] == det.get_id()).any()
    listed = ss.surface_ids(lens) + [wall]
    assert list(rays.surfaces) == listed and rays.rays_per_hit == 2 and rays.seed == 5 and rays.toward is toward
    tables = np.stack([polish.table, paint.table])
    numbers = [0] * len(ss.surface_ids(lens)) + [1]
    want = ss.reference(frame, parts, listed, numbers, tables, target=toward.packed(), rays_per_hit=2, seed=5,
                        rays_per_group=500, n_groups=1)
    agree(rays, want, "the children")
    # (the lens faces see the detector from behind: their children are below the horizon, the wall's are not)
    assert rays.n_spawned > 500 and rays.n_below > 1000 and rays.keys.tolist() == [[0, wall]]
    traced_by_oracle, _ = c_oracle.trace(gs.flat(parts), want["rays"], 10)
    helpers.assert_frames_identical(analysis.scattered.rows.cpu().numpy().T, traced_by_oracle, "the children's frame")
    table = analysis.table()
    on = traced_by_oracle[:, IX["surface"]] == det.get_id()
    energy = float(np.sum(traced_by_oracle[on, IX["intensity"]].astype(np.longdouble)))
    print(f"the wall: {table.loc[0, 'energy']!r} against {energy!r}, {int(on.sum())} rays on the detector")
    assert len(table) == 1 and table.loc[0, "surface"] == wall and table.loc[0, "source"] == 0
    assert table.loc[0, "rays"] == int(on.sum()) > 300
    assert np.isclose(table.loc[0, "energy"], energy, rtol=1e-12, atol=1e-12)  # (test_gpu_frame.py's bar)
    assert analysis.signal_energy() == 0.0 and np.isnan(table.loc[0, "share"])  # (the source is out of the field)
    launched = float(plain[:500, IX["intensity"]].sum())
    assert 0.002 < energy / launched < 0.03  # (0.04 of the beam scattered, a fifth of the hemisphere is detector)
    image, y_edges, z_edges = analysis.image(bins=8, range=((-0.5, 0.5), (-0.5, 0.5)))
    assert image.shape == (8, 8) and np.isclose(image.sum(), energy, rtol=1e-12)
    # the hemisphere mode and Fresnel losses first: the reference on the applied frame
    lossy = tracer.trace_scatter(det, models, rays_per_hit=1, seed=6, fresnel={}, min_share=1e-9)
    applied = lossy.frame.rows.cpu().numpy().T
    assert np.all(applied[:, IX["intensity"]] <= plain[:, IX["intensity"]]) and not np.array_equal(applied, plain)
    want = ss.reference(applied, parts, listed, numbers, tables, rays_per_hit=1, seed=6, rays_per_group=500, n_groups=1,
                        min_intensity=1e-9 * float(plain[:500, IX["intensity"]].max()))
    agree(lossy.rays, want, "the children of the applied frame")
    assert lossy.rays.toward is None and lossy.rays.n_below == 0 and lossy.rays.n_groups == 3
    tracer.record_only()
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), plain, equal_nan=True)


def test_trace_scatter_refuses_what_it_cannot_follow():
    import scenes
    from pyrayt_amd.scatter import Scatter

    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    parts, _ = scenes.custom_retro(scenes.product_api())
    tracer = pyrayt.RayTracer(pyrayt.components.LineOfRays(), parts, rays_per_source=8)
    with pytest.raises(TypeError, match=r"user-defined trace\(\)"):
        tracer.trace_scatter(parts[0], {parts[0]: Scatter.lambertian(0.1)})
    tracer, lens, det, barrel, parts = lens_tracer(16)
    with pytest.raises(ValueError, match="min_share"):
        tracer.trace_scatter(det, {lens: Scatter.lambertian(0.1)}, min_share=-1)
    with pytest.raises(ValueError, match="toward is None"):
        tracer.trace_scatter(det, {lens: Scatter.lambertian(0.1)}, toward=det)  # (an imager is not a target)


# ---- closed forms on the device ----------------------------------------------------------------------------------------------
def _plate(rows, direction):
    a = gs.api()
    plane = a.cg.XYPlane(3, 3, material=a.materials.absorber)
    frame = np.zeros((rows, 15))
    frame[:, IX["id"]] = np.arange(rows)
    frame[:, IX["intensity"]], frame[:, IX["wavelength"]], frame[:, IX["index"]] = 1.0, 0.55, 1.0
    frame[:, IX["surface"]], frame[:, 12:15] = plane.get_id(), direction
    return plane, frame


@pytest.mark.parametrize("rows, rays_per_hit, seed", [(4096, 4, 0), (1500, 16, 1), (20000, 1, 2 ** 63 + 11)])
def test_the_lambertian_plate_and_the_coaxial_disk_on_the_device(rows, rays_per_hit, seed):
    """The sum of the children's energies per unit of incoming energy: rho over the hemisphere, rho R^2 / (R^2 + d^2)
    into a coaxial disk; each within 5 standard errors, the error from the children's own energies."""
    from pyrayt_amd.scatter import Scatter, Target

    plane, frame = _plate(rows, (0.0, 0.0, -1.0))
    device = device_frame(frame)
    wall = Scatter.lambertian(0.3)
    table = ref.table_of(ss.prims_of([plane]))
    got = device.scatter({plane: wall}, [plane], rays_per_hit=rays_per_hit, seed=seed)
    agree(got, ref.scatter(frame, table, [plane.get_id()], [0], wall.table[None], rays_per_hit=rays_per_hit, seed=seed), "plate")
    total, sigma = ref.estimate(got.rays[9].cpu().numpy(), rows, rays_per_hit)
    print(f"hemisphere {rows} x {rays_per_hit}, seed {seed}: {total:.6f} +- {sigma:.6f}: {(total - 0.3) / sigma:+.2f} standard errors")
    assert abs(total - 0.3) <= 5 * sigma and sigma < 0.01
    radius, distance = 0.5, 1.0
    disk = Target.disk((0, 0, distance), (0, 0, 1), radius)
    got = device.scatter({plane: wall}, [plane], toward=disk, rays_per_hit=rays_per_hit, seed=seed)
    agree(got, ref.scatter(frame, table, [plane.get_id()], [0], wall.table[None], target=disk.packed(), rays_per_hit=rays_per_hit,
                           seed=seed), "disk")
    total, sigma = ref.estimate(got.rays[9].cpu().numpy(), rows, rays_per_hit)
    exact = 0.3 * radius ** 2 / (radius ** 2 + distance ** 2)
    print(f"disk {rows} x {rays_per_hit}, seed {seed}: {total:.6f} +- {sigma:.6f}: {(total - exact) / sigma:+.2f} standard errors")
    assert abs(total - exact) <= 5 * sigma and sigma < 0.002
