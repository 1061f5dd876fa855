"""Ray-path analysis of the result frame on the device (DeviceFrame.paths, RayTracer.trace_paths): against the numpy /
dict restatement of the definitions (tests/paths_reference.py) on the reference's own frames (tests/golden/scene_*.npz)
and on synthetic frames built by hand, exactly: the counts, the numbering and the per-row and per-ray nodes are
integers, and the energies are integer sums scaled by a power of two."""
import numpy as np
import pytest

import helpers
import paths_reference as ref
from paths_partitions import check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX
FIXTURES = ["config1", "config2", "config3", "config4", "config5", "mirrors_and_stops", "adv_prism", "adv_lens",
            "two_mirrors", "tutorial", "stopped_lens", "stale_box", "adv_short_b"]
_CACHE = {}


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def synthetic_frame():
    """20 000 ids from 1000 in three groups of 7000, six generations, surfaces drawn from {0, 1, 2} and a death
    probability per generation: up to 3 + 9 + ... + 729 = 1092 nodes, every wave of 64 consecutive ids holding all three
    keys of several parents; weights that are no integers, and a few that do not count."""
    if "synthetic" not in _CACHE:
        rng = np.random.default_rng(11)
        n = 20_000
        alive = np.arange(n)
        blocks = []
        for generation in range(6):
            block = np.zeros((len(alive), 15))
            block[:, IX["generation"]] = generation
            block[:, IX["id"]] = 1000 + alive
            block[:, IX["surface"]] = rng.integers(0, 3, len(alive))
            block[:, IX["intensity"]] = 100 * rng.random(len(alive)) * 0.8 ** generation
            block[:, 12:15] = rng.normal(size=(len(alive), 3))
            block[rng.random(len(alive)) < 0.1, 12:15] = [0.0, 0.0, 1e-9]  # (absorbed, where it is the ray's last row)
            blocks.append(block)
            alive = alive[rng.random(len(alive)) > 0.15 + 0.05 * generation]
        frame = np.concatenate(blocks)
        frame[[5, 77, 30_000, 50_001], IX["intensity"]] = [np.nan, -1.0, np.inf, -np.inf]
        _CACHE["synthetic"] = (frame, ref.paths(frame, rays_per_source=7000, n_groups=3))
    return _CACHE["synthetic"]


@pytest.mark.parametrize("name", FIXTURES)
def test_paths_of_the_reference_frames(name):
    frame = helpers.load(f"scene_{name}.npz")["frame"]
    want = ref.paths(frame)
    got = device_frame(frame).paths()
    check(got, want)
    assert got.n_groups == 1 and got.ended.sum() == want["n_rays"]
    # per source: groups of 512 ids, and one group too few (its rows keep their nodes and leave the tables)
    n_groups = int(frame[:, IX["id"]].max() // 512) + 1
    check(device_frame(frame).paths(rays_per_source=512), ref.paths(frame, rays_per_source=512, n_groups=n_groups))
    if n_groups > 1:
        check(device_frame(frame).paths(rays_per_source=512, n_groups=n_groups - 1),
              ref.paths(frame, rays_per_source=512, n_groups=n_groups - 1))
    check(device_frame(frame).paths(weights=None), ref.paths(frame, weights=None))


def test_paths_of_a_synthetic_frame():
    frame, want = synthetic_frame()
    assert len(want["sequences"]) > 900 and want["n_bad_weight"] == 4 and want["dark"].sum() > 100
    assert not want["integer_weights"]
    got = device_frame(frame).paths(rays_per_source=7000, n_groups=3)
    check(got, want)
    check(device_frame(frame).paths(rays_per_source=7000, n_groups=2), ref.paths(frame, rays_per_source=7000, n_groups=2))
    # integer weights: the energies are the exact sums
    whole = frame.copy()
    whole[:, IX["intensity"]] = np.floor(np.nan_to_num(whole[:, IX["intensity"]], nan=0.0, posinf=0.0, neginf=0.0) + 1)
    want = ref.paths(whole, rays_per_source=7000, n_groups=3)
    assert want["integer_weights"]
    check(device_frame(whole).paths(rays_per_source=7000, n_groups=3), want)


def test_sixty_four_distinct_first_surfaces_in_one_wave():
    frame = np.zeros((64 + 40, 15))
    frame[:, 12] = 1.0
    frame[:, IX["intensity"]] = 100.0
    frame[:64, IX["id"]] = np.arange(64)
    frame[:64, IX["surface"]] = np.arange(64)[::-1] * 1000  # (descending: the canonical order is not the order made)
    frame[64:, IX["generation"]] = 1
    frame[64:, IX["id"]] = np.arange(40)
    frame[64:, IX["surface"]] = 2 ** 31 - 1 - (np.arange(40) % 2)
    want = ref.paths(frame)
    assert len(want["sequences"]) == 104 and want["surface"].max() == 2 ** 31 - 1
    check(device_frame(frame).paths(), want)
    check(device_frame(frame).paths(max_paths=104), want)


def test_many_waves_insert_one_key_at_once():
    n = 200_000
    frame = np.zeros((n, 15))
    frame[:, IX["id"]] = np.arange(n)
    frame[:, IX["surface"]] = 0  # (surface 0 under no parent: the key an all-zero word would stand for)
    frame[:, IX["intensity"]] = 100.0
    frame[:, 13] = 1.0
    got = device_frame(frame).paths()
    assert got.sequences == [(0,)] and got.n_nodes == 1
    assert got.through.tolist() == [[n]] and got.ended.tolist() == [[n]] and got.dark.tolist() == [[0]]
    assert got.energy_through.tolist() == [[100.0 * n]] and got.energy_ended.tolist() == [[100.0 * n]]
    assert int(got.row_node.abs().sum()) == 0 and int(got.ray_node.abs().sum()) == 0
    assert torch.equal(got.ray_last_row, torch.arange(n, device="cuda:0"))


def test_too_many_nodes_are_refused_and_nothing_is_left_behind():
    frame = helpers.load("scene_stale_box.npz")["frame"]
    want = ref.paths(frame)
    nodes = len(want["sequences"])
    device = device_frame(frame)
    with pytest.raises(ValueError, match="max_paths = 8 "):
        device.paths(max_paths=8)
    check(device.paths(max_paths=4096), want)
    check(device.paths(max_paths=nodes), want)
    with pytest.raises(ValueError, match=f"max_paths = {nodes - 1} "):
        device.paths(max_paths=nodes - 1)
    check(device.paths(), want)


def test_frames_the_definitions_refuse():
    frame = helpers.load("scene_stopped_lens.npz")["frame"]
    device = device_frame(frame)
    with pytest.raises(ValueError, match="where"):
        device.where(surface=6).paths()
    cut = device_frame(frame[frame[:, IX["surface"]] == 6])
    cut.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        cut.paths()
    for column, value, message in (("id", frame[6, IX["id"]], "repeats within a generation"),
                                   ("id", frame[5, IX["id"]] + 0.5, "id is not an integer"),
                                   ("surface", 1.5, "surface is not an integer"),
                                   ("surface", -1.0, "surface is not an integer"),
                                   ("surface", 2.0 ** 31, "surface is not an integer")):
        bad = frame.copy()
        bad[5, IX[column]] = value
        with pytest.raises(ValueError, match=message):
            device_frame(bad).paths()
    late = np.flatnonzero(frame[:, 0] == 2)[0]
    gone = np.flatnonzero((frame[:, 0] == 1) & (frame[:, IX["id"]] == frame[late, IX["id"]]))[0]
    with pytest.raises(ValueError, match="not whole"):
        device_frame(np.delete(frame, gone, axis=0)).paths()
    check(device.paths(), ref.paths(frame))  # (the refusals left nothing behind)


def outputs(paths):
    return [torch.from_numpy(np.ascontiguousarray(getattr(paths, name))) for name in
            ("parent", "surface", "depth", "subtree_size", "through", "ended", "dark", "energy_through",
             "energy_ended")] + [paths.row_node, paths.ray_node, paths.ray_last_row]


def test_the_same_bits_on_every_run_and_in_any_order_of_the_rows():
    frame, want = synthetic_frame()
    options = dict(rays_per_source=7000, n_groups=3)
    first, second = device_frame(frame).paths(**options), device_frame(frame).paths(**options)
    for a, b in zip(outputs(first), outputs(second)):
        assert torch.equal(a.cpu(), b.cpu())
    rng = np.random.default_rng(3)
    counts = np.bincount(frame[:, 0].astype(int))
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = np.concatenate([starts[g] + rng.permutation(counts[g]) for g in range(len(counts))])  # new row -> old row
    shuffled = device_frame(frame[order]).paths(**options)
    for a, b in zip(outputs(first)[:9], outputs(shuffled)[:9]):
        assert torch.equal(a, b)
    assert shuffled.sequences == first.sequences
    assert torch.equal(shuffled.ray_node, first.ray_node)
    where = torch.from_numpy(order).to("cuda:0")
    assert torch.equal(shuffled.row_node, first.row_node[where])
    assert torch.equal(where[shuffled.ray_last_row], first.ray_last_row)


def stopped_lens_tracer(n):
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    c = pyrayt.components
    stop = c.aperture((3.0, 3.0), 0.5).move_x(-0.5)
    lens = c.plano_convex_lens(1.5, 0.3, aperture=1.2)
    det = c.baffle((4, 4)).move_x(2.5)
    # (two fans in the xy plane from one point: the wide one is clipped by the stop, the narrow one passes whole)
    sources = [c.WedgeOfRays(30).move_x(-3), c.WedgeOfRays(10).move_x(-3)]
    return pyrayt.RayTracer(sources, [stop, lens, det], rays_per_source=n), stop, lens, det


def test_one_million_rays_give_the_same_bits_twice():
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-2)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    frame = pyrayt.RayTracer(src, [lens, det], rays_per_source=1_000_000).trace_device()
    first, second = frame.paths(), frame.paths()
    assert first.n_nodes == 3 and first.through.tolist() == [[1_000_000] * 3] and first.ended.tolist() == [[0, 0, 1_000_000]]
    assert first.energy_through.tolist() == [[1e8] * 3]
    for a, b in zip(outputs(first), outputs(second)):
        assert torch.equal(a.cpu(), b.cpu())
    assert torch.equal(first.row_node, torch.arange(3, device="cuda:0", dtype=torch.int32).repeat_interleave(1_000_000))


def test_a_path_cuts_the_frame_for_the_other_passes():
    frame = helpers.load("scene_stopped_lens.npz")["frame"]
    device = device_frame(frame)
    paths = device.paths()
    through = paths.index((3, 4, 6))
    import pandas as pd

    table = pd.DataFrame(frame, columns=ref.COLUMNS)
    sequence = table.groupby("id")["surface"].agg(tuple)
    ids = sequence.index[sequence == (3.0, 4.0, 6.0)]
    mask = np.isin(frame[:, IX["id"]], ids)
    assert mask.sum() == 3 * 447
    cut = device.select(paths.rows(through))
    assert np.array_equal(cut.to_numpy(), frame[mask])
    assert np.array_equal(paths.rays(through).cpu().numpy(), np.isin(np.arange(2048) + paths.id0, ids))
    by_host = device.select(torch.from_numpy(mask).to("cuda:0"))
    assert cut.group_stats(surface=6).equals(by_host.group_stats(surface=6))
    # the stopped rays: the prefix (0,) is also complete; every ray under (3,) reached the detector
    assert int(paths.rays(paths.index((3,)), complete=False).sum()) == 447 and int(paths.rays(paths.index((3,))).sum()) == 0
    assert int(paths.rows(paths.index((0,))).sum()) == 1601


def test_trace_paths_and_the_tracer_is_left_as_it_was():
    tracer, stop, lens, det = stopped_lens_tracer(4096)
    plain = tracer.trace().to_numpy(dtype=float)
    kept = tracer.device_frame
    want = tracer.trace_device().paths(rays_per_source=4096, n_groups=2)
    held = tracer._device_frame
    got = tracer.trace_paths()
    assert tracer._device_frame is held and kept is not None
    for a, b in zip(outputs(got), outputs(want)):
        assert torch.equal(a.cpu(), b.cpu())
    assert got.sequences == want.sequences and got.launched == 4096 and got.n_nodes >= 4
    check(got, ref.paths(plain, rays_per_source=4096, n_groups=2))
    at_stop = np.isin(got.surface, [sid for sid, _ in stop.surface_ids])
    assert got.ended[0, at_stop].sum() > 100 and got.ended[1, at_stop].sum() == 0
    fates = got.fates()
    assert fates["ended"].sum() == 2 * 4096
    assert fates.loc[fates["surface"] == -1, "ended"].tolist() == [4096 - int(n) for n in got.through[:, got.depth == 0].sum(1)]
    assert len(got.find(through=[s for s, _ in lens.surface_ids][:1], ends_at=det)) >= 1
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), plain, equal_nan=True)
    tracer.record_only(det, columns=("y1", "z1"))
    spot = tracer.trace().to_numpy(dtype=float)
    again = tracer.trace_paths()
    assert tracer._record_surfaces == (det.get_id(),) and tracer._record_columns == ("y1", "z1")
    assert again.sequences == got.sequences and np.array_equal(again.through, got.through)
    assert np.array_equal(tracer.get_results().to_numpy(dtype=float), spot)
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), spot)
    with pytest.raises(ValueError, match="record_only"):
        tracer.trace_device().paths()
