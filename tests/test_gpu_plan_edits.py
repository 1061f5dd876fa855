"""Record plans across scene edits: the design loop they exist for -- edit the system, trace under the plan, read one
number, repeat.  A plan names surfaces by id; the kernels know them by primitive index.  ``prt_scene_update`` rewrites
the scene in place, and a reordered component list or a part replaced by a new one (a new id) moves those indices: the
plan must follow.

The reference of every check is a plain float64 restatement of the EDITED system -- the numpy oracle's frame of the
edited snapshot, filtered by surface and reduced by the frame oracle, or the full trace() of a new RayTracer built on
the edited system -- never the kernel compared with itself.  Also here: SinkStats.mean_square over several groups,
what "last" means for the fused sums, the RayTracer's host state after a failed update, and the dense-mode hints of a
sums-only plan on a stop that absorbs a few rays.
"""
import numpy as np
import pytest

import helpers
import scenes
from oracle import frame_oracle
from oracle import prt_oracle
from pyrayt_amd import engine
from pyrayt_amd.frame import DeviceFrame, SinkStats

# (tools/run_matrix.sh runs the suites under every trace flag: a plan's traces run on the fused path only)
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(bool(engine.DEFAULT_TRACE_FLAGS & (engine.TRACE_UNFUSED | engine.TRACE_COUNT_PATHS)),
                                                  reason="record plans need the fused path")]

torch = pytest.importorskip("torch")

LIMIT = 10
N = 4000
BUILDERS = {
    "config2": lambda api: scenes.config2(api, N),
    "config3": lambda api: scenes.config3(api, N),
    "config5": lambda api: scenes.config5(api, N),
    "mirrors_and_stops": lambda api: scenes.mirrors_and_stops(api, N),
    "stopped_lens": lambda api: scenes.stopped_lens(api, N),
    "adv_bench_a": scenes.adv_bench_a,
    # (two-part scenes have no other order of the same program shape -- a lens and a baffle compile to component
    # programs of different sizes: prt_scene_update refuses the swap -- so their reordering swaps two detectors)
    "config2_two_detectors": lambda api: two_detectors(scenes.config2(api, N), api, 1.5),
    "config5_two_detectors": lambda api: two_detectors(scenes.config5(api, N), api, 7.0),
}


def two_detectors(scene, api, x):
    parts, rays = scene
    return list(parts) + [api.components.baffle((8, 8)).move_x(x)], rays


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to("cuda:0")


def snapshot(parts):
    from pyrayt_amd.scene import SceneSnapshot

    return SceneSnapshot(list(parts))


def build(name, reset=True):
    from pyrayt_amd.g3d.objects import CountedObject

    if reset:
        CountedObject.reset_ids()
    parts, rays = BUILDERS[name](scenes.product_api())
    return list(parts), rays


def oracle_frame(parts, rays):
    frame, _ = prt_oracle.trace(helpers.flat_scene(snapshot(parts)), rays, LIMIT)
    return frame


def filtered(frame, ids):
    return frame[np.isin(frame[:, 5].astype(np.int64), np.asarray(ids, dtype=np.int64))]


def counts_of(frame):
    counts = [int((frame[:, 0] == g).sum()) for g in range(LIMIT)]
    while counts and counts[-1] == 0:
        counts.pop()
    return counts


def imager_and_pair(frame):
    """The surface the frame's last generation hits most (the "imager"), and it with the most frequent other one."""
    surf = frame[:, 5].astype(np.int64)
    last = surf[frame[:, 0] == frame[:, 0].max()]
    ids, counts = np.unique(last, return_counts=True)
    imager = int(ids[np.argmax(counts)])
    others, other_counts = np.unique(surf[surf != imager], return_counts=True)
    return imager, (imager, int(others[np.argmax(other_counts)]))


def prim_index(snap, surface):
    where = np.nonzero(snap.prims["surface_id"] == surface)[0]
    return int(where[-1]) if len(where) else -1


def check(rows, counts, plan, frame, ids, what):
    """What a trace under `plan` gave against the oracle frame cut to `ids`: the rows (surface / generation / id exact),
    and the fused sums per generation to the bound of tests/test_gpu_record_plan.py."""
    sel = filtered(frame, ids)
    if plan.rows:
        helpers.assert_close_to_reference(rows.cpu().numpy().T, sel, what=what)
        assert counts == counts_of(sel), (what, counts, counts_of(sel))
    else:
        assert rows.shape[1] == 0 and sum(counts) == 0, what
    if plan.stats:
        torch.cuda.synchronize()
        got = plan.sums.cpu().numpy()
        for g in range(LIMIT):
            want = frame_oracle.reduce_sums(sel.T, None, float(g), None, 1)
            scale = np.maximum(np.abs(want), 1.0)
            assert np.all(np.abs(got[g, :, :9] - want) <= 1e-12 * scale * max(sel.shape[0], 1) ** 0.5 + 1e-300), (
                what, g, got[g, :, :9], want)


def edit(name, kind, ds, parts, imager, pair):
    """Apply edit `kind` to the scene `parts` were built into and put it into `ds` with update(), which must fit.
    Returns (edited parts, {old id: new id} of the surfaces of a replaced part)."""
    snap = snapshot(parts)
    renamed = {}
    if kind == "move":
        parts[-1].move_x(0.05)
        edited = parts
    elif kind == "reorder":
        # an order that keeps the program's shape (prt_scene_update refuses the others) and moves the imager's
        # primitive, else one that moves a primitive of the pair, else any
        import itertools

        orders = [[parts[k] for k in perm] for perm in itertools.permutations(range(len(parts)))][1:]
        for wanted in ((imager,), pair, None):
            for order in orders:
                moved = [int(s) for q, s in enumerate(snap.prims["surface_id"]) if prim_index(snapshot(order), int(s)) != q]
                if (any(s in moved for s in wanted) if wanted else moved) and ds.update(snapshot(order)):
                    return order, renamed
        pytest.fail(f"{name}: no reordering of the components fits the scene")
    else:  # "replace": the part that holds the imager, by a new one of the same kind (new ids)
        fresh, _ = build(name, reset=False)
        edited = None
        for k in range(len(parts)):
            trial = parts[:k] + [fresh[k]] + parts[k + 1:]
            changed = {int(a): int(b) for a, b in zip(snap.prims["surface_id"], snapshot(trial).prims["surface_id"]) if a != b}
            if imager in changed:
                edited, renamed = trial, changed
                break
        assert edited is not None, name
    assert ds.update(snapshot(edited)) is True, (name, kind)    # the in-place path ran
    return edited, renamed


def plan_cases(name):
    """The scene's rays, its oracle frame as built, the imager and a two-surface set."""
    parts, rays = build(name)
    frame = oracle_frame(parts, rays)
    imager, pair = imager_and_pair(frame)
    return rays, frame, imager, pair


# (config 2 and 5 have no reordering that fits: their two-detector forms stand in for them there)
EDITS = [(name, kind) for name in BUILDERS for kind in ("move", "reorder", "replace")
         if not (kind == "reorder" and name in ("config2", "config5"))]


@pytest.mark.parametrize("name, kind", EDITS)
@pytest.mark.parametrize("stats", [False, True])
def test_a_plan_follows_its_surfaces_through_update(name, kind, stats):
    """A rows plan (or a sums-only plan) on the imager and on a two-surface set, set before the update: after it, the
    first trace and two hinted ones give the rows / sums of the edited system's oracle frame cut to those ids.  A
    replaced part's old id matches nothing any more, and plans that list its new ids pass the replacement's rows."""
    rays, frame0, imager, pair = plan_cases(name)
    rays_d = dev(rays)
    for ids in [(imager,), pair]:
        parts, _ = build(name)
        ds = engine.DeviceScene(snapshot(parts))
        plan = engine.RecordPlan(surfaces=ids, rows=not stats, stats=stats, generation_limit=LIMIT)
        rows, counts = ds.trace(rays_d, LIMIT, plan=plan)
        check(rows, counts, plan, frame0, ids, f"{name} {ids} before the edit")
        edited, renamed = edit(name, kind, ds, parts, imager, pair)
        frame1 = oracle_frame(edited, rays)
        if kind == "replace":
            assert imager in renamed and not np.isin(frame1[:, 5], list(renamed)).any()   # (the old ids are gone)
        for attempt in range(3):   # (a first trace after the update, then two on the plan's own hints)
            rows, counts = ds.trace(rays_d, LIMIT)                            # (the plan set above stays in force)
            check(rows, counts, plan, frame1, ids, f"{name} {kind} {ids} attempt {attempt}")
        if kind == "replace":
            # a plan that lists the new ids (and an old one beside them) passes the replacement's rows
            new_ids = tuple(renamed.get(s, s) for s in ids)
            for listed in (new_ids, (imager,) + new_ids[:1]):
                plan = engine.RecordPlan(surfaces=listed, rows=not stats, stats=stats, generation_limit=LIMIT)
                for attempt in range(3):
                    rows, counts = ds.trace(rays_d, LIMIT, plan=plan)
                    check(rows, counts, plan, frame1, listed, f"{name} replaced, plan {listed} attempt {attempt}")
        ds.close()


@pytest.mark.parametrize("name", ["config2_two_detectors", "config3", "stopped_lens", "adv_bench_a"])
@pytest.mark.parametrize("kind", ["move", "reorder", "replace"])
def test_plans_of_two_tickets_in_flight_follow_an_update(name, kind):
    """Ticket 1 stores the imager's rows, ticket 2 sums them, both traced together (prt_trace_begin / end on two
    streams) before and after the update, against the oracle of the system as it is at the time."""
    rays, frame0, imager, pair = plan_cases(name)
    parts, _ = build(name)
    ds = engine.DeviceScene(snapshot(parts))
    rays_d = dev(rays)
    ids = pair
    plan_rows = engine.RecordPlan(surfaces=ids, rows=True, generation_limit=LIMIT)
    plan_sums = engine.RecordPlan(surfaces=ids, rows=False, stats=True, generation_limit=LIMIT)
    ds.set_plan(1, plan_rows)
    ds.set_plan(2, plan_sums)
    streams = ds.ticket_streams(rays_d.device, 3)
    outs = {t: torch.empty((15, rays_d.shape[1] * LIMIT), dtype=torch.float64, device="cuda:0") for t in (1, 2)}

    def both(frame, what):
        for ticket in (1, 2):
            streams[ticket].wait_stream(torch.cuda.current_stream())
            ds.trace_begin(ticket, rays_d, LIMIT, outs[ticket], stream=streams[ticket])
        results = {ticket: ds.trace_end(ticket) for ticket in (1, 2)}
        torch.cuda.synchronize()
        check(results[1][0], results[1][1], plan_rows, frame, ids, f"{what}, ticket 1 (rows)")
        check(results[2][0], results[2][1], plan_sums, frame, ids, f"{what}, ticket 2 (sums)")

    both(frame0, f"{name} before the edit")
    edited, renamed = edit(name, kind, ds, parts, imager, pair)
    frame1 = oracle_frame(edited, rays)
    for rounds in range(3):
        both(frame1, f"{name} {kind} round {rounds}")
    ds.close()


# --- through RayTracer ----------------------------------------------------------------------------------------------
RPS = 6_000


def raytracer_system(n_sources=3):
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    back = pyrayt.components.baffle((3, 3)).move_x(3)           # (a second detector: what a reordering can swap with)
    sources = [pyrayt.components.ConeOfRays(cone_angle=6).move_x(-1.9),
               pyrayt.components.ConeOfRays(cone_angle=4, wavelength=0.5).move_x(-1.9).move_y(0.05),
               pyrayt.components.ConeOfRays(cone_angle=2, wavelength=0.7).move_x(-2.1)][:n_sources]
    return pyrayt, sources, lens, det, back


def fresh_full(pyrayt, sources, components):
    """The whole frame (pandas) and DeviceFrame of a new tracer built on the system as it is now."""
    tracer = pyrayt.RayTracer(sources, list(components), rays_per_source=RPS)
    table = tracer.trace()
    return table, tracer.device_frame


def assert_rows_of(got, full, ids, what):
    want = full.loc[full["surface"].isin(list(ids))].reset_index(drop=True)
    helpers.assert_same_bits(got.to_numpy(), want.to_numpy(), what=what)


def assert_stats_of(stats, device_full, ids, n_groups, what):
    want = device_full.group_stats(surface=ids[0], rays_per_source=RPS, n_groups=n_groups)
    table = stats.group_stats()
    assert np.array_equal(table["count"].to_numpy(), want["count"].to_numpy()), (what, table, want)
    for column in ("y", "z", "rms_radius", "focus", "focus_std", "wavelength", "intensity"):
        assert np.allclose(table[column].to_numpy(), want[column].to_numpy(), rtol=1e-9, atol=1e-12, equal_nan=True), (
            what, column, table[column].to_numpy(), want[column].to_numpy())
    want_ms = device_full.mean_square("y_tilt", about=0.01, transform="sin", surface=ids[0], rays_per_source=RPS,
                                      n_groups=n_groups)
    got_ms = stats.mean_square(None, per_source=True)
    assert np.array_equal(got_ms["count"].to_numpy(), want_ms["count"].to_numpy()), what
    assert np.allclose(got_ms["mean_square"].to_numpy(), want_ms["mean_square"].to_numpy(), rtol=1e-10, atol=1e-300,
                       equal_nan=True), what


@pytest.mark.parametrize("n_sources", [2, 3])
@pytest.mark.parametrize("mode", ["record_only", "trace_stats"])
def test_raytracer_record_only_and_trace_stats_follow_the_edits(mode, n_sources):
    """record_only(det), or trace_stats(surface=det, rays_per_source=True, mean_square=...), while the detector
    moves, the component list is reordered and the detector is replaced by a new one: the scene is updated in place
    every time, and the rows / tables are those of a new tracer's full trace of the edited system, cut to the
    detector.  (One mode per test: the plan the tracer holds when the system is edited is the one traced next.)"""
    pyrayt, sources, lens, det, back = raytracer_system(n_sources)
    tracer = pyrayt.RayTracer(sources, [lens, det, back], rays_per_source=RPS)
    tracer.trace()
    scene = tracer._device_scene()

    def both(listed, what):
        full, device_full = fresh_full(pyrayt, sources, tracer.get_system())
        ids = pyrayt.RayTracer._surface_ids(listed)
        stats = None
        if mode == "record_only":
            assert_rows_of(tracer.record_only(*listed).trace(), full, ids, f"{what}: record_only")
        else:
            stats = tracer.trace_stats(surface=listed[0], rays_per_source=True, mean_square=("y_tilt", 0.01, "sin"))
            assert_stats_of(stats, device_full, ids, n_sources, f"{what}: trace_stats")
        assert tracer._device_scene() is scene, what                   # updated in place, not rebuilt
        return stats

    both([det], "first")
    for step in range(3):
        det.move_x(0.05)
        both([det], f"detector moved {step}")
    tracer.load_components([lens, back, det])     # (a lens and a baffle have programs of different shapes: not swapped)
    both([det], "reordered")
    new_det = pyrayt.components.baffle((1, 1)).move_x(1.15)
    tracer.load_components([lens, back, new_det])
    stats = both([det], "detector replaced, plan on the old id")
    if stats is not None:
        assert not stats.group_stats()["count"].any()                  # (the old id matches nothing)
    both([new_det], "detector replaced, plan on the new id")
    tracer.load_components([lens, new_det, back])
    both([new_det, lens], "replaced and reordered")


def test_sink_mean_square_over_all_groups_equals_the_frame_without_groups():
    """SinkStats.mean_square(g, per_source=False) of a plan with three groups and no surface filter == DeviceFrame
    .mean_square without rays_per_source, for g = None, "last" and every generation (without a filter both meanings of
    "last" are the frame's last generation)."""
    pyrayt, sources, lens, det, _ = raytracer_system(3)
    tracer = pyrayt.RayTracer(sources, [lens, det], rays_per_source=RPS)
    full = tracer.trace_device()
    for quantity, about, transform in (("y_tilt", 0.01, "sin"), ("axis_intercept", 1.0, None), ("y1", 0.0, None)):
        stats = tracer.trace_stats(rays_per_source=True, mean_square=(quantity, about, transform))
        assert stats.sums.shape[1] == 3
        assert stats.last_generation_number() == full.last_generation_number()
        for generation in [None, "last"] + list(range(LIMIT)):
            want = full.mean_square(quantity, about=about, transform=transform, generation=generation)
            got = stats.mean_square(generation, per_source=False)
            assert np.isclose(got, want, rtol=1e-10, atol=1e-300, equal_nan=True), (quantity, generation, got, want)


# --- host state of RayTracer ---------------------------------------------------------------------------------------
def test_a_failed_update_is_not_taken_for_a_current_scene(monkeypatch):
    """An update that raises, or a rebuild that raises after the old scene was closed: the next trace() with no
    further edit looks at the system again and gives the frame of a new tracer."""
    pyrayt, sources, lens, det, _ = raytracer_system(2)
    tracer = pyrayt.RayTracer(sources, [lens, det], rays_per_source=RPS)
    tracer.trace()
    det.move_x(0.05)
    original = engine.DeviceScene.update
    raised = []

    def failing_update(self, snap):
        if not raised:
            raised.append(1)
            raise RuntimeError("update failed (injected)")
        return original(self, snap)

    monkeypatch.setattr(engine.DeviceScene, "update", failing_update)
    with pytest.raises(RuntimeError, match="injected"):
        tracer.trace()
    got = tracer.trace()
    want, _ = fresh_full(pyrayt, sources, tracer.get_system())
    helpers.assert_same_bits(got.to_numpy(), want.to_numpy(), what="after a failed update")
    monkeypatch.undo()

    # the update does not fit, and building the new scene fails once
    original_class = engine.DeviceScene
    built = []

    def failing_build(snap, *args, **kwargs):
        if not built:
            built.append(1)
            raise RuntimeError("build failed (injected)")
        return original_class(snap, *args, **kwargs)

    det.move_x(0.05)
    monkeypatch.setattr(engine.DeviceScene, "update", lambda self, snap: False)
    monkeypatch.setattr(engine, "DeviceScene", failing_build)
    with pytest.raises(RuntimeError, match="injected"):
        tracer.trace()
    got = tracer.trace()
    monkeypatch.undo()
    want, _ = fresh_full(pyrayt, sources, tracer.get_system())
    helpers.assert_same_bits(got.to_numpy(), want.to_numpy(), what="after a failed rebuild")


def test_trace_ray_set_records_everything_after_plans():
    """trace_ray_set() after trace_stats() and after record_only() returns the whole frame, not the rows (or none) of
    the plan an earlier run left behind."""
    pyrayt, sources, lens, det, _ = raytracer_system(2)
    tracer = pyrayt.RayTracer(sources, [lens, det], rays_per_source=RPS)
    tracer.trace()
    rays_host = np.asarray(tracer.initial_ray_set())
    device = torch.device("cuda:0")
    want = pyrayt.RayTracer(sources, [lens, det], rays_per_source=RPS).trace_ray_set(rays_host, device)
    assert set(np.unique(want["surface"])) != {det.get_id()}             # (more than the detector's rows)
    tracer.trace_stats(surface=det)
    got = tracer.trace_ray_set(rays_host, device)
    helpers.assert_same_bits(got.to_numpy(), want.to_numpy(), what="trace_ray_set after trace_stats")
    tracer.record_only(det)
    tracer.trace()
    got = tracer.trace_ray_set(rays_host, device)
    helpers.assert_same_bits(got.to_numpy(), want.to_numpy(), what="trace_ray_set after record_only")


# --- what "last" means for the fused sums ----------------------------------------------------------------------------
def test_last_is_the_last_generation_of_the_filtered_rows():
    """SinkStats "last" under a surface filter is the highest generation in which a row of those surfaces was counted
    -- here lower than the frame's last generation, which is asserted first -- and its table is DeviceFrame.group_stats
    of the imager's rows in that generation."""
    fx = helpers.load("scene_adv_stop.npz")
    limit, frame = int(fx["generation_limit"]), fx["frame"]
    imager = 4
    imager_last = int(frame[frame[:, 5] == imager, 0].max())
    assert imager_last < int(frame[:, 0].max())                        # (the two meanings differ on this fixture)
    ds = engine.DeviceScene(helpers.FixtureSnapshot(helpers.scene_of(fx)))
    rays = dev(fx["rays0"])
    rows, counts = ds.trace(rays, limit, plan=None)
    full = DeviceFrame(rows.clone(), counts)
    plan = engine.RecordPlan(surfaces=(imager,), rows=False, stats=True, mean_square=("y1", 0.0, None),
                             generation_limit=limit)
    ds.trace(rays, limit, plan=plan)
    torch.cuda.synchronize()
    stats = SinkStats(plan.sums)
    assert stats.last_generation_number() == imager_last
    got, want = stats.group_stats("last"), full.group_stats(surface=imager, generation=imager_last)
    assert np.array_equal(got["count"].to_numpy(), want["count"].to_numpy()) and want["count"].iloc[0] > 0
    for column in ("y", "z", "rms_radius", "focus", "focus_std", "wavelength", "intensity"):
        assert np.allclose(got[column].to_numpy(), want[column].to_numpy(), rtol=1e-9, atol=1e-12, equal_nan=True), column
    want_ms = full.mean_square("y1", surface=imager, generation=imager_last)
    assert np.isclose(stats.mean_square("last"), want_ms, rtol=1e-10)
    ds.close()


# --- dense-mode hints of a sums-only plan behind a sparsely absorbing stop -------------------------------------------
def test_sums_only_plan_behind_a_sparsely_absorbing_stop_does_not_miss_again_and_again():
    """Config 2 with a stop just in front of the lens that absorbs 0 < k <= 1/64 of 200 000 rays: generation 0 learns to
    keep its absorbed rays (hint bit 5), which then arrive dead in generation 1.  Forty sums-only traces on the
    detector (past the every-32nd re-measure of that bit): every one's sums are the oracle's, and at most one hinted
    attempt is refuted over the whole run."""
    from pyrayt_amd.g3d.objects import CountedObject

    CountedObject.reset_ids()
    api = scenes.product_api()
    parts, rays = scenes.config2(api, 200_000)
    stop = api.components.aperture((3.0, 3.0), 0.3646).move_x(-0.3)
    parts = [stop] + parts
    detector = parts[-1].get_id()
    frame = oracle_frame(parts, rays)
    absorbed = int((frame[:, 0] == 0).sum() - (frame[:, 0] == 1).sum())
    assert 0 < absorbed * 64 <= rays.shape[1], absorbed                # (a sparse loss in generation 0)
    ds = engine.DeviceScene(snapshot(parts))
    rays_d = dev(rays)
    plan = engine.RecordPlan(surfaces=(detector,), rows=False, stats=True, generation_limit=LIMIT)
    before = ds.telemetry()
    for k in range(40):
        rows, counts = ds.trace(rays_d, LIMIT, plan=plan)
        check(rows, counts, plan, frame, (detector,), f"sums-only trace {k}")
    after = ds.telemetry()
    misses = after["plan_misses"] - before["plan_misses"]
    print(f"plan_misses over 40 sums-only traces: {misses} (plan_dense_launches "
          f"{after['plan_dense_launches'] - before['plan_dense_launches']} of {after['plan_launches'] - before['plan_launches']})")
    assert misses <= 1, (misses, before, after)
    ds.close()
