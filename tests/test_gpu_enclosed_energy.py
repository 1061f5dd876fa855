"""Geometric enclosed energy of the result frame on the device (DeviceFrame.enclosed_energy,
RayTracer.trace_enclosed_energy): against the numpy restatement of the definitions (tests/energy_reference.py) on a
synthetic frame and on one of the reference's frames, on shapes that cross the kernels' seams, against closed forms,
through focus against a moved detector, on cut frames bit for bit, and run twice for bit-identical outputs."""
import numpy as np
import pytest

import energy_reference as ref
import helpers
from test_gpu_mtf import config2_tracer, device_frame, synthetic_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX


def staged(frame, surface, options):
    from pyrayt_amd.frame import pupil_axes

    n_groups = options.get("n_groups", 1)
    reference = options.get("reference", "centroid")
    return ref.stage(frame, surface, pupil_axes(options.get("axis")), options.get("rays_per_source"), n_groups,
                     options.get("weights", "intensity"),
                     None if isinstance(reference, str) else np.broadcast_to(np.asarray(reference, float), (n_groups, 3)))


def clear_radii(frame, surface, count, **options):
    """`count` radii between the distances the restatement finds at every plane of every group."""
    follow, shape = options.get("follow_centroid", True), options.get("shape", "circle")
    found = [ref.distances(p, s, delta, ref.plane_centre(p, s, w, delta, follow), shape)
             for p, s, w, _, used, _ in staged(frame, surface, options) if used and w.sum() > 0
             for delta in options.get("focus", (0.0,))]
    return ref.clear_radii(np.concatenate(found), count)


def check(frame, device, surface, radii, shifts=True, **options):
    """The device against the restatement: energy equal (no ray within 1e-9 of a radius, asserted), radius to 1e-12;
    shifts=False leaves pbar and sbar out (values near 1e300 have no absolute 1e-12)."""
    got = device.enclosed_energy(surface, radii, **options)
    fractions = options.get("fractions", (0.5, 0.8, 0.9))
    fractions = () if fractions is None else fractions
    focus, radii = options.get("focus", (0.0,)), (() if radii is None else radii)
    groups = staged(frame, surface, options)
    assert got.energy.shape == (len(groups), len(focus), len(radii))
    assert got.radius.shape == (len(groups), len(focus), len(fractions))
    for g, (p, s, w, centre, used, missed) in enumerate(groups):
        energy, radius, margin = ref.enclosed(p, s, w, radii, fractions, focus, options.get("shape", "circle"),
                                              options.get("follow_centroid", True))
        assert margin > 1e-9, (g, margin)  # (what makes the equality below legitimate)
        assert np.array_equal(got.energy[g], energy, equal_nan=True), g
        np.testing.assert_allclose(got.radius[g], radius, rtol=1e-12, atol=0, equal_nan=True)
        assert got.n_rays[g] == used and got.n_missed[g] == missed
        np.testing.assert_allclose(got.centre[g], centre, rtol=0, atol=1e-12, equal_nan=True)
        if used and w.sum() > 0 and shifts:
            shift = np.stack([(w @ p) / w.sum(), (w @ s) / w.sum()])
            np.testing.assert_allclose(got.centroid_shift[g], shift, rtol=0, atol=1e-12)
            np.testing.assert_allclose(got.sum_weights[g], w.sum(), rtol=1e-12)
        if not (used and w.sum() > 0):
            assert np.all(np.isnan(got.energy[g])) and np.all(np.isnan(got.radius[g]))
    return got


def plane_frame(p, s, w, ids=None):
    """Rows at surface 4 whose staged rays about the origin are exactly (p, s, w): Q = (0, p), u = (1, s)."""
    p, s = np.asarray(p, dtype=float), np.asarray(s, dtype=float)
    frame = np.zeros((len(p), 15))
    frame[:, IX["intensity"]], frame[:, IX["surface"]] = w, 4.0
    frame[:, IX["id"]] = np.arange(len(p)) if ids is None else ids
    frame[:, 10:12], frame[:, 12], frame[:, 13:15] = p, 1.0, s
    return frame


ORIGIN = dict(reference=(0.0, 0.0, 0.0), follow_centroid=False)
SIXTEEN = tuple(np.linspace(0.03, 1.0, 16))


# ---- against the restatement --------------------------------------------------------------------------------------------
def test_enclosed_energy_against_numpy_on_a_synthetic_frame():
    frame, axis = synthetic_frame()
    device = device_frame(frame)
    two = dict(axis=axis, rays_per_source=6000, n_groups=2)
    options = dict(two, focus=(-0.05, 0.0, 0.02), fractions=(0.05, 0.2, 0.5, 0.8, 0.9, 0.95, 0.99, 1.0))
    got = check(frame, device, 5.0, clear_radii(frame, 5.0, 2, **options), **options)
    assert np.all(got.n_rays > 1000) and got.n_missed.sum() == 5 and np.all(got.sum_weights > 0)
    assert np.all(np.diff(got.radius, axis=2) >= 0) and np.all(np.diff(got.energy, axis=2) >= 0)
    # 41 planes x 130 radii: more than one tile of the curve's window; 13 fractions: more than one fraction tile
    options = dict(two, focus=tuple(np.linspace(-0.1, 0.1, 41)), fractions=SIXTEEN[:13], shape="square",
                   follow_centroid=False)
    check(frame, device, 5.0, clear_radii(frame, 5.0, 130, **options), **options)
    options = dict(axis=axis, weights=None, shape="slit_e1", reference=(0.0, -0.01, 0.02), fractions=(0.5,))
    check(frame, device, 5.0, clear_radii(frame, 5.0, 1, **options), **options)
    options = dict(two, shape="slit_e2", focus=(0.0, 0.3, -0.2), fractions=None)
    check(frame, device, 5.0, clear_radii(frame, 5.0, 130, **options), **options)
    options = dict(two, shape="circle", focus=(0.04,), fractions=SIXTEEN)
    check(frame, device, 5.0, None, **options)
    # a group without rays is NaN
    empty = device.enclosed_energy(5.0, [0.01], rays_per_source=6000, n_groups=3)
    assert np.all(np.isnan(empty.energy[2])) and np.all(np.isnan(empty.radius[2])) and empty.n_rays[2] == 0
    assert np.isnan(empty.best_focus(0.8)[2])


def test_enclosed_energy_against_numpy_on_a_reference_frame():
    frame = helpers.load("scene_config2.npz")["frame"]
    device = device_frame(frame)
    last = frame[:, 0].max()
    imager = float(frame[frame[:, 0] == last][-1, IX["surface"]])
    n_groups = int(frame[:, IX["id"]].max() // 512) + 1
    for shape in ref.SHAPES:
        options = dict(shape=shape, focus=(-0.2, 0.0, 0.3), rays_per_source=512, n_groups=n_groups)
        got = check(frame, device, imager, clear_radii(frame, imager, 9, **options), **options)
    assert got.n_rays.sum() > 500


# ---- shapes that cross the kernels' seams -------------------------------------------------------------------------------
def test_group_sizes_across_the_chunks_and_slices():
    """Rays used per group of 1, 63, 64, 65, 257, 4097 (two chunks, three slices) and 2049 (just past one slice), and a
    group without rays, in one frame."""
    sizes = (1, 63, 64, 65, 257, 4097, 2049, 0)
    per = 5000
    rng = np.random.default_rng(11)
    ids = np.concatenate([g * per + np.arange(n) for g, n in enumerate(sizes)]).astype(float)
    n = len(ids)
    weights = 0.5 + rng.random(n)
    weights[0] = 1.0  # (the lone ray of group 0 is then its own centroid exactly)
    frame = plane_frame(rng.normal(0, 0.01, (n, 2)), rng.normal(0, 0.05, (n, 2)), weights, ids)
    device = device_frame(frame)
    options = dict(rays_per_source=per, n_groups=len(sizes), focus=(-0.1, 0.0, 0.2), fractions=(0.3, 0.5, 0.8, 0.9, 1.0))
    got = check(frame, device, 4.0, clear_radii(frame, 4.0, 7, **options), **options)
    assert list(got.n_rays) == list(sizes)
    assert np.all(np.isfinite(got.radius[:-1])) and np.all(np.isnan(got.radius[-1]))
    # one ray: every fraction is its own distance, 0 about the centroid it is
    assert np.all(got.radius[0] == 0.0)


def test_one_point_a_ring_and_the_far_ends_of_the_doubles():
    # all rays at one point: every radius 0 and EE = 1 at R = 0
    n = 300
    frame = plane_frame(np.tile([0.25, -1.5], (n, 1)), np.zeros((n, 2)), np.ones(n))
    got = device_frame(frame).enclosed_energy(4.0, [0.0, 1.0], fractions=SIXTEEN)
    assert np.all(got.radius == 0.0) and np.all(got.energy == 1.0)
    # many exactly equal distances: the radius lands on the ring for every fraction
    ring = np.stack([np.full(640, 3.0), np.zeros(640)], 1)
    ring[::2] *= -1
    inner = np.array([[0.5, 0.0], [-0.5, 0.0]])
    frame = plane_frame(np.concatenate([inner, ring]), np.zeros((642, 2)), np.concatenate([[1.0, 1.0], np.full(640, 7.0)]))
    got = check(frame, device_frame(frame), 4.0, [1.0, 3.5], fractions=SIXTEEN, **ORIGIN)
    assert np.all(got.radius == 3.0) and got.energy[0, 0, 1] == 1.0
    # distances from 1e-300 to 1e300 in one group: every digit level of the select decides something
    spread = np.zeros((1201, 2))
    spread[:, 0] = 10.0 ** np.linspace(-300, 300, 1201) * np.where(np.arange(1201) % 2, -1.0, 1.0)
    frame = plane_frame(spread, np.zeros_like(spread), 1.0 + np.arange(1201) % 5)
    device = device_frame(frame)
    for shape in ("square", "circle", "slit_e2"):
        got = check(frame, device, 4.0, [2e-290, 3e-7, 2.0, 3e150, 2e299], shifts=False, fractions=SIXTEEN, shape=shape,
                    **ORIGIN)
        # (a circle squares the coordinates: below 1e-162 the distance is 0, above 1e154 it is +inf)
        assert got.radius.min() < 1e-100 and got.radius.max() == (np.inf if shape == "circle" else 1e300)
    # one ray whose distance overflows to +inf at a far plane
    p = np.array([[1.0, 0.0], [0.0, 2.0], [-3.0, 0.0], [0.5, 0.5]])
    s = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [1e200, 0.0]])
    frame = plane_frame(p, s, np.ones(4))
    got = check(frame, device_frame(frame), 4.0, [2.5, 1e308], fractions=(0.5, 0.75, 1.0), focus=(0.0, 1e200), **ORIGIN)
    assert got.radius[0, 1, 2] == np.inf and got.energy[0, 1, 1] == 0.75 and np.isfinite(got.radius[0, 0]).all()


# ---- closed forms -------------------------------------------------------------------------------------------------------
def test_a_vogel_disk_a_square_lattice_and_a_perfect_cone():
    n, a = 10_000, 0.37
    p, r = ref.vogel_disk(n, a)
    radii = ref.clear_radii(r, 50)
    fractions = np.array([0.1, 0.5, 0.8, 0.9, 1.0])
    got = device_frame(plane_frame(p, np.zeros((n, 2)), np.ones(n))).enclosed_energy(4.0, radii, fractions=fractions,
                                                                                      **ORIGIN)
    assert np.abs(got.energy[0, 0] - (radii / a) ** 2).max() <= 1.0 / n
    np.testing.assert_allclose(got.radius[0, 0], a * np.sqrt((np.ceil(fractions * n) - 0.5) / n), rtol=1e-12)
    side = 100
    grid = (np.arange(side) + 0.5) / side * 2 * a - a
    lattice = np.stack(np.meshgrid(grid, grid, indexing="ij"), -1).reshape(-1, 2)
    half = ref.clear_radii(np.abs(lattice).max(1), 20)
    got = device_frame(plane_frame(lattice, np.zeros_like(lattice), np.ones(len(lattice)))).enclosed_energy(
        4.0, half, fractions=(0.25, 1.0), shape="square", **ORIGIN)
    assert np.all(np.abs(got.energy[0, 0] - (half / a) ** 2) <= 4 * (half / a) / side + 4 / side ** 2)
    np.testing.assert_allclose(got.radius[0, 0], [grid[74], grid[99]], rtol=1e-12)
    # a perfect cone converging at delta0, a sampled plane: radius = |delta - delta0| x the slope quantile
    m, delta0 = 4001, 0.25
    _, slope = ref.vogel_disk(m, 0.1)
    t = np.arange(m) * 2.399963229728653
    s = np.stack([slope * np.cos(t), slope * np.sin(t)], 1)
    focus = np.linspace(-0.25, 0.75, 17)  # (0.25 is sample 8, exactly)
    got = device_frame(plane_frame(-delta0 * s, s, np.ones(m))).enclosed_energy(4.0, None, fractions=(0.8,), focus=focus,
                                                                               **ORIGIN)
    quantile = np.sort(np.hypot(s[:, 0], s[:, 1]))[int(np.ceil(0.8 * m)) - 1]
    np.testing.assert_allclose(got.radius[0, :, 0], np.abs(focus - delta0) * quantile, rtol=1e-12, atol=1e-17)
    assert got.best_focus(0.8)[0] == delta0


# ---- through focus against a moved detector -----------------------------------------------------------------------------
def test_through_focus_equals_a_moved_detector():
    """The radius at focus = delta against a re-trace with the detector moved by delta, to the 1e-9 (absolute) that
    tests/test_gpu_mtf.py::test_through_focus_equals_a_moved_detector asks of the MTF."""
    tracer, lens, det = config2_tracer(20_000, baffle=(20, 20))
    shifted = tracer.trace_enclosed_energy(det, fractions=(0.5, 0.8, 0.9), focus=[0.05])
    moved, lens, det2 = config2_tracer(20_000, baffle=(20, 20), det_x=1.05)
    fresh = moved.trace_enclosed_energy(det2, fractions=(0.5, 0.8, 0.9))
    assert shifted.n_rays[0] == fresh.n_rays[0] > 19_000
    print("moved detector: radius", shifted.radius[0, 0], fresh.radius[0, 0], "difference",
          np.abs(shifted.radius - fresh.radius).max())
    assert np.abs(shifted.radius - fresh.radius).max() <= 1e-9


# ---- cut frames, trace_enclosed_energy, reproducibility -----------------------------------------------------------------
def same(a, b):
    for name in ("energy", "radius", "record", "radii", "fractions", "focus"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


def test_cut_frames_give_the_same_bits_and_trace_enclosed_energy():
    tracer, lens, det = config2_tracer(100_000)
    radii = np.linspace(0.001, 0.2, 64)
    options = dict(fractions=(0.5, 0.8, 0.9), focus=(-0.1, 0.0, 0.05))
    frame = tracer.trace_device()
    whole = frame.enclosed_energy(det, radii, **options)
    same(whole, frame.enclosed_energy(det, radii, **options))
    same(whole, frame.where(surface=det.get_id()).enclosed_energy(det, radii, **options))
    same(whole, frame.where(surface=det.get_id()).enclosed_energy(None, radii, **options))
    tracer.record_only(det)
    same(whole, tracer.trace_device().enclosed_energy(det, radii, **options))
    tracer.record_only()
    same(whole, tracer.trace_enclosed_energy(det, radii, **options))
    assert whole.n_rays[0] > 90_000 and np.all(np.isfinite(whole.radius)) and whole.energy.max() <= 1.0
    assert np.all(np.diff(whole.energy, axis=2) >= 0) and np.all(np.diff(whole.radius, axis=2) >= 0)
    # an active record_only() setting survives the call
    tracer.record_only(det, columns=("y1", "z1"))
    spot = tracer.trace().to_numpy(dtype=float)
    tracer.trace_enclosed_energy(det, radii, rays_per_source=True)
    assert tracer._record_surfaces == (det.get_id(),) and tracer._record_columns == ("y1", "z1")
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), spot)
    with pytest.raises(ValueError, match="without the column"):
        tracer.trace_device().enclosed_energy(det, radii)


# ---- the staging pass shared with mtf() ---------------------------------------------------------------------------------
def test_mtf_and_enclosed_energy_stage_the_same_rays():
    """mtf() and enclosed_energy() of one frame and one set of arguments run one staging pass: each group's centre, sum
    of weights, rays used and rays left out are the same bits in both records.  1, 2049 and 4097 rays among 4196 rows of
    another surface (one chunk and one slice, two slices, two chunks and three slices), and three groups of which the
    middle one keeps no ray; every group also holds a row with a NaN end point, one with u.a == 0 and one with a
    negative weight, so that ``missed`` is not zero -- which the host reference says before the device is asked.  The
    two passes add up sum w in different orders (slices, chunks), so the weights are multiples of 1/8 below 8: their
    sum is exact in any order."""
    import diffraction_reference as R
    from pyrayt_amd.frame import pupil_axes

    for counts, filler in (([1], 4196), ([2049], 4196), ([4097], 4196), ([300, 0, 2049], 0)):
        case = R.mtf_case(counts, filler=filler, left_out=3, seed=130 + counts[0])
        frame = case.frame
        here = frame[:, IX["surface"]] == R.SURFACE
        frame[here, IX["intensity"]] = np.where(frame[here, IX["intensity"]] < 0, -1.0,
                                                np.floor(frame[here, IX["intensity"]] % 7 * 8 + 8) / 8)
        rows, group = R.select_rows(frame, R.SURFACE, case.rays_per_source, case.n_groups)
        kept = R.mtf_kept(rows[:, 9:12], rows[:, 12:15], rows[:, IX["intensity"]], pupil_axes())
        missed = np.bincount(group[~kept], minlength=case.n_groups)
        used = np.bincount(group[kept], minlength=case.n_groups)
        assert list(used) == counts and list(missed) == [3] * len(counts)  # (a vacuous case must not pass)
        assert np.isnan(rows[~kept, 10]).sum() == len(counts) and (rows[~kept, 12] == 0.0).sum() == len(counts)
        device = device_frame(frame)
        given = np.linspace(-1e-3, 2e-3, 3 * case.n_groups).reshape(case.n_groups, 3)
        for reference in ("centroid", given):
            options = dict(case.options, reference=reference, focus=(0.0, 0.03))
            mtf = device.mtf(R.SURFACE, [0.0, 40.0], **options)
            energy = device.enclosed_energy(R.SURFACE, [0.01], **options)
            what = (counts, "centroid" if isinstance(reference, str) else "given")
            assert list(mtf.record[:, 5]) == list(missed) and list(mtf.record[:, 4]) == counts, what
            for ours, theirs in ((slice(0, 3), slice(0, 3)), (3, 7), (4, 8), (5, 9)):
                a = np.ascontiguousarray(mtf.record[:, ours]).view(np.uint64)
                b = np.ascontiguousarray(energy.record[:, theirs]).view(np.uint64)
                assert np.array_equal(a, b), (what, ours, mtf.record[:, ours], energy.record[:, theirs])
            if not isinstance(reference, str):
                assert np.array_equal(mtf.record[:, :3], given)
