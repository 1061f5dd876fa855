"""Sensitivities of the frame, the parts that need no GPU: the refusals of Motion / sensitivity(), the numpy longdouble
reference (tests/sensitivity_reference.py) against closed forms, and the reference against Richardson-checked central
differences of the C oracle's own traces of the moved system."""
import numpy as np
import pytest

import sensitivity_reference as ref
import sensitivity_scenes as cases

EPS = np.finfo(np.float64).eps


def reference_of(case):
    from pyrayt_amd.scene import SceneSnapshot

    table = ref.table_of(SceneSnapshot(case.parts).prims)
    return ref.trace_tangents(case.frame, table, [ref.parameter(m) for m in case.motions])


# ---- input validation ------------------------------------------------------------------------------------------------------
def test_motion_refuses_bad_input():
    from pyrayt_amd import Motion

    with pytest.raises(ValueError):
        Motion("lens")
    with pytest.raises(ValueError):
        Motion(3, translate=(1, 2))
    with pytest.raises(ValueError):
        Motion(3, rotate=(0, np.nan, 0))
    with pytest.raises(ValueError):
        Motion(3, pivot=(0, 0, np.inf))
    with pytest.raises(ValueError):
        Motion(2.5)

    class Many:
        surface_ids = tuple((k, None) for k in range(65))

    with pytest.raises(ValueError, match="64"):
        Motion(Many())
    m = Motion(7, translate=(1, 0, 0), rotate=(0, 0, 2))
    assert m.surface_ids == (7,) and m.twist.tolist() == [1, 0, 0, 0, 0, 2, 0, 0, 0]


def test_a_component_moves_all_its_surfaces_about_its_position():
    from pyrayt_amd import Motion, components

    lens = components.biconvex_lens(2, 2, 0.25, aperture=1).move(0.5, -0.25, 2.0)
    m = Motion(lens, rotate=(0, 0, 1))
    assert set(m.surface_ids) == {int(sid) for sid, _ in lens.surface_ids} and len(m.surface_ids) == 3
    assert m.pivot.tolist() == [0.5, -0.25, 2.0]


def host_frame(case):
    torch = pytest.importorskip("torch")
    from pyrayt_amd.frame import DeviceFrame

    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(case.frame.T)), case.counts)


def test_sensitivity_refuses_bad_input_before_it_needs_a_device():
    from pyrayt_amd import Motion

    case = cases.build("config2", 16)
    frame = host_frame(case)
    lens, det = case.parts
    good = case.motions
    with pytest.raises(ValueError, match="16"):
        frame.sensitivity(det, [good[0]] * 17, case.parts)
    with pytest.raises(ValueError, match="Motion"):
        frame.sensitivity(det, [], case.parts)
    with pytest.raises(ValueError, match="Motion"):
        frame.sensitivity(det, [(1, 0, 0)], case.parts)
    with pytest.raises(ValueError, match="not in system"):
        frame.sensitivity(det, good, [det])  # (the lens moves, and is not there)
    with pytest.raises(ValueError, match="weights"):
        frame.sensitivity(det, good, case.parts, weights="energy")
    with pytest.raises(ValueError, match="reference"):
        frame.sensitivity(det, good, case.parts, reference="focus")
    with pytest.raises(ValueError, match="surface"):
        frame.sensitivity(None, good, case.parts)
    with pytest.raises(ValueError, match="whole frame"):
        frame.generation(0).sensitivity(det, good, case.parts)
    with pytest.raises(ValueError):
        Motion(lens, translate=(0, 0))


def test_trace_sensitivity_says_that_a_record_only_cut_cannot_serve_it():
    import pyrayt_amd as prt

    case = cases.build("config2", 16)
    lens, det = case.parts
    tracer = prt.RayTracer(prt.components.ConeOfRays(6).move_x(-1.9), list(case.parts))
    tracer.record_only(det)
    with pytest.raises(ValueError, match="record_only"):
        tracer.trace_sensitivity(det, case.motions)


# ---- the reference against closed forms -----------------------------------------------------------------------------------
def test_reference_detector_translated():
    case = cases.build("detector_shift", 65)
    dx, _, count = reference_of(case)
    frame = case.frame
    d = frame[:, 12:15]
    normal = np.asarray(case.parts[0].get_orientation(), dtype=float).reshape(-1)[:3]
    want = d * ((normal @ case.velocity) / (d @ normal))[:, None]
    assert len(frame) == 65 and not any(count.values())
    assert np.max(np.abs(dx[0] - want)) <= 8 * EPS


@pytest.mark.parametrize("name", ["plane_slide", "sphere_spin", "cylinder_spin"])
def test_reference_invariant_motions_move_nothing(name):
    case = cases.build(name, 65)
    dx, _, count = reference_of(case)
    assert len(case.frame) >= 65 and np.all(np.isfinite(dx.astype(float)))
    assert (count["n_unknown"], count["n_invalid"], count["n_unfit"]) == (0, 0, 0)
    if name != "plane_slide":
        assert len(case.counts) >= 2 and case.counts[1] > 30  # (the part is met, and the rays go on)
    # exact zero up to the roundings of longdouble on velocities of size 1 through at most three interfaces; the recorded
    # landing points are float64, off the surface by ~1e-16, which the curvature turns into ~1e-15 of normal
    assert np.max(np.abs(dx)) <= 1e-13


def test_reference_flat_mirror_turned_about_the_hit_point():
    case = cases.build("flat_mirror", 6)
    dx, dd, count = reference_of(case)
    frame = case.frame
    second = np.flatnonzero(frame[:, 0] == 1)
    assert len(second) == 6 and count["n_reflections"] == 6
    for k, row in enumerate(second):
        ray = int(frame[row, 4])
        want = 2 * np.cross(case.axes[ray], frame[row, 12:15])
        assert np.max(np.abs(dd[ray, row] - want)) <= 16 * EPS, (k, dd[ray, row], want)
        first = np.flatnonzero((frame[:, 0] == 0) & (frame[:, 4] == ray))[0]
        assert np.max(np.abs(dx[ray, first])) <= 16 * EPS  # (the hit point lies on the axis: it stays)


# ---- the reference against central differences of the oracle's traces ------------------------------------------------------
def moved_trace(case, k, amount):
    """The oracle's frame of the system, built afresh, with parameter k applied by `amount`."""
    fresh = cases._BUILDERS[case.name](case.rays.shape[1])
    motion = fresh.motions[k]
    matrix = ref.rigid(motion.rotate, motion.pivot, amount, motion.translate)
    moved = 0
    for part in fresh.parts:
        if set(int(sid) for sid, _ in part.surface_ids) <= set(motion.surface_ids):
            part.transform(matrix)
            moved += 1
    assert moved == 1
    frame, counts = cases.trace(fresh.parts, case.rays, case.limit)
    return frame, counts, fresh.parts


def difference(case, k, h):
    """D(h) (R, 3) of the landing points by central differences, and whether each row kept its surface sequence."""
    plus, counts_p, parts_p = moved_trace(case, k, h)
    minus, counts_m, parts_m = moved_trace(case, k, -h)
    same = counts_p == case.counts and counts_m == case.counts
    if not same:
        return None, np.zeros(len(case.frame), dtype=bool)
    # (a system built afresh draws new surface ids: compare the sequences through the order of the ids)
    def rank(frame):
        return np.searchsorted(np.unique(frame[:, 5]), frame[:, 5])

    keep = (rank(plus) == rank(case.frame)) & (rank(minus) == rank(case.frame))
    keep &= (plus[:, 4] == case.frame[:, 4]) & (minus[:, 4] == case.frame[:, 4])
    return (plus[:, 9:12] - minus[:, 9:12]) / (2 * h), keep


def test_reference_against_central_differences_of_the_oracle_on_the_lens():
    case = cases.build("config2", 257)
    dx, _, count = reference_of(case)
    assert not any(count.values()) and case.counts == [257, 257, 257]
    # h from the oracle alone: the smallest power of four at which its own Richardson estimate is still truncation, not
    # rounding (the median of (4/3) |D(h) - D(h/2)| over the moving elements at least ten times the rounding floor).  At
    # 2^-12 it is 25 times the floor, at 2^-14 a third of it; no ray changes its path at any h from 2^-6 to 2^-16 (the
    # beam, radius <= 0.2 at a lens of clear radius 0.5, stays well inside every aperture).
    h = 2.0 ** -12
    worst = 0.0
    for k in range(3):
        coarse, keep_coarse = difference(case, k, h)
        fine, keep_fine = difference(case, k, h / 2)
        keep = keep_coarse & keep_fine
        assert keep.all(), f"parameter {k}: {np.sum(~keep)} rows changed their path"  # (the share left out is zero)
        floor = 4 * EPS * np.max(np.abs(case.frame[:, 9:12])) / h
        estimate = (4.0 / 3.0) * np.abs(coarse - fine)
        if k < 2:  # (the detector's shift is exact in h: nothing to estimate there)
            assert np.median(estimate[estimate > 0]) >= 10 * floor, (k, float(np.median(estimate)), floor)
        bound = estimate + floor
        error = np.abs(dx[k].astype(float) - fine)
        print(f"parameter {k}: max error {error.max():.3e}, max bound {bound.max():.3e}, "
              f"worst error / bound {np.max(error / bound):.3f}")
        worst = max(worst, float(np.max(error / bound)))
        assert np.all(error <= bound), (k, float(np.max(error / bound)))
    assert worst > 0.0


def test_group_sums_unpack_to_what_they_pack():
    rng = np.random.default_rng(3)
    K, n = 3, 40
    x, w, dx = rng.normal(size=(n, 3)), rng.uniform(1, 2, n), rng.normal(size=(K, n, 3))
    dx[1, 5] = np.nan
    want = ref.group_sums(x, w, dx, (0.1, 0.2, 0.3))
    lower = want["moments"][np.tril_indices(K)]
    row = np.concatenate([[want["count"], want["w"]], want["wx"], [want["wrr"]], want["wd"].reshape(-1), want["wrd"], lower])
    got = ref.unpack(row.astype(float), K)
    assert got["count"] == n - 1
    for name in ("w", "wx", "wrr", "wd", "wrd", "moments"):
        assert np.allclose(np.asarray(got[name], dtype=float), np.asarray(want[name], dtype=float), rtol=1e-15, atol=0)


def test_the_sensitivity_class_turns_sums_into_gradients():
    """Sensitivity's host arithmetic against a direct evaluation: two parameters that shift every landing point."""
    from pyrayt_amd.frame import Sensitivity

    rng = np.random.default_rng(4)
    K, n = 2, 50
    x, w, dx = rng.normal(size=(n, 3)), rng.uniform(1, 2, n), rng.normal(size=(K, n, 3))
    pivot = x[0]
    s = ref.group_sums(x, w, dx, pivot)
    row = np.concatenate([[s["count"], s["w"]], s["wx"], [s["wrr"]], s["wd"].reshape(-1), s["wrd"],
                          s["moments"][np.tril_indices(K)]]).astype(float)
    got = Sensitivity(None, None, row[None], pivot[None], True, np.zeros(4, dtype=np.int64), [None] * K)

    def mean_square(p):
        moved = x + np.einsum("k,knc->nc", p, dx)
        c = (w[:, None] * moved).sum(axis=0) / w.sum()
        return (w * np.sum((moved - c) ** 2, axis=1)).sum() / w.sum()

    e = 1e-6
    for k in range(K):
        step = np.zeros(K)
        step[k] = e
        numeric = (mean_square(step) - mean_square(-step)) / (2 * e)
        assert abs(got.mean_square_gradient[0, k] - numeric) <= 1e-8
    assert abs(got.mean_square[0] - mean_square(np.zeros(K))) <= 1e-13
    assert np.allclose(got.rms_radius_gradient[0], got.mean_square_gradient[0] / (2 * np.sqrt(got.mean_square[0])))
    # the landing points are linear in p here, so one undamped step lands on the minimum: the gradient vanishes there
    p = got.step()[0]
    for k in range(K):
        step = np.zeros(K)
        step[k] = e
        assert abs((mean_square(p + step) - mean_square(p - step)) / (2 * e)) <= 1e-8
    assert mean_square(p) <= mean_square(np.zeros(K))
