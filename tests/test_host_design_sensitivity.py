"""Shape and index sensitivities of the frame, the parts that need no GPU: the refusals of Deformation / IndexChange, the
agreement of ``Deformation.matrix`` with the velocity field, the numpy longdouble reference (tests/design_reference.py)
against closed forms, and the reference against Richardson-checked central differences of the C oracle's own traces of
the system changed by ``Deformation.apply`` (for the index: built with a glass of index n +- h)."""
import numpy as np
import pytest

import design_reference as ref
import design_scenes as cases

EPS = np.finfo(np.float64).eps


def reference_of(case):
    from pyrayt_amd.scene import SceneSnapshot

    table = ref.table_of(SceneSnapshot(case.parts).prims)
    return ref.trace_tangents(case.frame, table, [ref.parameter(m) for m in case.parameters])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_deformation_and_index_change_refuse_bad_input():
    import pyrayt_amd as prt
    from pyrayt_amd import Deformation, IndexChange

    ball = prt.g3d.Sphere(0.5, material=prt.materials.glass["BK7"])
    rod = prt.g3d.Cylinder(0.5, -1, 1, material=prt.materials.mirror)
    dish = prt.g3d.Paraboloid(2.0, 0.5, material=prt.materials.mirror)
    box = prt.g3d.Cuboid.from_sides(1, 1, 1, material=prt.materials.mirror)
    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    for wrong in (dish, box, lens, 7):
        with pytest.raises(ValueError, match="radius"):
            Deformation.radius(wrong)
    for wrong in (ball, rod, box, lens, 7):
        with pytest.raises(ValueError, match="focus"):
            Deformation.focus(wrong)
    for linear in (np.full((3, 3), np.nan), [[1, 0, 0], [0, np.inf, 0], [0, 0, 1]], np.eye(2), "shear"):
        with pytest.raises(ValueError, match="linear"):
            Deformation(ball, linear=linear)
    with pytest.raises(ValueError):
        Deformation(ball, translate=(0, np.nan, 0))
    with pytest.raises(ValueError, match="axis"):
        Deformation.stretch(box, (0, 0, 0))
    for wrong in (rod, box, prt.components.baffle((1, 1)), prt.components.spherical_mirror(4.0, 0.3)):
        with pytest.raises(ValueError, match="glass"):
            IndexChange(wrong)
    with pytest.raises(ValueError, match="rate"):
        IndexChange(ball, rate=np.nan)
    with pytest.raises(ValueError):
        IndexChange(7)
    with pytest.raises(ValueError, match="bare id"):
        Deformation(7, translate=(1, 0, 0)).apply(0.1)
    assert IndexChange(lens).surface_ids == tuple(sorted(int(sid) for sid, _ in lens.surface_ids))
    assert Deformation.radius(ball).surface_ids == (ball.get_id(),) and Deformation.radius(rod).linear[2, 2] == 0
    assert not Deformation(ball, translate=(1, 0, 0)).linear.any()


def test_sensitivity_refuses_a_bad_mix_before_it_needs_a_device():
    torch = pytest.importorskip("torch")
    from pyrayt_amd import Deformation, IndexChange
    from pyrayt_amd.frame import DeviceFrame

    case = cases.build("lens", 16)
    frame = DeviceFrame(torch.from_numpy(np.ascontiguousarray(case.frame.T)), case.counts)
    lens, det = case.parts
    with pytest.raises(ValueError, match="16"):
        frame.sensitivity(det, [case.parameters[0]] * 17, case.parts)
    with pytest.raises(ValueError, match="Deformation"):
        frame.sensitivity(det, [case.parameters[0], (1, 0, 0)], case.parts)
    with pytest.raises(ValueError, match="not in system"):
        frame.sensitivity(det, [Deformation.radius(lens.surface_ids[0][1])], [det])
    with pytest.raises(ValueError, match="not in system"):
        frame.sensitivity(det, [IndexChange(lens)], [det])


# ---- matrix() against the velocity field ----------------------------------------------------------------------------------
def test_matrix_is_the_finite_transform_whose_derivative_is_the_velocity_field():
    import pyrayt_amd as prt
    from pyrayt_amd import Deformation

    ball = prt.g3d.Sphere(0.7, material=prt.materials.glass["BK7"]).scale(1.0, 1.6, 0.8).rotate_z(25).move(0.2, 0.1, 0.0)
    rod = prt.g3d.Cylinder(0.5, -1, 1, material=prt.materials.mirror).scale(1.4, 0.7, 1.0).rotate_x(90).move(0, 0.3, 0.2)
    dish = prt.g3d.Paraboloid(2.0, 0.5, material=prt.materials.mirror).rotate_y(90).move(-1, 0, 0.5)
    shear = [[0.1, 0.4, 0.0], [-0.3, 0.2, 0.5], [0.0, 0.1, -0.2]]
    every = [Deformation.radius(ball), Deformation.radius(ball, keep=(0.5, 0.2, -0.1)), Deformation.radius(rod),
             Deformation.radius(rod, keep=(1, 1, 1)), Deformation.focus(dish), Deformation.focus(dish, keep=(0.2, 0, 0)),
             Deformation.stretch(rod, (0.3, 1.0, -0.2)), Deformation.stretch(rod, (0, 0, 1), about=(0.5, 0.5, 0.5)),
             Deformation(ball, translate=(0.3, -0.2, 0.5), rotate=(0.1, 0.7, -0.4), linear=shear, pivot=(0.5, 0.1, 0.0)),
             Deformation(ball, rotate=(0, 0, 1)), Deformation(ball, linear=shear)]
    h = 2.0 ** -10
    for k, one in enumerate(every):
        numeric = (one.matrix(h) - one.matrix(-h)) / (2 * h)
        # the truncation of the central difference: h^2 / 6 times the third derivative, at most |G|^3 e^(h |G|) here
        size = np.linalg.norm(one.generator(), 2)
        assert np.abs(numeric - one.generator()).max() <= h * h * max(size, 1.0) ** 3 + 64 * EPS / h, k
        assert np.array_equal(one.matrix(0.0), np.eye(4)) or np.abs(one.matrix(0.0) - np.eye(4)).max() <= 8 * EPS
        v, w, s, c = one.translate, one.rotate, one.linear, one.pivot
        x = np.array([0.3, -1.1, 0.7])
        assert np.allclose(one.generator() @ np.append(x, 1), np.append(v + np.cross(w, x - c) + s @ (x - c), 0),
                           rtol=0, atol=1e-15)
    # a radius change is exact: the sphere of radius R scaled by (R + a) / R about the kept point, which stays
    grown = Deformation.radius(ball, keep=(0.5, 0.2, -0.1)).matrix(0.35)
    assert np.allclose(grown @ [0.5, 0.2, -0.1, 1], [0.5, 0.2, -0.1, 1], rtol=0, atol=1e-15)
    assert np.allclose(grown[:3, :3], np.eye(3) * (0.7 + 0.35) / 0.7, rtol=0, atol=1e-15)
    wider = Deformation.focus(dish).matrix(1.0)
    local = np.asarray(dish.get_object_transform()) @ wider @ np.asarray(dish.get_world_transform())
    assert np.allclose(local, np.diag([np.sqrt(1.5), np.sqrt(1.5), 1, 1]), rtol=0, atol=1e-14)


def test_apply_transforms_the_leaves_and_the_scene_sees_it():
    import pyrayt_amd as prt
    from pyrayt_amd import Deformation
    from pyrayt_amd.g3d.objects import SceneEpoch

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    front = lens.surface_ids[0][1]
    before, epoch = front.get_world_transform(), SceneEpoch.value
    one = Deformation.radius(front, keep=(-0.125, 0, 0))
    assert one.apply(0.5) is one and SceneEpoch.value > epoch
    assert np.allclose(front.get_world_transform(), one.matrix(0.5) @ before)
    # the sphere of radius 2 is one of radius 2.5 now, and its vertex is where it was
    centre = np.asarray(front.get_position(), dtype=float).reshape(-1)[:3]
    assert np.allclose(centre, [-0.125 + 2.5, 0, 0], atol=1e-14)
    assert np.allclose(np.asarray(lens.surface_ids[1][1].get_position()).reshape(-1)[:3], [0.125 - 2, 0, 0], atol=1e-14)


# ---- the reference against closed forms -------------------------------------------------------------------------------------
def test_reference_ball_whose_radius_grows_about_its_centre():
    case = cases.build("ball_radius", 65)
    dx, dd, count = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65, 65] and not any(count.values())
    d, g = f[:, 12:15], f[:, 0]
    # the recorded landing points are float64, off the ball by ~1e-16, which its curvature (1 / 0.8) and the path to the
    # detector (4 units) turn into ~1e-15
    assert np.max(np.abs(dx[0][g == 0] + d[g == 0])) <= 32 * EPS
    assert np.max(np.abs(dx[0][g == 1] - d[g == 1])) <= 32 * EPS
    assert np.max(np.abs(dx[0][g == 2])) <= 64 * EPS and np.nanmax(np.abs(dd[0])) <= 32 * EPS


@pytest.mark.parametrize("name", ["plane_stretch", "cylinder_stretch"])
def test_reference_invariant_deformations_move_nothing(name):
    case = cases.build(name, 65)
    dx, _, count = reference_of(case)
    assert len(case.frame) >= 65 and np.all(np.isfinite(dx.astype(float)))
    assert (count["n_unknown"], count["n_invalid"], count["n_unfit"]) == (0, 0, 0)
    if name == "cylinder_stretch":
        from pyrayt_amd.scene import SceneSnapshot

        assert case.counts[1] > 30 and count["n_reflections"] == case.counts[1]
        rod = SceneSnapshot(case.parts).prims[0]
        local = case.frame[case.frame[:, 0] == 0][:, 9:12] @ rod["minv"].reshape(4, 4)[:3, :3].T + rod["minv"].reshape(4, 4)[:3, 3]
        assert np.all(np.abs(local[:, 2]) < 1.4)  # (met on the wall: the caps are at +-1.5)
    assert np.max(np.abs(dx)) <= 1e-13  # (as tests/test_host_sensitivity.py puts it for the rigid invariances)


def test_reference_similarity_about_the_source_point():
    """The ball scaled about the point all rays come from: dd = 0 everywhere, dx = x - P on the ball, and on the detector,
    which is not scaled, the exit point's shift carried along the unchanged direction: (I - d a^T / (a.d)) (x2 - P)."""
    case = cases.build("similarity", 65)
    dx, dd, count = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65, 65] and not any(count.values())
    on_ball = f[:, 0] < 2
    assert np.max(np.abs(dx[0][on_ball] - (f[on_ball, 9:12] - case.source))) <= 32 * EPS
    assert np.nanmax(np.abs(dd[0])) <= 32 * EPS
    last, exit_ = f[f[:, 0] == 2], f[f[:, 0] == 1]
    assert np.array_equal(last[:, 4], exit_[:, 4])
    d, a, shift = last[:, 12:15], np.array([1.0, 0.0, 0.0]), exit_[:, 9:12] - case.source
    want = shift - d * ((shift @ a) / (d @ a))[:, None]
    assert np.max(np.abs(dx[0][f[:, 0] == 2] - want)) <= 64 * EPS * np.max(np.abs(want))


def test_reference_tilted_plate_index_and_thickness():
    case = cases.build("plate", 65)
    dx, _, count = reference_of(case)
    assert case.counts == [65, 65, 65] and not any(count.values())
    t, angle, n = cases.PLATE.thickness, np.radians(cases.PLATE.angle), cases.PLATE.index
    s, c = np.sin(angle), np.cos(angle)
    shift = t * s * (1 - c / np.sqrt(n * n - s * s))
    by_index = t * s * c * n * (n * n - s * s) ** -1.5
    at = case.frame[:, 5] == case.surface.get_id()
    moved = case.frame[at, 10] - case.rays[1, case.frame[at, 4].astype(int)]
    assert np.max(np.abs(moved - shift)) <= 16 * EPS  # (the oracle's own trace shows the closed form's displacement, towards +y)
    for k, want in ((0, by_index), (1, shift)):  # (d/dn; t d/dt, and the displacement is linear in t)
        got = dx[k][at].astype(float)
        assert np.max(np.abs(got - [0.0, want, 0.0])) <= 32 * EPS, (k, got[0], want)


def test_reference_parabolic_mirror_whose_focus_grows():
    case = cases.build("dish_focus", 65)
    dx, _, count = reference_of(case)
    assert case.counts == [65, 65] and count["n_reflections"] == 65 and not count["n_unfit"] and not count["n_invalid"]
    at = case.frame[:, 5] == case.surface.get_id()
    assert at.sum() == 65
    d = case.frame[at, 12:15]
    a = np.asarray(case.parts[1].get_orientation(), dtype=float).reshape(-1)[:3]
    assert abs(a @ case.axis) < 0.99  # (the detector is tilted: a is not the axis)
    want = case.axis - d * ((case.axis @ a) / (d @ a))[:, None]
    assert np.max(np.abs(dx[0][at] - want)) <= 32 * EPS


# ---- the reference against central differences of the oracle's traces ------------------------------------------------------
def difference(case, k, h):
    """D(h) (R, 3) of the landing points by central differences of the oracle's traces, and whether each row kept its path."""
    plus = cases.build(case.name, case.rays.shape[1], change=(k, h))
    minus = cases.build(case.name, case.rays.shape[1], change=(k, -h))
    if plus.counts != case.counts or minus.counts != case.counts:
        return None, np.zeros(len(case.frame), dtype=bool)

    def rank(frame):  # (a system built afresh draws new surface ids: compare the sequences through the order of the ids)
        return np.searchsorted(np.unique(frame[:, 5]), frame[:, 5])

    keep = (rank(plus.frame) == rank(case.frame)) & (rank(minus.frame) == rank(case.frame))
    keep &= (plus.frame[:, 4] == case.frame[:, 4]) & (minus.frame[:, 4] == case.frame[:, 4])
    return (plus.frame[:, 9:12] - minus.frame[:, 9:12]) / (2 * h), keep


@pytest.mark.parametrize("name, k", cases.DIFFERENCED)
def test_reference_against_central_differences_of_the_oracle(name, k):
    case = cases.build(name, 257)
    dx, _, count = reference_of(case)
    assert not any(count[key] for key in ("n_unknown", "n_invalid", "n_unfit")) and case.counts[0] == 257
    assert all(c == 257 for c in case.counts)
    # h from the oracle alone: the smallest power of four at which its own Richardson estimate is still truncation, not
    # rounding (the median of (4/3) |D(h) - D(h/2)| over the moving elements at least ten times the rounding floor)
    scale = np.max(np.abs(case.frame[:, 9:12]))
    chosen = None
    for exponent in range(-12, -1):
        h = 4.0 ** exponent
        coarse, keep_coarse = difference(case, k, h)
        fine, keep_fine = difference(case, k, h / 2)
        keep = keep_coarse & keep_fine
        assert keep.all(), f"h = 4^{exponent}: {np.sum(~keep)} rows changed their path"  # (the share left out is zero)
        floor = 4 * EPS * scale / h
        estimate = (4.0 / 3.0) * np.abs(coarse - fine)
        if np.any(estimate > 0) and np.median(estimate[estimate > 0]) >= 10 * floor:
            chosen = (h, fine, estimate, floor)
            break
    assert chosen is not None, "the oracle's differences never rose above their rounding floor"
    h, fine, estimate, floor = chosen
    bound = estimate + floor
    error = np.abs(dx[k].astype(float) - fine)
    print(f"{name} parameter {k}: h = 2^{int(np.log2(h))}, max |dx| {np.abs(fine).max():.3e}, max error {error.max():.3e}, "
          f"max bound {bound.max():.3e}, worst error / bound {np.max(error / bound):.3f}")
    assert np.abs(fine).max() > 1e-3
    assert np.all(error <= bound), float(np.max(error / bound))
