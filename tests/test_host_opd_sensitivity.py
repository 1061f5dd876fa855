"""Wavefront sensitivities, the part that needs no GPU: the numpy longdouble reference (tests/opd_sensitivity_reference.py)
against closed forms, against identities that hold by construction, and against Richardson-checked central differences of
the C oracle's own traces of the changed system, whose OPD the reference evaluates against the FIXED sphere (P, R, pivot,
pupil radius) of the unchanged one.  Nothing here touches the device."""
import numpy as np
import pytest

import design_reference as dref
import opd_scenes as cases
import opd_sensitivity_reference as ref

EPS = np.finfo(np.float64).eps


def solve(case, rows=None, **sphere):
    from pyrayt_amd.scene import SceneSnapshot

    table = dref.table_of(SceneSnapshot(case.parts).prims)
    tangents = ref.trace(case.frame, table, [dref.parameter(m) for m in case.parameters])
    assert not any(tangents["count"][key] for key in ("n_unknown", "n_invalid", "n_unfit"))
    if rows is None:
        rows = np.flatnonzero(case.frame[:, 5] == case.surface.get_id())
    ball = ref.default_sphere(case.frame, rows, **sphere)
    wave = ref.wavefront(case.frame, rows, tangents, ball)
    wave["dx"] = tangents["dx"][:, rows]
    return rows, ball, wave


def test_detector_move_changes_nothing_on_a_fixed_sphere():
    case = cases.build("detector_move", 65)
    rows, ball, wave = solve(case)
    assert len(rows) == 65 and np.all(wave["met"])
    dx = np.max(np.abs(wave["dx"].astype(float)))
    assert dx > 0.1  # (the landing points do move)
    # only Q slides along the ray: what is left is the recorded direction's own departure from a unit vector (float64)
    assert np.max(np.abs(wave["dfield"])) <= 8 * EPS * dx
    assert np.max(np.abs(wave["dopd"])) <= 16 * EPS * dx
    assert np.max(np.abs(wave["dpupil"])) <= 16 * EPS * dx / float(ball["pupil_radius"])


def test_plate_index_and_thickness():
    case = cases.build("plate_square", 65)
    rows, ball, wave = solve(case)
    glass = case.frame[case.frame[:, 0] == 1]
    assert np.all(glass[:, 3] == cases.PLATE["index"]) and np.array_equal(glass[:, 4], case.frame[rows, 4])
    length = np.sqrt(np.sum((glass[:, 9:12] - glass[:, 6:9]) ** 2, axis=1))
    assert abs(length[0] - (cases.PLATE["thickness"] - 1e-6)) < 4 * EPS
    assert np.max(np.abs(wave["dfield"][0] - length)) <= 8 * EPS  # (the index: the glass segment's recorded length)
    # the thickness, per unit of relative elongation: (n_glass - n_air) t
    want = (cases.PLATE["index"] - 1.0) * cases.PLATE["thickness"]
    assert np.max(np.abs(wave["dfield"][1] - want)) <= 8 * EPS
    assert np.max(np.abs(wave["dpupil"])) <= 8 * EPS and np.max(np.abs(wave["dopd"] - wave["dfield"])) <= 8 * EPS


def test_flat_mirror_pushed_away_lengthens_the_path_by_two():
    case = cases.build("mirror_normal", 65)
    rows, ball, wave = solve(case)
    assert np.all(case.frame[rows, 3] == 1.0)
    assert np.max(np.abs(wave["dfield"][0] - 2.0)) <= 8 * EPS  # (+: the mirror moves along the incoming rays)


def closed_form_dish(pupil, ball):
    """The mirror moved by the unit vector e moves the focus, and the spherical wave about it, by e: at the fixed sphere's
    point E the wavefront changes by n e.(E - P) / R (E lies upstream of the focus), and the plane wave, which comes along
    -x, meets the mirror sooner by n e.x."""
    sin = pupil * float(ball["pupil_radius"]) / float(ball["R"])
    cos = np.sqrt(1 - np.sum(sin * sin, axis=1))
    return -(1 + cos), sin[:, 0]  # (e = x: E - P = R (-cos, sin); e = y: e1 = y)


def test_parabolic_mirror_axial_and_lateral_translation():
    case = cases.build("dish_axial", 257)
    rows, ball, wave = solve(case, P=(0.0, 0.0, 0.0))
    assert len(rows) == 257 and np.all(wave["met"])
    path = 2.0 + 2 * cases.DISH["focus"]
    assert np.max(np.abs(wave["opd"])) <= 8 * EPS * path  # (stigmatic: the nominal OPD is zero)
    assert np.max(np.abs(wave["dopd"] - wave["dfield"])) <= 64 * EPS  # (u is along E - P and dE is tangent)
    pupil = wave["pupil"].astype(float)
    axial, lateral = closed_form_dish(pupil, ball)
    assert np.max(np.abs(wave["dfield"][0] - axial)) <= 64 * EPS and np.max(np.abs(wave["dfield"][1] - lateral)) <= 64 * EPS
    J = 15
    total = ref.sums(wave, np.ones(len(rows)), J)
    zwz = total["zwz"].astype(float)
    rounding = np.linalg.cond(zwz) * EPS  # (of the float64 solve, relative to the largest coefficient)
    a = ref.fit(zwz, total["z_dfield"][0])
    na = cases.DISH["beam"] / cases.DISH["focus"]
    assert abs(a[0] + 2) < na * na and 0 < a[3] < na * na  # (-(1 + cos): piston -2 and a defocus of about NA^2 / (4 sqrt 3))
    assert abs(a[3] - na * na * (float(ball["pupil_radius"]) / cases.DISH["beam"]) ** 2 / (4 * np.sqrt(3))) < 1e-3 * a[3]
    others = np.delete(a, [0, 3])
    print(f"axial: piston {a[0]:.6f} defocus {a[3]:.3e} others {np.abs(others).max():.3e}, bound {2 * rounding + na ** 4:.3e}")
    assert np.max(np.abs(others)) <= 2 * rounding + na ** 4  # (cos's fourth-order term: NA^4 / 8 at most)
    b = ref.fit(zwz, total["z_dfield"][1])
    tilt = float(ball["pupil_radius"]) / float(ball["R"]) / 2  # (sin_y = (pr / R) rho cos(theta), Z2 = 2 rho cos(theta))
    print(f"lateral: Z2 {b[1]:.6e} (closed form {tilt:.6e}), others {np.abs(np.delete(b, 1)).max():.3e}, bound {tilt * rounding:.3e}")
    assert abs(b[1] - tilt) <= tilt * rounding + 64 * EPS and np.max(np.abs(np.delete(b, 1))) <= tilt * rounding + 64 * EPS
    # ... and central differences of the reference's own Zernike fit of the oracle's re-traced frames
    for k, coefficients in ((0, a), (1, b)):
        def fitted(h):
            changed = cases.build("dish_axial", 257, change=(k, h))
            assert changed.counts == case.counts and np.array_equal(changed.frame[:, 4], case.frame[:, 4])
            opd, at = ref.opd_of(changed.frame, rows, ball)
            z = ref.zernike(J, at[:, 0], at[:, 1])
            return ref.fit(np.einsum("in,jn->ij", z, z), z @ opd)
        h = 2.0 ** -14
        coarse, fine = (fitted(h) - fitted(-h)) / (2 * h), (fitted(h / 2) - fitted(-h / 2)) / h
        bound = (4.0 / 3.0) * np.abs(coarse - fine) + 4 * EPS * path * np.linalg.cond(zwz) / h
        error = np.abs(coefficients - fine)
        print(f"parameter {k}: max error {error.max():.3e}, worst error / bound {np.max(error / bound):.3f}")
        assert np.all(error <= bound)


def differences(case, rows, ball, k, h):
    """Central differences of the OPD (n,), the pupil point (n, 2) and the weighted RMS OPD of the oracle's traces."""
    out = []
    for amount in (h, -h):
        changed = cases.build(case.name, case.rays_per_source or case.rays.shape[1], change=(k, amount))
        same = changed.counts == case.counts and np.array_equal(changed.frame[:, 4], case.frame[:, 4])
        rank = lambda f: np.searchsorted(np.unique(f[:, 5]), f[:, 5])  # noqa: E731 (a system built afresh draws new ids)
        assert same and np.array_equal(rank(changed.frame), rank(case.frame)), "a ray changed its path"
        opd, pupil = ref.opd_of(changed.frame, rows, ball)
        w = changed.frame[rows, 1].astype(ref.LD)
        mean = (w * opd).sum() / w.sum()
        out.append((opd, pupil, np.sqrt((w * (opd - mean) ** 2).sum() / w.sum())))
    return tuple((out[0][q] - out[1][q]) / (2 * h) for q in range(3))


def groups_of(case):
    at = np.flatnonzero(case.frame[:, 5] == case.surface.get_id())
    if not case.rays_per_source:
        return [at]
    return [at[case.frame[at, 4] // case.rays_per_source == g] for g in range(2)]


@pytest.mark.parametrize("name, k", [("singlet", k) for k in range(5)] + [("two_fields", k) for k in (0, 1, 2, 3, 4)])
def test_reference_against_central_differences_of_the_oracle(name, k):
    case = cases.build(name, 129)
    for g, rows in enumerate(groups_of(case)):
        rows, ball, wave = solve(case, rows)
        assert len(rows) == 129 and np.all(wave["met"]) and np.all(wave["followed"])  # (the share left out is zero)
        total = ref.sums(wave, case.frame[rows, 1], 4)
        gradient = ref.statistics(total)["rms_gradient"][k]
        # h from the oracle alone, as tests/test_host_design_sensitivity.py chooses it
        scale = float(np.max(np.abs(ref.optical_path(case.frame))))
        chosen = None
        for exponent in range(-12, -1):
            h = 4.0 ** exponent
            coarse, fine = differences(case, rows, ball, k, h), differences(case, rows, ball, k, h / 2)
            floor = 4 * EPS * scale / h
            estimate = (4.0 / 3.0) * np.abs(coarse[0] - fine[0]).astype(float)
            if np.any(estimate > 0) and np.median(estimate[estimate > 0]) >= 10 * floor:
                chosen = (h, coarse, fine, floor)
                break
        assert chosen is not None, "the oracle's differences never rose above their rounding floor"
        h, coarse, fine, floor = chosen
        reach = float(np.max(np.abs(case.frame[rows, 9:12]))) / float(ball["pupil_radius"])
        for what, got, q, low in (("dopd", wave["dopd"][k], 0, floor), ("dpupil", wave["dpupil"][k].T, 1, 4 * EPS * reach / h),
                                  ("rms gradient", gradient, 2, floor)):
            bound = (4.0 / 3.0) * np.abs(coarse[q] - fine[q]).astype(float) + low
            error = np.abs((got - fine[q]).astype(float))
            print(f"{name} group {g} parameter {k} {what}: h = 2^{int(np.log2(h))}, max |value| {np.max(np.abs(fine[q])):.3e}, "
                  f"max error {np.max(error):.3e}, worst error / bound {np.max(error / bound):.3f}")
            assert np.all(error <= bound), (what, float(np.max(error / bound)))
        assert np.max(np.abs(fine[0])) > 1e-4


def test_identities_that_hold_by_construction():
    case = cases.build("two_fields", 129)
    for rows in groups_of(case):
        rows, ball, wave = solve(case, rows)
        # dopd - dfield == n u.dE
        lift = wave["n"] * np.sum(ref.sref._unit(wave["u"]) * wave["dE"], axis=2)
        assert np.max(np.abs((wave["dopd"] - wave["dfield"]) - lift)) <= 4 * np.finfo(ref.LD).eps * np.max(np.abs(wave["dopd"]))
        # dE is tangent to the sphere
        ep = ref.extend(case.frame, rows, ball["P"], ball["R"])[1] - ball["P"]
        assert np.max(np.abs(np.sum(ep * wave["dE"], axis=2))) <= 64 * np.finfo(ref.LD).eps
        # a reference that follows the centroid: the fixed one minus n (u.dP_k), in the right-hand sides as in the rows
        w = case.frame[rows, 1].astype(ref.LD)
        total = ref.sums(wave, w, 15)
        dx = wave["dx"]
        dP = np.einsum("n,knc->kc", w, dx) / w.sum()
        follow = dict(wave, dfield=wave["dfield"] - np.einsum("nc,kc->kn", wave["n"][:, None] * wave["u"], dP))
        moved = ref.sums(follow, w, 15)["z_dfield"]
        want = total["z_dfield"] - np.einsum("kc,cj->kj", dP, total["z_nu"])
        assert np.max(np.abs(moved - want)) <= 64 * np.finfo(ref.LD).eps * np.max(np.abs(total["z_dfield"]))
        assert np.max(np.abs(dP)) > 0.1  # (the centroid does move)
