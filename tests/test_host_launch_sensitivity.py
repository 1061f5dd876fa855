"""Launch and wavelength sensitivities of the frame, the parts that need no GPU: the refusals of SourceMotion and
WavelengthChange, the ABI surface, the numpy longdouble reference (tests/launch_reference.py) against closed forms and the
Lagrange invariant, and the reference against Richardson-checked central differences of the C oracle's own re-traces with
the rays transformed in numpy and the wavelengths shifted (tests/launch_scenes.py ``retrace``): landing points, slopes, the
OPD against the fixed sphere and the best-focus shift.

Tolerances of the closed forms.  Reference and closed form read the same float64 frame, whose landing points and
directions are rounded to EPS = 2^-52 relative; what differs is how each carries that rounding.  A landing point off its
surface by EPS |x| moves a normal by kappa EPS |x| and a later landing point by that times the path behind it: with
curvatures <= 1, |x| <= 6 and paths <= 6 a bound of 64 EPS times the magnitude of the expected value (at least 1) holds
for flat and singly curved scenes, and the rigid-invariance scene, which goes through two spheres and sums three
tangents, is held to the 1e-13 of tests/test_host_sensitivity.py's invariances.  The prism's expected value is built from
differences of recorded directions (n d_glass - d_in, of length 0.5): 256 EPS."""
import os

import numpy as np
import pytest

import launch_reference as ref
import launch_scenes as cases
import opd_sensitivity_reference as oref

EPS = np.finfo(np.float64).eps
LD = ref.LD


def reference_of(case, parameters=None, frame=None, info=None):
    from pyrayt_amd.scene import SceneSnapshot

    snapshot = SceneSnapshot(case.parts)
    parameters = case.parameters if parameters is None else parameters
    return ref.trace(case.frame if frame is None else frame, ref.table_of(snapshot.prims),
                     [ref.parameter(m) for m in parameters], ref.glasses_of(snapshot), info)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bk7_dispersion(wavelength):
    import pyrayt_amd as prt
    from pyrayt_amd.scene import SceneSnapshot

    coef = SceneSnapshot([prt.g3d.Sphere(1, material=prt.materials.glass["BK7"])]).materials[0]["coef"]
    dndl, n = ref.dispersion(coef, wavelength)
    return float(dndl), float(n)


# ---- refusals and the ABI ------------------------------------------------------------------------------------------------------
def test_source_motion_and_wavelength_change_refuse_bad_input():
    from pyrayt_amd import SourceMotion, WavelengthChange

    for wrong in ((1,), (0, 0), (-1, 5), (0.5, 3), (0, 2.5), "all", (1, 2, 3), 7):
        with pytest.raises(ValueError, match="rays"):
            SourceMotion(wrong)
        with pytest.raises(ValueError, match="rays"):
            WavelengthChange(wrong)
    for name in ("translate", "rotate", "pivot"):
        for wrong in ((0, np.nan, 0), (1, 2), "up"):
            with pytest.raises(ValueError, match=name):
                SourceMotion(None, **{name: wrong})
    for wrong in (np.nan, np.inf, "fast"):
        with pytest.raises(ValueError, match="rate"):
            WavelengthChange(rate=wrong)
    for wrong in (-1, 0.5, "first"):
        with pytest.raises(ValueError, match="index"):
            SourceMotion.of_source(wrong, 10)
    for wrong in (0, -3, 2.5):
        with pytest.raises(ValueError, match="rays_per_source"):
            SourceMotion.of_source(1, wrong)
    one = SourceMotion.of_source(2, 65, rotate=(0, 0, 1))
    assert one.id_range == (130.0, 195.0) and one.rays == (130, 65) and one.surface_ids == ()
    assert SourceMotion().id_range == (-np.inf, np.inf) and WavelengthChange((3, 4)).id_range == (3.0, 7.0)
    assert "SourceMotion" in repr(one) and "rays=(130, 65)" in repr(one) and "rate=-2.0" in repr(WavelengthChange(rate=-2))
    late = SourceMotion.of_source(1, translate=(0, 1, 0))
    assert late.id_range is None and late.resolved(10).id_range == (10.0, 20.0)
    assert np.array_equal(late.resolved(10).translate, (0, 1, 0))
    with pytest.raises(ValueError, match="rays_per_source"):
        late.resolved(None)


def test_sensitivity_refuses_a_bad_launch_mix_before_it_needs_a_device():
    torch = pytest.importorskip("torch")
    import scenes
    from pyrayt_amd import Motion, SourceMotion, WavelengthChange
    from pyrayt_amd.frame import DeviceFrame

    case = cases.build("cone", 16)
    frame = DeviceFrame(torch.from_numpy(np.ascontiguousarray(case.frame.T)), case.counts)
    lens, det = case.parts
    mix = [SourceMotion(None, translate=(0, 1, 0)), WavelengthChange(), Motion(det, translate=(1, 0, 0))]
    with pytest.raises(ValueError, match="16"):
        frame.sensitivity(det, mix * 6, case.parts)
    with pytest.raises(ValueError, match="SourceMotion"):
        frame.sensitivity(det, [mix[0], (0, 16)], case.parts)
    with pytest.raises(ValueError, match="rays_per_source"):
        frame.sensitivity(det, [SourceMotion.of_source(0, translate=(0, 1, 0))], case.parts)
    table_parts, _ = scenes.custom_cauchy(scenes.product_api(), 4)
    with pytest.raises(ValueError, match="table glass"):
        frame.sensitivity(table_parts[1], [mix[0], WavelengthChange()], table_parts)
    # a record plan that left the wavelength out cannot serve a WavelengthChange
    from pyrayt_amd.frame import _PATH_COLUMNS

    from pyrayt_amd.frame import COLUMNS

    lean = DeviceFrame(torch.from_numpy(np.ascontiguousarray(case.frame.T)), case.counts,
                       columns=[COLUMNS.index(name) for name in tuple(_PATH_COLUMNS) + ("intensity",)])
    with pytest.raises(ValueError, match="wavelength"):
        lean.sensitivity(det, [WavelengthChange()], case.parts)


def test_the_library_exports_the_entry_point_and_the_binding_declares_it():
    from pyrayt_amd import engine

    names = ("prt_frame_launch_sensitivity", "prt_frame_launch_sensitivity_workspace_bytes")
    assert all(name in engine.EXPORTED_SYMBOLS for name in names)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "prt.h")).read()
    assert all(f" {name}(" in header for name in names)
    import ctypes

    lib = ctypes.CDLL(engine.LIB_PATH)
    assert all(hasattr(lib, name) for name in names)
    declared = engine.library()
    assert declared.prt_frame_launch_sensitivity.argtypes is not None and len(declared.prt_frame_launch_sensitivity.argtypes) == 45
    size = declared.prt_frame_launch_sensitivity_workspace_bytes
    assert size(195, 4, 16, 3, 65, 0) > 0 and size(195, 4, 16, 3, 65, 15) > size(195, 4, 16, 3, 65, 0)
    assert size(195, 4, 17, 3, 65, 0) < 0 and size(195, 4, 16, 3, 65, 37) < 0
    # the dispersion table is what the launch form adds to the wavefront form's workspace
    assert 0 <= size(195, 4, 16, 3, 65, 15) - declared.prt_frame_opd_sensitivity_workspace_bytes(195, 4, 16, 3, 65, 15) - 4 * 56 <= 8


# ---- the reference against closed forms -------------------------------------------------------------------------------------
def test_reference_rigid_invariance_of_source_and_system_together():
    case = cases.build("invariance", 65)
    out = reference_of(case)
    assert case.counts == [65, 65, 65] and not any(out["count"].values())
    f = case.frame
    v, w, c = (np.array(t) for t in (cases.TWIST.v, cases.TWIST.w, cases.TWIST.c))
    dx, dd, dL = (out[name].astype(float).sum(axis=0) for name in ("dx", "dd", "dL"))
    want_x = v + np.cross(w, f[:, 9:12] - c)
    want_d = np.cross(w, unit(f[:, 12:15]))
    print(f"invariance: max |dx - rigid| {np.abs(dx - want_x).max():.3e}, |dd - w x d| {np.abs(dd - want_d).max():.3e}, "
          f"|dL| {np.abs(dL).max():.3e}")
    assert np.abs(want_x).max() > 0.3 and np.abs(out["dL"][0].astype(float)).max() > 0.1  # (each part alone does change the path)
    assert np.abs(dx - want_x).max() <= 1e-13 and np.abs(dd - want_d).max() <= 1e-13 and np.abs(dL).max() <= 1e-13


def test_reference_source_turned_about_its_apex_in_free_space():
    case = cases.build("free_space", 65)
    out = reference_of(case)
    f = case.frame
    assert case.counts == [65] and not any(out["count"].values())
    n = np.asarray(case.parts[0].get_orientation(), dtype=float).reshape(-1)[:3]
    d = unit(f[:, 12:15])
    t = np.linalg.norm(f[:, 9:12] - case.apex, axis=1)
    turned = np.cross(case.w, d)
    want = t[:, None] * (turned - d * ((turned @ n) / (d @ n))[:, None])
    assert np.abs(want).max() > 1.0
    assert np.abs(out["dx"][0].astype(float) - want).max() <= 64 * EPS * np.abs(want).max()
    assert np.abs(out["dd"][0].astype(float) - turned).max() <= 8 * EPS


def test_reference_translated_source_before_a_flat_mirror():
    case = cases.build("flat_mirror", 65)
    out = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65] and out["count"]["n_reflections"] == 65
    m = np.asarray(case.mirror.get_orientation(), dtype=float).reshape(-1)[:3]
    a = np.asarray(case.parts[1].get_orientation(), dtype=float).reshape(-1)[:3]
    d = unit(f[:, 12:15])
    first, last = f[:, 0] == 0, f[:, 0] == 1
    on_mirror = case.v - d[first] * ((case.v @ m) / (d[first] @ m))[:, None]
    mirrored = case.v - 2 * m * (m @ case.v)
    on_detector = mirrored - d[last] * ((mirrored @ a) / (d[last] @ a))[:, None]
    dx = out["dx"][0].astype(float)
    assert np.abs(dx[first] - on_mirror).max() <= 64 * EPS and np.abs(dx[last] - on_detector).max() <= 64 * EPS
    assert np.abs(out["dd"][0].astype(float)).max() <= 8 * EPS


def test_reference_tilted_collimated_beam_on_a_parabolic_mirror():
    """The beam's direction (-1, 0, 0) turned by theta about z through the vertex is (-1, -theta, 0); the vertex ray comes
    back along (1, -theta, 0) and meets the focal plane, f away, at y = -f tan(theta)."""
    case = cases.build("parabola", 65)
    out = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65] and out["count"]["n_reflections"] == 65
    vertex_ray = (f[:, 4] == 0) & (f[:, 0] == 1)
    assert vertex_ray.sum() == 1 and np.allclose(f[(f[:, 4] == 0) & (f[:, 0] == 0), 9:12], cases.PARABOLA.vertex, atol=1e-15)
    dx = out["dx"][0][vertex_ray][0].astype(float)
    print(f"parabola: d(landing point)/d(theta) of the vertex ray {dx}")
    assert np.abs(dx - [0.0, -cases.PARABOLA.focus, 0.0]).max() <= 64 * EPS * cases.PARABOLA.focus
    # the other rays show the mirror's coma, which is linear in theta: they differ from f, by less than (r / 2f)^2 f
    others = out["dx"][0][f[:, 0] == 1].astype(float)
    assert np.abs(others[:, 1] + cases.PARABOLA.focus).max() > 1e-3
    assert np.abs(np.linalg.norm(others, axis=1) - cases.PARABOLA.focus).max() < 3 * (0.6 / 6.0) ** 2 * cases.PARABOLA.focus


def test_reference_tilted_plate_in_bk7_follows_the_wavelength_through_the_index():
    case = cases.build("plate", 65)
    out = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65, 65] and not any(out["count"].values())
    dndl, n = bk7_dispersion(0.55)
    assert np.all(f[f[:, 0] == 1, 3] == n) and -0.06 < dndl < -0.04  # (the trace's own index; BK7 near 0.55 um)
    t, angle = cases.PLATE.thickness, np.radians(cases.PLATE.angle)
    s, c = np.sin(angle), np.cos(angle)
    by_index = t * s * c * n * (n * n - s * s) ** -1.5
    last, inside = f[:, 0] == 2, f[:, 0] == 1
    dx = out["dx"][0].astype(float)
    assert np.abs(dx[last] - [0.0, by_index * dndl, 0.0]).max() <= 64 * EPS
    # the optical path: by Fermat the whole derivative is (the recorded length in the glass) dn/dlambda on the detector; on
    # the exit face it is that plus the geometric term n d.dx = -t s^2 / (n^2 cos^3 theta_t) dn/dlambda
    length = np.linalg.norm(f[inside, 9:12] - f[inside, 6:9], axis=1)
    cos_t = np.sqrt(1 - s * s / (n * n))
    assert np.abs(length - (t / cos_t - 1e-6)).max() <= 16 * EPS
    dL = out["dL"][0].astype(float)
    assert np.abs(dL[last] - length * dndl).max() <= 64 * EPS
    assert np.abs(dL[inside] - (length * dndl - t * s * s / (n * n * cos_t ** 3) * dndl)).max() <= 64 * EPS
    assert np.abs(out["dnu"][0][inside].astype(float) - dndl).max() <= EPS and not out["dnu"][0][last].any()


def test_reference_a_basic_refractor_has_no_dispersion():
    case = cases.build("plate_constant", 65)
    out = reference_of(case)
    assert case.counts == [65, 65, 65] and not any(out["count"].values())
    for name in ("dx", "dd", "dL", "dnu"):
        assert not out[name].any(), name


def test_reference_prism_dispersion_is_the_closed_form_of_the_deviation():
    case = cases.build("prism", 65)
    out = reference_of(case)
    f = case.frame
    assert case.counts == [65, 65, 65] and not any(out["count"].values())
    dndl, n = bk7_dispersion(0.55)
    d_in, d_glass, d_out = (unit(f[f[:, 0] == g, 12:15]) for g in range(3))
    assert all(np.array_equal(f[f[:, 0] == g, 4], np.arange(65)) for g in range(3)) and np.all(f[f[:, 0] == 1, 3] == n)
    n1, n2 = unit(n * d_glass - d_in), unit(d_out - n * d_glass)
    cos1, cos2 = np.abs(np.sum(d_glass * n1, axis=1)), np.abs(np.sum(d_out * n2, axis=1))
    apex = np.linalg.norm(np.cross(n1, n2), axis=1)
    assert np.abs(apex - np.sin(np.radians(60))).max() <= 64 * EPS
    axis = unit(np.cross(d_in, d_out))  # (the deviation turns d_in towards d_out about it)
    want = (apex / (cos1 * cos2) * dndl)[:, None] * np.cross(axis, d_out)
    got = out["dd"][0][f[:, 0] == 2].astype(float)
    print(f"prism: d(deviation)/d(lambda) {np.linalg.norm(want, axis=1).min():.4f} to {np.linalg.norm(want, axis=1).max():.4f} "
          f"rad/um, max error {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 256 * EPS * np.abs(want).max()


@pytest.mark.parametrize("name, pairs", [("fields", ((0, 2), (1, 3), (0, 15), (10, 15))), ("two_mirrors", ((0, 1), (2, 3), (1, 2)))])
def test_reference_lagrange_invariant_is_kept_along_every_ray(name, pairs):
    """n (dx_a.dd_b - dx_b.dd_a) of two launch parameters is the same at every row of a ray as at its launch, where it is
    do_a.dd_b - do_b.dd_a in the ambient index 1: free flight, the 1e-6 relaunch, refraction and reflection at surfaces that
    do not move are symplectic.  Bound: the reference works in longdouble on a float64 frame, so a row's recorded direction
    is not to the bit the one its own interface gives (d'.dd' is EPS |dd'|, not 0), and its landing point is EPS |x| off its
    surface; each of those enters a row's terms a few times, scaled by 1 / |n.d| in the landing.  With 64 such roundings a
    row, the invariant may drift by 64 EPS (1 + 1 / |n.d|) n (|dx_a| |dd_b| + |dx_b| |dd_a| + |do_a| |dd_b| + |do_b| |dd_a|)
    per row, summed along the ray."""
    case = cases.build(name, 65)
    info = {}
    out = reference_of(case, info=info)
    f = case.frame
    assert len(case.counts) >= 3 and not any(out["count"][key] for key in ("n_unknown", "n_invalid", "n_unfit"))
    if name == "two_mirrors":
        assert out["count"]["n_reflections"] > 200
    d = unit(f[:, 12:15])
    worst = 0.0
    for a, b in pairs:
        pa, pb = (ref.parameter(case.parameters[k]) for k in (a, b))
        first = f[:, 0] == 0
        launch = {}
        for par, key in ((pa, "a"), (pb, "b")):
            on = ((f[:, 4] >= par["lo"]) & (f[:, 4] < par["hi"]))[:, None]
            launch[key] = (np.where(on, par["v"] + np.cross(par["w"], f[:, 6:9] - par["c"]), 0.0), np.where(on, np.cross(par["w"], d), 0.0))
        at_launch = np.sum(launch["a"][0] * launch["b"][1] - launch["b"][0] * launch["a"][1], axis=1)
        by_id = dict(zip(f[first, 4], at_launch[first]))
        dxa, dxb, dda, ddb = (out[key][k] for key, k in (("dx", a), ("dx", b), ("dd", a), ("dd", b)))
        value = (f[:, 3] * np.sum(dxa * ddb - dxb * dda, axis=1)).astype(float)
        norm = lambda v: np.sqrt(np.sum(np.asarray(v, dtype=float) ** 2, axis=1))  # noqa: E731
        size = f[:, 3] * (norm(dxa) * norm(ddb) + norm(dxb) * norm(dda))
        size_launch = {i: s for i, s in zip(f[first, 4], (norm(launch["a"][0]) * norm(launch["b"][1])
                                                           + norm(launch["b"][0]) * norm(launch["a"][1]))[first])}
        drift = 64 * EPS * (1 + 1 / np.abs(info["nd"])) * (size + np.array([size_launch[i] for i in f[:, 4]]))
        bound = np.zeros(len(f))
        for r in range(len(f)):  # (generation-major: a ray's previous row is already done)
            p = info["previous"][r]
            bound[r] = drift[r] + (bound[p] if p >= 0 else 0.0)
        want = np.array([by_id[i] for i in f[:, 4]])
        assert np.abs(want).max() > 1e-3, (a, b)  # (the pair does have an invariant to keep)
        ratio = np.max(np.abs(value - want)[bound > 0] / bound[bound > 0])
        worst = max(worst, ratio)
        assert np.all(np.abs(value - want) <= bound), (a, b, float(ratio))
    print(f"{name}: Lagrange invariant, {len(pairs)} pairs, worst drift / bound {worst:.4f}")


# ---- the reference against central differences of the oracle's re-traces ---------------------------------------------------
_RETRACED = {}


def retraced(case, k, h):
    key = (case.name, case.rays.shape[1], k, h)
    if key not in _RETRACED:
        _RETRACED[key] = cases.retrace(case, k, h)
    return _RETRACED[key]


def richardson(case, k, measure, floor_of, what):
    """D(h / 2) of ``measure(frame_plus, frame_minus, h)`` at the first h = 4^e at which the oracle's own Richardson
    estimate (4/3 |D(h) - D(h/2)|) is truncation and not rounding (its median at least ten times ``floor_of(h)``), with the
    bound estimate + floor: test_host_design_sensitivity.py's rule, from the two step sizes' disagreement alone."""
    for exponent in range(-12, -1):
        h = 4.0 ** exponent
        values = []
        for step in (h, h / 2):
            (plus, counts_plus), (minus, counts_minus) = retraced(case, k, step), retraced(case, k, -step)
            assert counts_plus == case.counts and counts_minus == case.counts, f"h = 4^{exponent}: rays changed their path"
            for other in (plus, minus):
                assert np.array_equal(other[:, 4], case.frame[:, 4]) and np.array_equal(other[:, 5], case.frame[:, 5])
            values.append(measure(plus, minus, step))
        coarse, fine = values
        floor = floor_of(h)
        estimate = (4.0 / 3.0) * np.abs(coarse - fine)
        if np.any(estimate > 0) and np.median(estimate[estimate > 0]) >= 10 * np.median(floor):
            return h, fine, estimate + floor
    raise AssertionError(f"{what}: the oracle's differences never rose above their rounding floor")


@pytest.mark.parametrize("name, k", cases.DIFFERENCED)
def test_reference_against_central_differences_of_the_oracle(name, k):
    case = cases.build(name, 65)
    out = reference_of(case)
    f = case.frame
    assert not any(out["count"][key] for key in ("n_unknown", "n_invalid", "n_unfit"))
    rows = np.flatnonzero(f[:, 5] == case.surface.get_id())
    rows = rows[f[rows, 0] == f[rows, 0].max()] if name == "two_mirrors" else rows
    scale = np.max(np.abs(f[:, 9:12]))
    report = []

    def held(what, analytic, measure, floor_of, moving=None):
        h, fine, bound = richardson(case, k, measure, floor_of, what)
        error = np.abs(np.asarray(analytic, dtype=float) - fine)
        report.append(f"{what} h = 2^{int(np.log2(h))} max |D| {np.abs(fine).max():.3e} error {error.max():.3e} "
                      f"bound {bound.max():.3e} ratio {np.max(error / bound):.3f}")
        if moving is not None:
            assert np.abs(fine).max() > moving, what
        assert np.all(error <= bound), (what, float(np.max(error / bound)))

    try:
        # landing points and slopes of every row
        held("dx", out["dx"][k], lambda p, m, h: (p[:, 9:12] - m[:, 9:12]) / (2 * h), lambda h: 4 * EPS * scale / h, 1e-3)
        held("dd", out["dd"][k], lambda p, m, h: (unit(p[:, 12:15]) - unit(m[:, 12:15])) / (2 * h), lambda h: 4 * EPS / h)
        # the OPD of the rows on the surface, following the ray, against the sphere of the unchanged frame
        sphere = oref.default_sphere(f, rows)
        wave = oref.wavefront(f, rows, out, sphere)
        assert np.all(np.isfinite(wave["dopd"][k].astype(float)))
        path_scale = float(np.max(np.abs(oref.optical_path(f).astype(float))))
        held("dopd", wave["dopd"][k],
             lambda p, m, h: ((oref.opd_of(p, rows, sphere)[0] - oref.opd_of(m, rows, sphere)[0]) / (2 * h)).astype(float),
             lambda h: 8 * EPS * path_scale / h)
        if not getattr(case, "focused", False):  # (the beam between the two flat mirrors comes to no focus)
            return
        # the best-focus shift of each source's rays on the surface: the same statistic on the re-traced frames.  Its
        # rounding floor: an error e in every landing point moves -cov(p, s) / var(s) by at most e / rms(s), an error e_s in
        # every slope by at most e_s (rms(p) + 2 |delta| rms(s)) / var(s)
        per_source = getattr(case, "rays_per_source", None) or case.rays.shape[1]
        groups = [rows[(f[rows, 4] // per_source) == g] for g in range(int(f[rows, 4].max() // per_source) + 1)]
        axis = (1.0, 0.0, 0.0)

        def shifts(frame):
            return np.array([float(ref.focus_shift(frame[g, 9:12], unit(frame[g, 12:15]), frame[g, 1], axis)) for g in groups])

        def focus_floor(h):
            floors = []
            for g in groups:
                p, s = f[g, 10:12], unit(f[g, 12:15])[:, 1:] / unit(f[g, 12:15])[:, :1]
                pc, sc = p - p.mean(axis=0), s - s.mean(axis=0)
                rms_p, rms_s = np.sqrt(np.mean(np.sum(pc * pc, axis=1))), np.sqrt(np.mean(np.sum(sc * sc, axis=1)))
                delta = abs(float(ref.focus_shift(f[g, 9:12], unit(f[g, 12:15]), f[g, 1], axis)))
                floors.append(4 * EPS / h * (scale / rms_s + (rms_p + 2 * delta * rms_s) / rms_s ** 2))
            return np.array(floors)

        analytic = [ref.focus_gradient(f[g, 9:12], unit(f[g, 12:15]), f[g, 1], out["dx"][k:k + 1, g], out["dd"][k:k + 1, g], axis)[0]
                    for g in groups]
        held("focus", analytic, lambda p, m, h: (shifts(p) - shifts(m)) / (2 * h), focus_floor)
    finally:
        for line in report:
            print(f"{name} parameter {k} ({type(case.parameters[k]).__name__}): {line}")
