"""Launch and wavelength sensitivities of the frame on the device (DeviceFrame.sensitivity with SourceMotion and
WavelengthChange, the entry point prt_frame_launch_sensitivity) against the numpy longdouble restatement
(tests/launch_reference.py), on frames the C oracle traced on the CPU.  Shapes: three sources of 65 rays (195 ids: a partial
wave past one, the sources' boundaries at 64|65 and 129|130 inside waves), one scene of 257 rays (a second workgroup of one
row), K = 1 and 16.

The error budget is tests/test_gpu_design_sensitivity.py's (its docstring derives E, the bound of the absolute error of
|dx| + |dd| of a row, from the REFERENCE's geometry: gain G = (1 + c) T (1 + a + b), E' <= G E + fresh), extended by what the
launch form adds, counted from the formulas of include/prt.h as N_OPS is counted there.  u = 2^-53 an operation.

  seed        do = v + w x (o - c): 3 subtractions, the cross product 9, 3 additions; dd = w x d: 9.  24 operations in
              generation 0 on values no larger than |do| + |dd| of the seed, which joins the magnitudes of ``fresh`` there.
  dispersion  w2 1, t_i 3, n2 9, `down` 14 (three times two products, a square and a quotient, two additions), the root and
              the quotient 2, the rate 1: 30 operations, no cancellation (every term of `down` has one sign, t_i = w2 - c_i is
              far from zero for a wavelength the trace accepted): dnt and dnu carry a RELATIVE error of at most 32 u.  They
              enter dd' through dmu = (dnu - mu dnt) / nt, whose two terms are bounded apart, (|dnu| + mu |dnt|) / nt: the
              index magnitude I = (2 + mu q) that, which ``fresh`` already multiplies by N_OPS u.
  N_OPS       224 + 24 + 32 = 280.
  slopes      dd of the row: E bounds it as it bounds dx.

The wavefront outputs continue tests/test_gpu_opd_sensitivity.py's bounds (``row_bounds`` there) with two changes: in
generation 0 the segment's start is the seed, not 0 (M gains n |do|, the carried error n E of the seed's own row), and dnu is
no longer exact: EL gains 32 u |dnu| len, dfield 32 u |s dnu|.

Every check prints its worst error / bound ratio per scene before it asserts; the worst ones observed are recorded in
profiles/launch_sensitivity/README.md.  The sums are held as ``check_sums`` of the two earlier tests holds them."""
import numpy as np
import pytest

import helpers
import launch_reference as ref
import launch_scenes as cases
import opd_sensitivity_reference as oref
from test_gpu_design_sensitivity import check_sums, device_frame
from test_gpu_opd_sensitivity import ball_of
from test_gpu_opd_sensitivity import check_sums as check_opd_sums

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
N_OPS = 280
N_DISPERSION = 32
_REFERENCE = {}


def budget(frame, info, dx, dd, parameters):
    """The bound E per row (module docstring), from the reference's dx, dd (K, R, 3) and its per-row geometry."""
    rows = len(frame)
    size = np.nan_to_num(np.max(np.linalg.norm(dx.astype(float), axis=2) + np.linalg.norm(dd.astype(float), axis=2), axis=0))
    moving = np.zeros(rows)
    for par in parameters:
        on = np.isin(frame[:, 5], list(par["ids"]))
        r = frame[:, 9:12] - par["c"]
        stretch = np.linalg.norm(par["S"])
        speed = (np.linalg.norm(par["v"] + np.cross(par["w"], r), axis=1) + np.linalg.norm(par["w"])
                 + stretch * (np.linalg.norm(r, axis=1) + 1))
        moving = np.maximum(moving, np.where(on, speed, 0.0))
    bound = np.zeros(rows)
    generation = frame[:, 0].astype(int)
    for g in range(generation.max() + 1 if rows else 0):
        here = np.flatnonzero(generation == g)
        c = 1.0 / np.abs(info["nd"][here])
        reach = np.maximum(1.0, np.abs(info["t"][here]))
        a, b, index = np.zeros(len(here)), np.zeros(len(here)), np.zeros(len(here))
        before, moving_before, conditioning = np.zeros(len(here)), np.zeros(len(here)), info["conditioning"][here].copy()
        size_before = info["seed"][here].copy()  # (generation 0: the seed is the state the landing starts from)
        if g > 0:
            p = info["previous"][here]
            kind, mu, q, gamma, kappa = info["kind"][here], info["mu"][here], 1.0 / info["ct"][here], np.abs(info["gamma"][here]), info["kappa"][p]
            a = np.where(kind == 1, mu * (2 + mu * q), np.where(kind == 2, 3.0, 1.0))
            b = np.where(kind == 1, kappa * (mu * (1 + mu * q) + gamma), np.where(kind == 2, 4 * kappa, 0.0))
            index = np.where(kind == 1, (2 + mu * q) * info["dmu_size"][here], 0.0)
            before, size_before, moving_before = bound[p], size[p], moving[p]
            conditioning = np.maximum(conditioning, info["conditioning"][p])
        gain = (1 + c) * reach * (1 + a + b)
        fresh = N_OPS * U * conditioning * gain * (size_before + size[here] + moving_before + moving[here] + index)
        bound[here] = np.nan_to_num(gain * before + fresh)
    return bound


def reference_of(case, parameters=None, key=None):
    """The reference's tangents and the rows' bound E, computed once per (scene, parameters) and shared, never changed."""
    from pyrayt_amd.scene import SceneSnapshot

    key = (case.name, case.rays.shape[1], key)
    if key not in _REFERENCE:
        snapshot = SceneSnapshot(case.parts)
        pars = [ref.parameter(m) for m in (case.parameters if parameters is None else parameters)]
        info = {}
        out = ref.trace(case.frame, ref.table_of(snapshot.prims), pars, ref.glasses_of(snapshot), info)
        out["info"] = info
        _REFERENCE[key] = (out, budget(case.frame, info, out["dx"], out["dd"], pars))
    return _REFERENCE[key]


def wave_bounds(frame, rows, tangents, E, wave, ball):
    """tests/test_gpu_opd_sensitivity.py's ``row_bounds`` with the seed as the start of generation 0 and a rounded dnu."""
    big = lambda v, axis: np.nan_to_num(np.max(np.abs(np.asarray(v, dtype=float)), axis=axis))  # noqa: E731
    norm = lambda v: np.nan_to_num(np.max(np.linalg.norm(np.asarray(v, dtype=float), axis=2), axis=0))  # noqa: E731
    dx, dd, dnu, dL = tangents["dx"], tangents["dd"], tangents["dnu"], tangents["dL"]
    previous, seed = tangents["previous"], tangents["info"]["seed"]
    n_all = frame[:, 3]
    length = np.linalg.norm(frame[:, 9:12] - frame[:, 6:9], axis=1)
    EL = np.zeros(len(frame))
    generation = frame[:, 0].astype(int)
    for g in range(generation.max() + 1):
        here = np.flatnonzero(generation == g)
        p = previous[here]
        before = EL[p] if g else 0.0
        E_prev = E[p] if g else E[here]
        dL_prev = big(dL[:, p], 0) if g else 0.0
        start = (norm(dx[:, p]) + 1e-6 * norm(dd[:, here])) if g else seed[here]
        carried = big(dnu[:, here], 0) * length[here]
        M = dL_prev + carried + n_all[here] * (norm(dx[:, here]) + start)
        EL[here] = np.nan_to_num(before + n_all[here] * (E_prev + 2 * E[here]) + 16 * U * M + N_DISPERSION * U * carried)
    n = frame[rows, 3]
    q, u, P, R = frame[rows, 9:12], frame[rows, 12:15], np.asarray(ball["P"], dtype=float), float(ball["R"])
    d = q - P
    a, b, dd2 = np.sum(u * u, axis=1), np.sum(d * u, axis=1), np.sum(d * d, axis=1)
    disc = b * b - a * (dd2 - R * R)
    s = np.nan_to_num(np.asarray(wave["s"], dtype=float))
    with np.errstate(invalid="ignore", divide="ignore"):
        Es = 24 * U * (b * b + a * (dd2 + R * R)) / disc * np.maximum(np.abs(s), R)
        Es = np.where(disc > 0, Es, 0.0)
    Eep = Es + 4 * U * (np.linalg.norm(q, axis=1) + np.abs(s) + np.linalg.norm(P))
    Er, dxs, dds = E[rows], norm(dx[:, rows]), norm(dd[:, rows])
    dnus, dLs = big(dnu[:, rows], 0), big(dL[:, rows], 0)
    E_dfield = EL[rows] + dnus * Es + n * Er + (12 * U) * (dLs + np.abs(s) * dnus + n * dxs) + N_DISPERSION * U * np.abs(s) * dnus
    y = dxs + np.abs(s) * dds
    Ey = (1 + np.abs(s)) * Er + Es * dds + 6 * U * y
    ep = np.asarray(oref.extend(frame, rows, ball["P"], ball["R"])[1], dtype=float) - P
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.linalg.norm(ep, axis=1) / np.abs(np.sum(ep * u, axis=1))
    Eds = c * (Ey + 2 * Eep * y / R) + 12 * U * c * y
    EdE = Ey + Eds + 4 * U * (y + c * y)
    dE = norm(wave["dE"])
    E_dopd = E_dfield + n * EdE + 8 * U * (big(wave["dfield"], 0) + n * dE)
    pr = float(ball["pupil_radius"])
    path = np.asarray(oref.optical_path(frame)[rows], dtype=float)
    E_opd = (8 * (generation[rows] + 1) + 4) * U * (np.abs(path) + n * np.abs(s) + abs(float(ball["pivot"]))) + n * Es
    out = dict(dfield=E_dfield, dopd=E_dopd, dpupil=(EdE + 8 * U * dE) / pr, opd=E_opd,
               pupil=(Eep + 8 * U * np.nan_to_num(np.linalg.norm(ep, axis=1))) / pr)
    return {name: np.nan_to_num(value, nan=0.0) for name, value in out.items()}


def worst_ratio(error, bound):
    """The largest error / bound over the entries that have both (a NaN on both sides and 0 within 0 are no ratio)."""
    at = np.isfinite(error) & (bound > 0)
    return float(np.max(error[at] / bound[at])) if at.any() else 0.0


def counters(got):
    return got.n_unknown, got.n_invalid, got.n_unfit, got.n_reflections


def check(case, parameters=None, key=None, surfaces=None, wavefront=False, J=6, frame=None, what=""):
    """The Jacobian and the slopes of the rows on each surface against the reference within E, NaN where it has NaN, the
    four counters and the sums; with ``wavefront`` (on the case's own surface, one group per source) the wavefront outputs
    and their sums as well.  Returns the worst error / bound ratio."""
    parameters = list(case.parameters if parameters is None else parameters)
    tangents, E = reference_of(case, parameters, key)
    dev = device_frame(case.frame, case.counts) if frame is None else frame
    K, worst = len(parameters), 0.0
    count = tuple(tangents["count"][name] for name in ("n_unknown", "n_invalid", "n_unfit", "n_reflections"))
    for surface in ([int(case.surface.get_id())] if surfaces is None else surfaces):
        got = dev.sensitivity(int(surface), parameters, case.parts)
        rows = got.rows().cpu().numpy()
        assert sorted(rows.tolist()) == np.flatnonzero(case.frame[:, 5] == surface).tolist()
        assert got.slopes is not None and got.slopes.shape == got.jacobian.shape == (K, 3, len(rows))
        for name, mine, want in (("jacobian", got.jacobian, tangents["dx"]), ("slopes", got.slopes, tangents["dd"])):
            mine = mine.cpu().numpy()
            want = np.transpose(want[:, rows], (0, 2, 1)).astype(float)
            assert np.array_equal(np.isnan(mine), np.isnan(want)), name
            error = np.abs(mine - want)
            ratio = worst_ratio(error, np.broadcast_to(E[rows][None, None, :], error.shape))
            worst = max(worst, ratio)
            print(f"{case.name}{what} surface {int(surface)} K {K} ({len(rows)} rows) {name}: max |value| "
                  f"{np.nanmax(np.abs(want)) if want.size else 0:.3e}, max error {np.nanmax(error) if error.size else 0:.3e}, "
                  f"worst error / bound {ratio:.4f}")
            assert np.all(np.nan_to_num(error) <= E[rows][None, None, :]), (case.name, name, int(surface), ratio)
        assert counters(got) == count
        check_sums(got, case.frame, K)
    if wavefront:
        per_source = case.rays_per_source
        n_groups = int(case.rays.shape[1] // per_source)
        wave_of = dev.wavefront(case.surface, zernike=J, weights="intensity", rays_per_source=per_source, n_groups=n_groups)
        plain = dev.sensitivity(case.surface, parameters, case.parts, rays_per_source=per_source, n_groups=n_groups)
        got = dev.sensitivity(case.surface, parameters, case.parts, rays_per_source=per_source, n_groups=n_groups, wavefront=wave_of)
        for a, b, name in ((got.jacobian, plain.jacobian, "jacobian"), (got.slopes, plain.slopes, "slopes")):
            helpers.assert_same_bits(a.cpu().numpy(), b.cpu().numpy(), f"{name} with and without wavefront=")
        helpers.assert_same_bits(np.asarray(got.sums), np.asarray(plain.sums), "sums with and without wavefront=")
        assert counters(got) == count == counters(plain)
        selected = got.rows().cpu().numpy()
        group = (case.frame[selected, 4] // per_source).astype(int)
        assert np.array_equal(group, np.sort(group))
        have = {name: getattr(got, name).cpu().numpy() for name in ("dfield", "dopd", "dpupil", "opd", "pupil")}
        for g in range(n_groups):
            at = np.flatnonzero(group == g)
            rows = selected[at]
            ball = ball_of(wave_of, g)
            wave = oref.wavefront(case.frame, rows, tangents, ball)
            bound = wave_bounds(case.frame, rows, tangents, E, wave, ball)
            for name, mine, want in (("dfield", have["dfield"][:, at], wave["dfield"]), ("dopd", have["dopd"][:, at], wave["dopd"]),
                                     ("dpupil", have["dpupil"][:, :, at], wave["dpupil"]), ("opd", have["opd"][at], wave["opd"]),
                                     ("pupil", have["pupil"][at].T, wave["pupil"].T)):
                want = np.asarray(want, dtype=float)
                assert np.array_equal(np.isnan(mine), np.isnan(want)), name
                error = np.abs(mine - want)
                ratio = worst_ratio(error, np.broadcast_to(bound[name], error.shape))
                worst = max(worst, ratio)
                print(f"{case.name}{what} K {K} J {J} group {g} ({len(at)} rows) {name}: max |value| {np.nanmax(np.abs(want)):.3e}, "
                      f"max error {np.nanmax(error):.3e}, worst error / bound {ratio:.4f}")
                assert np.all(np.nan_to_num(error) <= bound[name]), (name, ratio)
            check_opd_sums(got, g, have, at, wave, case.frame[rows, 1], K, J)
            assert got.n_missed[g] == int(np.sum(wave["followed"] & ~wave["met"]))
    print(f"{case.name}{what} K {K}: worst error / bound of the scene {worst:.4f}")
    return worst


# ---- the device against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 1])
def test_three_sources_of_65_rays_against_the_reference(K):
    case = cases.build("fields", 65)
    assert case.counts == [195, 195, 195] and sorted(set(case.frame[:, 2])) == list(cases.WAVELENGTHS)
    if K == 16:
        check(case, key=16, surfaces=np.unique(case.frame[:, 5]), wavefront=True)
    else:
        for k in (2, 4, 5):  # (a launch rotation, a wavelength change, one source's rotation: each alone)
            check(case, [case.parameters[k]], key=("alone", k), wavefront=True, what=f" parameter {k}")


def test_257_rays_a_second_workgroup_of_one_row():
    case = cases.build("cone", 257)
    assert case.counts == [257, 257, 257]
    check(case, key="all", surfaces=np.unique(case.frame[:, 5]), wavefront=True)


@pytest.mark.parametrize("name", ["invariance", "free_space", "flat_mirror", "parabola", "plate", "plate_constant", "prism",
                                  "two_mirrors"])
def test_closed_form_scenes_and_mirrors(name):
    case = cases.build(name, 65)
    check(case, key="all", surfaces=np.unique(case.frame[:, 5]))
    got = device_frame(case.frame, case.counts).sensitivity(case.surface, case.parameters, case.parts)
    if name == "plate_constant":  # (no dispersion: nothing moves, to the bit)
        assert not got.jacobian.any() and not got.slopes.any()
    if name == "parabola":
        rows = got.rows().cpu().numpy()
        vertex = np.flatnonzero(case.frame[rows, 4] == 0)
        E = reference_of(case, None, "all")[1]
        assert np.all(np.abs(got.jacobian.cpu().numpy()[0, :, vertex[0]] - [0.0, -cases.PARABOLA.focus, 0.0])
                      <= E[rows[vertex[0]]] + 64 * np.finfo(float).eps * cases.PARABOLA.focus)
        focal = got.effective_focal_length(0, axis=(-1, 0, 0))
        assert abs(focal[0] - cases.PARABOLA.focus) < 3 * (0.6 / 6.0) ** 2 * cases.PARABOLA.focus  # (the group's mean: coma)


# ---- the edges of a parameter's id range ------------------------------------------------------------------------------------
def positive_zero(values, what):
    helpers.assert_same_bits(values, np.zeros_like(values), what)


@pytest.mark.parametrize("among", [False, True])
def test_a_source_motion_of_the_middle_source_moves_ids_65_to_129_alone(among):
    from pyrayt_amd import SourceMotion

    case = cases.build("fields", 65)
    one = SourceMotion.of_source(1, 65, translate=(0.1, 0.4, -0.2), rotate=(0.2, -0.1, 1.0), pivot=(-0.125, 0, 0))
    parameters = (list(case.parameters[:7]) + [one] + list(case.parameters[7:15])) if among else [one]
    k = 7 if among else 0
    tangents, E = reference_of(case, parameters, ("edge", among))
    dev = device_frame(case.frame, case.counts)
    for surface in np.unique(case.frame[:, 5]):
        got = dev.sensitivity(int(surface), parameters, case.parts)
        rows = got.rows().cpu().numpy()
        ids = case.frame[rows, 4]
        named = (ids >= 65) & (ids < 130)
        assert named.sum() == 65 and (~named).sum() == 130
        for name, mine, want in (("jacobian", got.jacobian, tangents["dx"]), ("slopes", got.slopes, tangents["dd"])):
            mine = mine.cpu().numpy()[k]
            want = want[k][rows].T.astype(float)
            assert np.all(np.abs(want[:, named]).max(axis=0) > 0) and not want[:, ~named].any()
            assert np.all(np.abs(mine - want)[:, named] <= E[rows][named])
            positive_zero(mine[:, ~named], f"{name} of the rays outside [65, 130) on surface {int(surface)}")


# ---- per-ray wavelengths ------------------------------------------------------------------------------------------------------
def test_each_source_has_its_own_dispersion_and_a_nan_wavelength_is_lost_where_the_reference_loses_it():
    from pyrayt_amd import WavelengthChange

    case = cases.build("fields", 65)
    tangents, _ = reference_of(case, None, 16)
    inside = case.frame[:, 0] == 1
    rates = np.abs(tangents["dnu"][4][inside].astype(float))
    by_source = [np.unique(rates[(case.frame[inside, 4] // 65) == g]) for g in range(3)]
    assert all(len(v) == 1 for v in by_source) and by_source[0][0] > by_source[1][0] > by_source[2][0] > 0.02
    broken = cases.build("fields_nan", 65)
    assert np.isnan(broken.frame[:, 2]).sum() >= 1 and broken.counts[0] == 195
    worst = check(broken, [WavelengthChange(), broken.parameters[2]], key="nan", surfaces=np.unique(broken.frame[:, 5]))
    assert worst > 0
    # the same ray with its rows kept, by hand: the NaN goes into its index in the glass, and the pass counts it invalid
    frame = case.frame.copy()
    lost = frame[:, 4] == 72
    frame[lost, 2] = np.nan
    frame[lost & (frame[:, 0] == 1), 3] = np.nan
    by_hand = type("Case", (), dict(vars(case), frame=frame, name="fields_by_hand"))
    out, _ = reference_of(by_hand, [WavelengthChange(), case.parameters[2]], "by hand")
    assert out["count"]["n_invalid"] == 1
    check(by_hand, [WavelengthChange(), case.parameters[2]], key="by hand")
    got = device_frame(frame, case.counts).sensitivity(case.surface, [WavelengthChange(), case.parameters[2]], case.parts)
    at = case.frame[got.rows().cpu().numpy(), 4] == 72
    assert got.n_invalid == 1 and bool(torch.isnan(got.jacobian[:, :, at]).all()) and bool(torch.isnan(got.slopes[:, :, at]).all())
    assert bool(torch.isfinite(got.jacobian[:, :, ~at]).all())


# ---- bit for bit --------------------------------------------------------------------------------------------------------------
def outputs(got):
    out = {"jacobian": got.jacobian.cpu().numpy(), "sums": np.asarray(got.sums)}
    if got.slopes is not None:
        out["slopes"] = got.slopes.cpu().numpy()
    if got.wavefront is not None:
        out.update({name: getattr(got, name).cpu().numpy() for name in ("dfield", "dopd", "dpupil", "opd", "pupil")})
        out["opd_sums"] = np.asarray(got.opd_sums)
    return out


def test_two_runs_and_a_permutation_of_the_rows_give_the_same_bits():
    case = cases.build("fields", 65)
    dev = device_frame(case.frame, case.counts)
    kw = dict(rays_per_source=65, n_groups=3)
    wave_of = dev.wavefront(case.surface, weights="intensity", **kw)
    first = dev.sensitivity(case.surface, case.parameters, case.parts, wavefront=wave_of, **kw)
    again = dev.sensitivity(case.surface, case.parameters, case.parts, wavefront=wave_of, **kw)
    for (what, a), b in zip(outputs(first).items(), outputs(again).values()):
        helpers.assert_same_bits(b, a, f"second run, {what}")
    rng = np.random.default_rng(5)
    shuffled, start = case.frame.copy(), 0
    for count in case.counts:
        shuffled[start:start + count] = case.frame[start + rng.permutation(count)]
        start += count
    assert not np.array_equal(shuffled, case.frame)
    other = device_frame(shuffled, case.counts)
    # the sphere is held fixed: the same P, R, pivot and pupil radius, whatever row the shuffled frame would take its pivot
    # from (tests/test_gpu_opd_sensitivity.py does the same)
    moved = other.wavefront(case.surface, reference=wave_of.reference, radius=wave_of.radius,
                            pupil_radius=float(wave_of.pupil_radius[0]), weights="intensity", **kw)
    moved.pivot[:] = wave_of.pivot
    moved.pupil_radius[:] = wave_of.pupil_radius
    mixed = other.sensitivity(case.surface, case.parameters, case.parts, wavefront=moved, **kw)
    for (what, a), b in zip(outputs(first).items(), outputs(mixed).values()):
        helpers.assert_same_bits(b, a, f"rows permuted, {what}")
    assert np.array_equal(shuffled[mixed.rows().cpu().numpy()], case.frame[first.rows().cpu().numpy()])


def test_sixteen_parameters_in_one_call_are_the_same_bits_as_one_at_a_time():
    case = cases.build("fields", 65)
    dev = device_frame(case.frame, case.counts)
    kw = dict(rays_per_source=65, n_groups=3)
    wave_of = dev.wavefront(case.surface, zernike=6, weights="intensity", **kw)
    together = dev.sensitivity(case.surface, case.parameters, case.parts, wavefront=wave_of, **kw)
    all_at_once, K = outputs(together), 16
    for k, one in enumerate(case.parameters):
        alone = outputs(dev.sensitivity(case.surface, one, case.parts, wavefront=wave_of, **kw))
        launched = type(one).__name__ in ("SourceMotion", "WavelengthChange")
        assert ("slopes" in alone) == launched  # (one of the earlier kinds alone takes the entry point it always took)
        for name in ("jacobian", "slopes", "dfield", "dopd", "dpupil") if launched else ("jacobian", "dfield", "dopd", "dpupil"):
            helpers.assert_same_bits(alone[name][0], all_at_once[name][k], f"{name} of parameter {k}")
        diagonal = 6 + 4 * K + k * (k + 1) // 2 + k
        for g in range(3):
            sums = all_at_once["sums"][g]
            shared = np.concatenate([sums[:6], sums[6 + 3 * k:9 + 3 * k], sums[6 + 3 * K + k:7 + 3 * K + k],
                                     sums[diagonal:diagonal + 1]])
            helpers.assert_same_bits(alone["sums"][g], shared, f"the sums of parameter {k}, group {g}")


def test_the_earlier_kinds_keep_the_bits_of_the_earlier_entry_points_beside_a_source_motion():
    from pyrayt_amd import Deformation, IndexChange, Motion

    case = cases.build("fields", 65)
    dev = device_frame(case.frame, case.counts)
    kw = dict(rays_per_source=65, n_groups=3)
    wave_of = dev.wavefront(case.surface, zernike=6, weights="intensity", **kw)
    launch = case.parameters[2]
    for k in (6, 7, 8, 12):
        old = case.parameters[k]
        assert isinstance(old, (Motion, Deformation, IndexChange))
        for wavefront in (None, wave_of):
            beside = dev.sensitivity(case.surface, [launch, old], case.parts, wavefront=wavefront, **kw)
            alone = dev.sensitivity(case.surface, [old], case.parts, wavefront=wavefront, **kw)
            assert alone.slopes is None and beside.slopes is not None
            helpers.assert_same_bits(beside.jacobian[1].cpu().numpy(), alone.jacobian[0].cpu().numpy(),
                                     f"{type(old).__name__} beside a SourceMotion")
            assert bool(torch.isfinite(alone.jacobian).all()) and float(alone.jacobian.abs().max()) > 1e-3
            if wavefront is not None:
                for name in ("dfield", "dopd", "dpupil", "opd", "pupil"):
                    a, b = getattr(beside, name).cpu().numpy(), getattr(alone, name).cpu().numpy()
                    helpers.assert_same_bits(a[1] if name.startswith("d") else a, b[0] if name.startswith("d") else b, name)


# ---- trace_sensitivity ---------------------------------------------------------------------------------------------------------
def test_trace_sensitivity_takes_both_new_kinds_and_is_sensitivity_of_the_traced_frame():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1, material=prt.materials.glass["BK7"])
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=3, wavelength=0.55).move_x(-6)  # (a real image, behind the detector)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=65)
    mixed = [prt.SourceMotion.of_source(0, rotate=(0, 0, 1), pivot=(-6, 0, 0)), prt.WavelengthChange(),
             prt.SourceMotion(None, translate=(0, 1, 0)), prt.Motion(det, translate=(1, 0, 0))]
    traced = tracer.trace_sensitivity(det, mixed)
    frame = tracer.trace_device()
    resolved = [prt.SourceMotion.of_source(0, 65, rotate=(0, 0, 1), pivot=(-6, 0, 0))] + mixed[1:]
    direct = frame.sensitivity(det, resolved, tracer.get_system())
    assert traced.jacobian.shape == traced.slopes.shape == (4, 3, 65)
    assert bool(torch.isfinite(traced.jacobian).all()) and float(traced.jacobian[1].abs().max()) > 1e-4
    for (what, a), b in zip(outputs(direct).items(), outputs(traced).values()):
        helpers.assert_same_bits(b, a, what)
    assert torch.equal(traced.rows(), direct.rows())
    gradient = traced.focus_gradient()
    assert gradient.shape == (1, 4) and np.all(np.isfinite(gradient)) and gradient[0, 1] > 0  # (red focuses farther: dn/dlambda < 0)
    host = np.ascontiguousarray(frame.to_numpy(), dtype=np.float64)
    rows = traced.rows().cpu().numpy()
    d = host[rows, 12:15] / np.linalg.norm(host[rows, 12:15], axis=1, keepdims=True)
    want = ref.focus_gradient(host[rows, 9:12], d, host[rows, 1], np.transpose(direct.jacobian.cpu().numpy(), (0, 2, 1)),
                              np.transpose(direct.slopes.cpu().numpy(), (0, 2, 1)), (1.0, 0.0, 0.0)).astype(float)
    # (the same formula in longdouble on the device's own tangents: what differs is torch's float64 sums over 65 rows of
    # terms that cancel in cov and var, relative to the sizes before the cancellation: |p| |s| / var(s) <= 1e4 here)
    assert np.all(np.abs(gradient[0] - want) <= 1e4 * 65 * 2.0 ** -52 * np.maximum(1.0, np.abs(want)))
    matrix = traced.transfer((2, 2), (0, 0), basis=[(0, 1, 0), (0, 0, 1)])
    assert matrix.shape == (65, 4, 4)
    helpers.assert_same_bits(matrix[:, 0, 0].cpu().numpy(), traced.jacobian[2, 1].cpu().numpy(), "A_yy is d(y1)/d(launch y)")
    helpers.assert_same_bits(matrix[:, 3, 2].cpu().numpy(), traced.slopes[0, 2].cpu().numpy(), "a slope entry")


# ---- the entry point's own refusals ------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_what_is_not_finite_or_not_a_range():
    from pyrayt_amd import SourceMotion, WavelengthChange

    case = cases.build("cone", 65)
    dev = device_frame(case.frame, case.counts)
    bad = WavelengthChange()
    bad.rate = float("inf")
    with pytest.raises(ValueError, match="wavelength rate is not finite"):
        dev.sensitivity(case.surface, [bad], case.parts)
    worse = SourceMotion((3, 4), translate=(0, 1, 0))
    worse.id_range = (7.0, 3.0)
    with pytest.raises(ValueError, match="not a range"):
        dev.sensitivity(case.surface, [worse], case.parts)
    worst = SourceMotion(None, translate=(0, 1, 0))
    worst.twist = np.full(9, np.nan)
    with pytest.raises(ValueError, match="twist is not finite"):
        dev.sensitivity(case.surface, [worst], case.parts)
