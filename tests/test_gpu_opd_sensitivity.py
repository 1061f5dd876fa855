"""Wavefront sensitivities on the device (DeviceFrame.sensitivity(wavefront=), the entry point prt_frame_opd_sensitivity)
against the numpy longdouble restatement (tests/opd_sensitivity_reference.py), on frames the C oracle traced on the CPU.
Small shapes: 2 groups x 300 rays x 3 generations (the selection spans two 256-row workgroups a group with a partial tail,
and with one group of 600 a source's boundary falls inside a workgroup), one 64-ray and one 1-ray group.

The error budget continues tests/test_gpu_design_sensitivity.py's, whose ``budget`` gives E, the bound of the absolute
error of |dx| + |dd| of a row; everything in it is taken from the REFERENCE's values, nothing from the device's output.
u = 2^-53 an operation, no contraction.  Per row, with n the index, |.| the reference's magnitudes, maxima over the
parameters:

  dL      dL = dL_prev + dnu len + n d.(dx - start), start = dx_prev + 1e-6 dd: the carried error is
          EL = EL_prev + n (E_prev + 2 E) and the row's own 16 operations (the difference 3, the product 5, len's 8 relative
          to dnu len, which is exact in dnu) act on values no larger than M = |dL_prev| + |dnu| len + n (|dx| + |start|):
          EL += 16 u M.
  s, E    the larger root from float64 Q, u, P, R: 24 operations, relative to the terms that cancel in c = |Q - P|^2 - R^2
          and in the discriminant: Es = 24 u (b^2 + a (|Q - P|^2 + R^2)) / disc * max(|s|, R); E - P then has
          Eep = Es + 4 u (|Q| + |s| + |P|).
  dfield  dL - s dnu - n u.dx: EL + |dnu| Es + n E + 12 u (|dL| + |s dnu| + n |dx|).
  dE      y = dx - s dd: Ey = (1 + |s|) E + Es |dd| + 6 u (|dx| + |s| |dd|);  ds = (E - P).y / (E - P).u with
          c = |E - P| / |(E - P).u|:  Eds = c (Ey + 2 Eep |y| / R) + 12 u c |y|;  EdE = Ey + Eds + 4 u (|y| + |ds|).
  dopd    dfield + n u.dE: E_dfield + n EdE + 8 u (|dfield| + n |dE|).
  dpupil  dE.e / r_p: (EdE + 8 u |dE|) / r_p.
  opd     (L - n s) - pivot, L the sum of g + 1 segments: E_opd = (8 (g + 1) + 4) u (|L| + n |s| + |pivot|) + n Es.

The sums are held as tests/test_gpu_sensitivity.py's ``check_sums`` holds them: against the longdouble sums of the
device's own rows, a product, a 256-row chain, the chunks and the fold: (8 + 256 + chunks + 6) u times the sum of the
absolute values; the basis Z by the device's recurrence against the factorial formula adds 64 u |Z| <= 64 u sqrt(2 (n + 1)).
dzernike and the gradients are functions of the sums: their bounds propagate the rows' bounds through the same formulas
(``derived``).  Every check prints its error / bound ratio before it asserts."""
import numpy as np
import pytest

import design_reference as dref
import helpers
import opd_scenes as cases
import opd_sensitivity_reference as ref
from test_gpu_design_sensitivity import budget, device_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
_REFERENCE = {}


def sixteen(case):
    """Sixteen parameters from the scene's five: the five, then rigid motions of the lens and the detector."""
    from pyrayt_amd import Deformation, Motion

    glass, det = case.parts
    extra = [Motion(glass, translate=(1, 0, 0)), Motion(glass, rotate=(0, 1, 0)), Motion(det, rotate=(0, 0, 1), pivot=(1, 0, 0)),
             Motion(det, translate=(1, 0, 0)), Deformation(glass, translate=(0, 0, 1)), Motion(glass, rotate=(1, 0, 0)),
             Deformation.radius(glass.surface_ids[1][1], keep=(0.125, 0, 0)), Motion(glass, translate=(0.3, -0.2, 0.5)),
             Deformation.stretch(glass, (0, 0, 1)), Motion(det, translate=(0, 1, 0)), Motion(glass, rotate=(0, 1, 1), pivot=(0.1, 0, 0))]
    return list(case.parameters) + extra


def reference_of(case, parameters, key):
    """The reference's tangents and the rows' bound E, computed once per (scene, parameters) and shared, never changed."""
    from pyrayt_amd.scene import SceneSnapshot

    if key not in _REFERENCE:
        pars = [dref.parameter(m) for m in parameters]
        table = dref.table_of(SceneSnapshot(case.parts).prims)
        info = {}
        dx, dd, _ = dref.trace_tangents(case.frame, table, pars, info)
        tangents = ref.trace(case.frame, table, pars)
        _REFERENCE[key] = (tangents, budget(case.frame, info, dx, dd, pars))
    return _REFERENCE[key]


def row_bounds(frame, rows, tangents, E, wave, ball):
    """The bounds of the module docstring for the selected rows: a dict of arrays (n,)."""
    big = lambda v, axis: np.nan_to_num(np.max(np.abs(np.asarray(v, dtype=float)), axis=axis))  # noqa: E731
    norm = lambda v: np.nan_to_num(np.max(np.linalg.norm(np.asarray(v, dtype=float), axis=2), axis=0))  # noqa: E731
    dx, dd, dnu, dL = tangents["dx"], tangents["dd"], tangents["dnu"], tangents["dL"]
    previous = tangents["previous"]
    n_all = frame[:, 3]
    length = np.linalg.norm(frame[:, 9:12] - frame[:, 6:9], axis=1)
    EL = np.zeros(len(frame))
    generation = frame[:, 0].astype(int)
    for g in range(generation.max() + 1):
        here = np.flatnonzero(generation == g)
        p = previous[here]
        before = EL[p] if g else 0.0
        E_prev = E[p] if g else 0.0
        dL_prev = big(dL[:, p], 0) if g else 0.0
        start = (norm(dx[:, p]) + 1e-6 * norm(dd[:, here])) if g else 0.0
        M = dL_prev + big(dnu[:, here], 0) * length[here] + n_all[here] * (norm(dx[:, here]) + start)
        EL[here] = before + n_all[here] * (E_prev + 2 * E[here]) + 16 * U * M
    n = frame[rows, 3]
    q, u, P, R = frame[rows, 9:12], frame[rows, 12:15], np.asarray(ball["P"], dtype=float), float(ball["R"])
    d = q - P
    a, b, dd2 = np.sum(u * u, axis=1), np.sum(d * u, axis=1), np.sum(d * d, axis=1)
    disc = b * b - a * (dd2 - R * R)
    s = np.nan_to_num(np.asarray(wave["s"], dtype=float))
    with np.errstate(invalid="ignore", divide="ignore"):
        Es = 24 * U * (b * b + a * (dd2 + R * R)) / disc * np.maximum(np.abs(s), R)
        Es = np.where(disc > 0, Es, 0.0)  # (a line that misses the sphere: NaN on both sides, nothing to bound)
    Eep = Es + 4 * U * (np.linalg.norm(q, axis=1) + np.abs(s) + np.linalg.norm(P))
    Er, dxs, dds = E[rows], norm(dx[:, rows]), norm(dd[:, rows])
    dnus, dLs = big(dnu[:, rows], 0), big(dL[:, rows], 0)
    E_dfield = EL[rows] + dnus * Es + n * Er + 12 * U * (dLs + np.abs(s) * dnus + n * dxs)
    y = dxs + np.abs(s) * dds
    Ey = (1 + np.abs(s)) * Er + Es * dds + 6 * U * y
    ep = np.asarray(ref.extend(frame, rows, ball["P"], ball["R"])[1], dtype=float) - P
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.linalg.norm(ep, axis=1) / np.abs(np.sum(ep * u, axis=1))
    Eds = c * (Ey + 2 * Eep * y / R) + 12 * U * c * y
    EdE = Ey + Eds + 4 * U * (y + c * y)
    dE = norm(wave["dE"])
    E_dopd = E_dfield + n * EdE + 8 * U * (big(wave["dfield"], 0) + n * dE)
    pr = float(ball["pupil_radius"])
    path = np.asarray(ref.optical_path(frame)[rows], dtype=float)
    E_opd = (8 * (generation[rows] + 1) + 4) * U * (np.abs(path) + n * np.abs(s) + abs(float(ball["pivot"]))) + n * Es
    out = dict(dfield=E_dfield, dopd=E_dopd, dpupil=(EdE + 8 * U * dE) / pr, opd=E_opd,
               pupil=(Eep + 8 * U * np.nan_to_num(np.linalg.norm(ep, axis=1))) / pr)
    return {name: np.nan_to_num(value, nan=0.0) for name, value in out.items()}  # (a ray that misses: NaN on both sides)


def ball_of(wavefront, g):
    from pyrayt_amd.frame import pupil_axes

    axes = pupil_axes()
    return dict(P=wavefront.reference[g], R=wavefront.radius[g], pivot=wavefront.pivot[g],
                pupil_radius=wavefront.pupil_radius[g], e1=axes[3:6], e2=axes[6:9])


def check(case, parameters, key, J, rays_per_source, n_groups, weights="intensity", frame=None, radius=None, note=""):
    """One call against the reference: the rows, the raw sums, dzernike and the gradients; returns the Sensitivity."""
    tangents, E = reference_of(case, parameters, key)
    K = len(parameters)
    dev = device_frame(case.frame, case.counts) if frame is None else frame
    wavefront = dev.wavefront(case.surface, zernike=J, weights=weights, rays_per_source=rays_per_source, n_groups=n_groups,
                              radius=radius)
    got = dev.sensitivity(case.surface, parameters, case.parts, weights=weights, rays_per_source=rays_per_source,
                          n_groups=n_groups, wavefront=wavefront)
    selected = got.rows().cpu().numpy()
    ids = case.frame[selected, 4]
    group = (ids // rays_per_source).astype(int) if rays_per_source else np.zeros(len(ids), dtype=int)
    assert np.array_equal(group, np.sort(group)) and sorted(selected.tolist()) == np.flatnonzero(
        case.frame[:, 5] == case.surface.get_id()).tolist()
    have = {name: getattr(got, name).cpu().numpy() for name in ("dfield", "dopd", "dpupil", "opd", "pupil")}
    for g in range(n_groups):
        at = np.flatnonzero(group == g)
        rows = selected[at]
        ball = ball_of(wavefront, g)
        wave = ref.wavefront(case.frame, rows, tangents, ball)
        bound = row_bounds(case.frame, rows, tangents, E, wave, ball)
        for name, mine, want in (("dfield", have["dfield"][:, at], wave["dfield"]), ("dopd", have["dopd"][:, at], wave["dopd"]),
                                 ("dpupil", have["dpupil"][:, :, at], wave["dpupil"]), ("opd", have["opd"][at], wave["opd"]),
                                 ("pupil", have["pupil"][at].T, wave["pupil"].T)):
            want = np.asarray(want, dtype=float)
            assert np.array_equal(np.isnan(mine), np.isnan(want)), name
            error = np.abs(mine - want)
            ratio = np.nanmax(error / bound[name]) if not np.all(np.isnan(error)) else 0.0
            print(f"{case.name}{note} K {K} J {J} group {g} ({len(at)} rows) {name}: max |value| {np.nanmax(np.abs(want)):.3e}, "
                  f"max error {np.nanmax(error):.3e}, worst error / bound {ratio:.4f}")
            assert np.all(np.nan_to_num(error) <= bound[name]), (name, float(ratio))
        w = case.frame[rows, 1] if weights else np.ones(len(rows))
        check_sums(got, g, have, at, wave, w, K, J)
        derived(got, wavefront, g, wave, w, bound, K, J, tangents["dx"][:, rows])
        assert got.n_missed[g] == int(np.sum(wave["followed"] & ~wave["met"])) == wavefront.n_missed[g]
    return got, wavefront


def check_sums(got, g, have, at, wave, w, K, J):
    """The device's sums against the longdouble sums of its own rows (module docstring)."""
    own = dict(wave, dfield=have["dfield"][:, at].astype(ref.LD), dopd=have["dopd"][:, at].astype(ref.LD),
               opd=have["opd"][at].astype(ref.LD), pupil=have["pupil"][at].astype(ref.LD))
    want = ref.sums(own, w, J)
    size_of = dict(own, dfield=np.abs(own["dfield"]), dopd=np.abs(own["dopd"]), opd=np.abs(own["opd"]),
                   u=np.abs(np.asarray(wave["u"])))
    keep = np.isfinite(own["opd"].astype(float))
    z = np.abs(ref.zernike(J, own["pupil"][keep, 0], own["pupil"][keep, 1]))
    aw = np.abs(np.asarray(w, dtype=ref.LD))[keep]
    size = ref.sums(size_of, np.abs(w), J)
    size["z_dfield"] = np.einsum("jn,n,kn->kj", z, aw, size_of["dfield"][:, keep])
    size["z_nu"] = np.einsum("jn,n,nc->cj", z, aw, (wave["n"][:, None] * size_of["u"])[keep])
    mine = ref.unpack(got.opd_sums[g], K, J)
    chunks = (len(at) + 255) // 256
    assert mine["count"] == want["count"] and mine["missed"] == want["missed"]
    for name in ("w", "w_opd", "w_opd2", "z_dfield", "z_nu", "w_dopd", "w_opd_dopd", "w_dfield", "w_opd_dfield", "moments"):
        error = np.abs(np.asarray(mine[name] - want[name], dtype=float))
        limit = (8 + 256 + chunks + 6 + (64 if name.startswith("z_") else 0)) * U * np.asarray(size[name], dtype=float)
        assert np.all(error <= limit), (name, float(np.max(error / np.maximum(limit, 1e-300))))


def derived(got, wavefront, g, wave, w, bound, K, J, dx):
    """dzernike and the gradients against the reference's, the rows' bounds carried through the same formulas: a
    right-hand side Z^T W y moves by at most sum w |Z| E_y + |dZ| ..., the solve multiplies by |(Z^T W Z)^-1| and adds
    cond * eps of its own; the variance gradient 2 (<OPD dopd> - <OPD> <dopd>) moves by 2 <|OPD - mean| E_dopd + 2 E_opd
    |dopd - mean|> and the RMS's by that over 2 rms plus the RMS's own relative error."""
    w = np.asarray(w, dtype=ref.LD)
    total = ref.sums(wave, w, J)
    keep = np.isfinite(wave["opd"].astype(float))
    W = float(total["w"])
    z = np.abs(np.asarray(ref.zernike(J, wave["pupil"][keep, 0], wave["pupil"][keep, 1]), dtype=float))
    grad_z = (np.arange(1, J + 1) ** 1.5)[:, None] * 4  # (|grad Z_j| <= sqrt(2 (n + 1)) n (n + 2) / 2 <= 4 j^1.5: n (n + 1) / 2 < j)
    zwz = np.asarray(total["zwz"], dtype=float)
    inverse = np.abs(np.linalg.pinv(zwz))
    cond = np.linalg.cond(zwz)
    fixed, follow = got.dzernike("fixed")[g], got.dzernike("centroid")[g]
    # (centroid_gradient is of every ray that was followed, the rays that miss the sphere among them)
    followed = np.all(np.isfinite(dx.astype(float)), axis=(0, 2))
    dP = np.einsum("n,knc->kc", w[followed], dx[:, followed]) / w[followed].sum()
    nu = np.abs(np.asarray(wave["n"][:, None] * wave["u"], dtype=float))[keep]
    wk = np.asarray(w, dtype=float)[keep]
    for k in range(K):
        for name, mine, rhs, extra in (
                ("fixed", fixed[k], total["z_dfield"][k], 0.0),
                ("centroid", follow[k], total["z_dfield"][k] - dP[k] @ total["z_nu"], (nu * bound["dfield"][keep, None]).sum(axis=1))):
            want = ref.fit(zwz, rhs)
            y = np.abs(np.asarray(wave["dfield"][k], dtype=float))[keep] + np.abs(np.asarray(dP[k], dtype=float)).sum()
            moved = (z * (wk * (bound["dfield"][keep] + extra))).sum(axis=1) + (grad_z * (wk * bound["pupil"][keep] * y)).sum(axis=1)
            limit = inverse @ (moved + 512 * U * (z * wk * y).sum(axis=1)) + 64 * cond * U * np.max(np.abs(want))
            error = np.abs(mine - want)
            assert np.all(error <= limit), (name, k, float(np.max(error / limit)))
    stats = ref.statistics(total)
    opd, dopd = np.asarray(wave["opd"], dtype=float)[keep], np.asarray(wave["dopd"], dtype=float)[:, keep]
    mean, rms = float(total["w_opd"] / total["w"]), float(np.sqrt(stats["variance"]))
    centred = np.abs(dopd - (dopd @ wk / W)[:, None])
    moved = 2 * ((np.abs(opd - mean) * bound["dopd"][keep] + 2 * bound["opd"][keep] * centred) @ wk) / W
    moved += 2 * 512 * U * (np.abs(opd) * np.abs(dopd)) @ wk / W
    error = np.abs(got.wavefront_variance_gradient[g] - np.asarray(stats["variance_gradient"], dtype=float))
    print(f"  variance gradient: max |value| {np.max(np.abs(stats['variance_gradient'])):.3e}, max error {error.max():.3e}, "
          f"worst error / bound {np.max(error / moved):.4f}")
    assert np.all(error <= moved)
    rms_moved = (bound["opd"][keep] @ wk / W) * 2 + 512 * U * np.abs(opd).max()
    limit = moved / (2 * rms) + np.abs(np.asarray(stats["rms_gradient"], dtype=float)) * rms_moved / rms
    error = np.abs(got.rms_opd_gradient[g] - np.asarray(stats["rms_gradient"], dtype=float))
    assert np.all(error <= limit), float(np.max(error / limit))
    assert abs(np.sqrt(got.wavefront_variance[g]) - wavefront.rms[g]) <= rms_moved  # (the statistic Wavefront.rms reports)


# ---- against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, J", [(1, 4), (5, 15), (16, 36), (5, 36), (16, 4)])
def test_two_groups_of_300_rays_against_the_reference(K, J):
    case = cases.build("two_fields", 300)
    assert case.counts == [600, 600, 600]
    parameters = {1: [case.parameters[2]], 5: list(case.parameters), 16: sixteen(case)}[K]
    got, wavefront = check(case, parameters, ("two_fields", 300, K), J, 300, 2)
    assert not (got.n_unknown or got.n_invalid or got.n_unfit) and not got.n_missed.any()  # (every ray meets the sphere)
    assert np.array_equal(got.count, [300, 300])


def test_one_group_of_600_a_source_boundary_inside_a_workgroup_and_no_weights():
    case = cases.build("two_fields", 300)
    got, _ = check(case, list(case.parameters), ("two_fields", 300, 5), 15, None, 1, weights=None, note=" as one group")
    assert got.count[0] == 600


@pytest.mark.parametrize("n", [64, 1])
def test_edge_shapes(n):
    case = cases.build("singlet", n)
    # (one ray: the default sphere has no radial extent to normalise by; a pupil radius is a property of the call)
    dev = device_frame(case.frame, case.counts)
    parameters = list(case.parameters)
    tangents, E = reference_of(case, parameters, ("singlet", n))
    wavefront = dev.wavefront(case.surface, zernike=4, pupil_radius=0.25)
    got = dev.sensitivity(case.surface, parameters, case.parts, wavefront=wavefront, weights=None)
    rows = got.rows().cpu().numpy()
    ball = ball_of(wavefront, 0)
    wave = ref.wavefront(case.frame, rows, tangents, ball)
    bound = row_bounds(case.frame, rows, tangents, E, wave, ball)
    for name in ("dfield", "dopd", "dpupil"):
        error = np.abs(getattr(got, name).cpu().numpy() - np.asarray(wave[name], dtype=float))
        print(f"singlet {n} rays {name}: max error {error.max():.3e}, worst error / bound {np.max(error / bound[name]):.4f}")
        assert np.all(error <= bound[name])
    have = {name: getattr(got, name).cpu().numpy() for name in ("dfield", "dopd", "dpupil", "opd", "pupil")}
    check_sums(got, 0, have, np.arange(n), wave, np.ones(n), 5, 4)
    assert got.count[0] == n and got.opd_sums[0, 0] == n


# ---- against the existing paths ---------------------------------------------------------------------------------------------
def test_jacobian_and_sums_keep_the_bits_of_the_existing_passes():
    from pyrayt_amd import Motion

    case = cases.build("two_fields", 300)
    dev = device_frame(case.frame, case.counts)
    glass, det = case.parts
    mixed = list(case.parameters)
    rigid = [Motion(glass, translate=(0, 1, 0)), Motion(glass, rotate=(0, 0, 1), pivot=(0, 0, 0)), Motion(det, translate=(1, 0, 0))]
    for parameters in (mixed, rigid):
        old = dev.sensitivity(case.surface, parameters, case.parts, rays_per_source=300, n_groups=2)
        new = dev.sensitivity(case.surface, parameters, case.parts, rays_per_source=300, n_groups=2, wavefront=True)
        helpers.assert_same_bits(new.jacobian.cpu().numpy(), old.jacobian.cpu().numpy(), "jacobian")
        helpers.assert_same_bits(new.sums, old.sums, "sums")
        assert torch.equal(new.rows(), old.rows())
        assert (new.n_unknown, new.n_invalid, new.n_unfit, new.n_reflections) == (old.n_unknown, old.n_invalid, old.n_unfit,
                                                                                   old.n_reflections)
        assert old.wavefront is None and new.wavefront is not None
        with pytest.raises(ValueError, match="wavefront"):
            old.dzernike()
        with pytest.raises(ValueError, match="wavefront"):
            old.step(merit="wavefront")


# ---- invariance -------------------------------------------------------------------------------------------------------------
def outputs(got):
    return [getattr(got, name).cpu().numpy() for name in ("jacobian", "dfield", "dopd", "dpupil", "opd", "pupil")] + [got.sums, got.opd_sums]


def test_two_runs_and_a_permutation_of_the_rows_give_the_same_bits():
    case = cases.build("two_fields", 300)
    parameters = list(case.parameters)
    kw = dict(rays_per_source=300, n_groups=2)
    dev = device_frame(case.frame, case.counts)
    wavefront = dev.wavefront(case.surface, weights="intensity", **kw)
    first = dev.sensitivity(case.surface, parameters, case.parts, wavefront=wavefront, **kw)
    again = dev.sensitivity(case.surface, parameters, case.parts, wavefront=wavefront, **kw)
    for a, b in zip(outputs(first), outputs(again)):
        helpers.assert_same_bits(a, b, "run to run")
    rng = np.random.default_rng(5)
    shuffled, start = case.frame.copy(), 0
    for count in case.counts:
        shuffled[start:start + count] = case.frame[start + rng.permutation(count)]
        start += count
    other = device_frame(shuffled, case.counts)
    # the sphere is held fixed: the same P, R, pivot and pupil radius, whatever row the shuffled frame would take its pivot from
    moved = other.wavefront(case.surface, reference=wavefront.reference, radius=wavefront.radius,
                            pupil_radius=float(wavefront.pupil_radius[0]), weights="intensity", **kw)
    moved.pivot[:] = wavefront.pivot
    moved.pupil_radius[:] = wavefront.pupil_radius
    again = other.sensitivity(case.surface, parameters, case.parts, wavefront=moved, **kw)
    assert np.array_equal(shuffled[again.rows().cpu().numpy(), 4], case.frame[first.rows().cpu().numpy(), 4])
    for a, b in zip(outputs(first), outputs(again)):
        helpers.assert_same_bits(a, b, "permuted rows")


def test_a_parameter_alone_has_the_bits_it_has_among_sixteen():
    case = cases.build("two_fields", 300)
    every = sixteen(case)
    kw = dict(rays_per_source=300, n_groups=2)
    dev = device_frame(case.frame, case.counts)
    wavefront = dev.wavefront(case.surface, zernike=15, weights="intensity", **kw)
    together = dev.sensitivity(case.surface, every, case.parts, wavefront=wavefront, **kw)
    z = together.dzernike()
    for k in (0, 3, 4, 7, 15):
        alone = dev.sensitivity(case.surface, [every[k]], case.parts, wavefront=wavefront, **kw)
        for name in ("dfield", "dopd", "dpupil", "jacobian"):
            helpers.assert_same_bits(getattr(alone, name).cpu().numpy()[0], getattr(together, name).cpu().numpy()[k], name)
        helpers.assert_same_bits(alone._z_rhs[:, 0], together._z_rhs[:, k], "Z^T W dfield")
        helpers.assert_same_bits(alone.dzernike()[:, 0], z[:, k], "dzernike")
        helpers.assert_same_bits(alone.rms_opd_gradient[:, 0], together.rms_opd_gradient[:, k], "rms gradient")


# ---- misses, caller-shaded surfaces -------------------------------------------------------------------------------------------
def test_rays_that_miss_the_sphere_are_nan_and_left_out():
    case = cases.build("two_fields", 300)
    rows = np.flatnonzero(case.frame[:, 5] == case.surface.get_id())
    # a sphere about the centroid of group 0 whose radius the outermost landing points exceed: a line that lands further
    # than R from P and runs nearly along the axis does not meet it.  The reference names the rays.
    at = rows[case.frame[rows, 4] < 300]
    P = case.frame[at, 9:12].mean(axis=0)
    far = np.sort(np.linalg.norm(case.frame[at, 9:12] - P, axis=1))
    radius = [0.5 * (far[-6] + far[-5]), 1.0]
    got, wavefront = check(case, list(case.parameters), ("two_fields", 300, 5), 15, 300, 2, radius=radius, note=" small sphere")
    assert got.n_missed[0] == wavefront.n_missed[0] and 1 <= got.n_missed[0] <= 8 and got.n_missed[1] == 0
    assert got.opd_sums[0, 0] == 300 - got.n_missed[0] and got.opd_sums[1, 0] == 300
    assert (300 - got.n_missed[0]) / 300 >= 0.97  # (the share of rays that are not left out)
    lost = np.isnan(got.opd.cpu().numpy())
    assert lost.sum() == got.n_missed[0]
    for name in ("dfield", "dopd"):
        assert np.all(np.isnan(getattr(got, name).cpu().numpy()[:, lost])) and not np.isnan(getattr(got, name).cpu().numpy()[:, ~lost]).any()
    assert np.all(np.isnan(got.dpupil.cpu().numpy()[:, :, lost])) and not np.isnan(got.jacobian.cpu().numpy()).any()
    assert np.all(np.isfinite(got.rms_opd_gradient)) and np.all(np.isfinite(got.dzernike()))


def test_a_caller_shaded_surface_is_nan_and_counted_unfit():
    case = cases.build("two_fields", 300)
    frame = case.frame.copy()
    last = np.flatnonzero((frame[:, 0] == 2) & np.isin(frame[:, 4], [3, 77, 412]))
    turn = np.array([[np.cos(0.01), -np.sin(0.01), 0], [np.sin(0.01), np.cos(0.01), 0], [0, 0, 1]])
    frame[last, 12:15] = frame[last, 12:15] @ turn.T  # (a direction that fits neither Snell's law nor a reflection)
    dev = device_frame(frame, case.counts)
    got = dev.sensitivity(case.surface, list(case.parameters), case.parts, rays_per_source=300, n_groups=2, wavefront=True)
    assert got.n_unfit == 3 and got.n_unknown == 0 and got.n_invalid == 0
    lost = np.isin(frame[got.rows().cpu().numpy(), 4], [3, 77, 412])
    for name in ("dfield", "dopd", "dpupil", "jacobian"):
        value = getattr(got, name).cpu().numpy()
        assert np.all(np.isnan(value[..., lost])) and not np.isnan(value[..., ~lost]).any(), name
    assert np.array_equal(got.opd_sums[:, 0], [298, 299]) and not got.n_missed.any()


# ---- argument errors, workspace -------------------------------------------------------------------------------------------------
def test_a_wavefront_of_another_selection_is_refused():
    case = cases.build("two_fields", 300)
    dev = device_frame(case.frame, case.counts)
    other = device_frame(case.frame, case.counts)
    parameters = list(case.parameters)
    kw = dict(rays_per_source=300, n_groups=2)
    front = int(case.frame[0, 5])
    for wrong in (dev.wavefront(front, **kw), dev.wavefront(case.surface, generation=2, **kw), dev.wavefront(case.surface),
                  dev.wavefront(case.surface, rays_per_source=150, n_groups=4), other.wavefront(case.surface, **kw),
                  dev.wavefront(case.surface, weights="intensity", **kw)):
        with pytest.raises(ValueError, match="wavefront"):
            dev.sensitivity(case.surface, parameters, case.parts, weights=None, wavefront=wrong, **kw)
    with pytest.raises(ValueError, match="wavefront"):
        dev.sensitivity(case.surface, parameters, case.parts, wavefront="centroid", **kw)
    with pytest.raises(ValueError, match="16"):
        dev.sensitivity(case.surface, sixteen(case) + [parameters[0]], case.parts, wavefront=True, **kw)
    good = dev.sensitivity(case.surface, parameters, case.parts, weights=None, wavefront=dev.wavefront(case.surface, **kw), **kw)
    assert good.dfield.shape == (5, 600) and good.dpupil.shape == (5, 2, 600) and good.dzernike().shape == (2, 5, 15)
    step = good.step(merit="wavefront")
    assert step.shape == (2, 5) and np.all(np.isfinite(step))
    with pytest.raises(ValueError, match="merit"):
        good.step(merit="strehl")


def test_workspace_is_carved_to_the_byte_and_the_old_sizes_stand():
    from pyrayt_amd import engine

    lib = engine.library()
    n_ids, n_surfaces, K, n_groups, most, J = 600, 4, 5, 2, 300, 15
    rigid = lib.prt_frame_sensitivity_workspace_bytes(n_ids, n_surfaces, K, n_groups, most)
    design = lib.prt_frame_design_sensitivity_workspace_bytes(n_ids, n_surfaces, K, n_groups, most)
    wave = lib.prt_frame_opd_sensitivity_workspace_bytes(n_ids, n_surfaces, K, n_groups, most, J)
    # 64 (alignment) + 64 (words) + 200 a surface + group_first + pivots + the state + last_row + partials + stamps + 64
    chunks, fixed = 2, 64 + 64 + 200 * n_surfaces + 8 * (n_groups + 1) + 24 * n_groups + 8 * n_ids + 4 * n_ids
    old = 8 * n_groups * chunks * (6 + 4 * K + K * (K + 1) // 2)
    assert rigid == fixed + 48 * K * n_ids + old and design == fixed + 56 * K * n_ids + old
    entries = 5 + J * (K + 3) + 4 * K + K * (K + 1) // 2
    assert wave == fixed + 64 * K * n_ids + old + 8 * 6 * n_groups + 8 * n_groups * chunks * entries
    for bad in ((n_ids, n_surfaces, 17, n_groups, most, J), (n_ids, n_surfaces, K, n_groups, most, 37),
                (n_ids, n_surfaces, K, n_groups, most, 0), (0, n_surfaces, K, n_groups, most, J)):
        assert lib.prt_frame_opd_sensitivity_workspace_bytes(*bad) < 0
    # the call stays inside what the function names: a workspace of exactly that size inside a larger, patterned buffer
    case = cases.build("two_fields", 300)
    dev = device_frame(case.frame, case.counts)
    kw = dict(rays_per_source=300, n_groups=2)
    real_empty, sizes = torch.empty, []

    def guarded(size, *a, **k):
        if k.get("dtype") is torch.uint8 and isinstance(size, int) and size > 0:
            whole = torch.full((size + 4096,), 0xA5, dtype=torch.uint8, device=k["device"])
            sizes.append((size, whole))
            return whole[:size]
        return real_empty(size, *a, **k)

    torch.empty = guarded
    try:
        got = dev.sensitivity(case.surface, list(case.parameters), case.parts, wavefront=True, **kw)
    finally:
        torch.empty = real_empty
    prims = 3 + 1  # (the lens's two spheres and its stock, the detector)
    want = lib.prt_frame_opd_sensitivity_workspace_bytes(600, prims, 5, 2, 300, 15)
    assert want in [size for size, _ in sizes]
    for size, whole in sizes:
        assert bool((whole[size:] == 0xA5).all()), size
    assert np.all(np.isfinite(got.rms_opd_gradient))


@pytest.mark.parametrize("scene, n, nobody", [("two_fields", 300, False), ("singlet", 1, False), ("singlet", 1, True)])
def test_every_form_runs_through_the_one_layout_and_the_motions_keep_their_bits(scene, n, nobody):
    """The five forms (rigid, design, wavefront, launch without and with wavefront=) and slopes=True with no launch
    parameter, each inside a workspace of exactly the size its own function names with a patterned guard behind it; the
    launch form's size from the others' ends; jacobian and sums of the two Motions the same bits in all of them.  The
    frame of the test above, then one ray in one group, then a surface no row ends on (no chunk, a fold of nothing)."""
    from pyrayt_amd import Motion, SourceMotion, engine

    lib = engine.library()
    case = cases.build(scene, n)
    dev = device_frame(case.frame, case.counts)
    glass, det = case.parts
    surface = 10 ** 6 if nobody else case.surface
    if scene == "two_fields":
        kw, n_ids, n_groups = dict(rays_per_source=300, n_groups=2, weights="intensity"), 600, 2
        wavefront = dev.wavefront(surface, zernike=15, **kw)
    else:  # (one ray has no radial extent to normalise by: a pupil radius is a property of the call)
        kw, n_ids, n_groups = dict(weights=None), 1, 1
        wavefront = dev.wavefront(surface, zernike=4, pupil_radius=0.25, **kw)
    J, prims, most = wavefront.terms, 3 + 1, 0 if nobody else n
    motions = [Motion(glass, translate=(0, 1, 0)), Motion(det, rotate=(0, 0, 1), pivot=(1, 0.1, 0))]
    shaped = motions + [case.parameters[2], case.parameters[4]]  # (a radius and the index)
    launched = motions + [SourceMotion(None, translate=(0, 1, 0))]

    def size(name, K, *more):
        return getattr(lib, f"prt_frame_{name}_workspace_bytes")(n_ids, prims, K, n_groups, most, *more)

    up8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
    for K in (2, 3, 4):
        assert size("launch_sensitivity", K, J) == up8(size("opd_sensitivity", K, J) - 64) + 56 * prims + 64
        assert size("launch_sensitivity", K, 0) == up8(size("design_sensitivity", K) - 64) + 56 * prims + 64
    forms = [("rigid", motions, {}, size("sensitivity", 2)),
             ("design", shaped, {}, size("design_sensitivity", 4)),
             ("wavefront", shaped, dict(wavefront=wavefront), size("opd_sensitivity", 4, J)),
             ("launch", launched, {}, size("launch_sensitivity", 3, 0)),
             ("launch with wavefront", launched, dict(wavefront=wavefront), size("launch_sensitivity", 3, J)),
             ("slopes=True", motions, dict(slopes=True), size("launch_sensitivity", 2, 0))]
    real_empty, first = torch.empty, None
    for what, parameters, more, want in forms:
        sizes = []

        def guarded(size, *a, **k):
            if k.get("dtype") is torch.uint8 and isinstance(size, int) and size > 0:
                whole = torch.full((size + 4096,), 0xA5, dtype=torch.uint8, device=k["device"])
                sizes.append((size, whole))
                return whole[:size]
            return real_empty(size, *a, **k)

        torch.empty = guarded
        try:
            got = dev.sensitivity(surface, parameters, case.parts, **kw, **more)
        finally:
            torch.empty = real_empty
        assert want > 0 and want in [size for size, _ in sizes], (what, want, [size for size, _ in sizes])
        for size_, whole in sizes:
            assert bool((whole[size_:] == 0xA5).all()), (what, size_)
        K = got.n_parameters
        assert got.jacobian.shape == (K, 3, 0 if nobody else n * n_groups)
        assert (got.slopes is not None) == what.startswith(("launch", "slopes")), what
        assert (got.wavefront is not None) == ("wavefront" in more), what
        assert bool(torch.isfinite(got.jacobian).all()) and np.array_equal(got.count, [most] * n_groups), what
        own = np.concatenate([got.sums[:, :6 + 3 * 2], got.sums[:, 6 + 3 * K:6 + 3 * K + 2],
                              got.sums[:, 6 + 4 * K:6 + 4 * K + 3]], axis=1)  # (the entries of parameters 0 and 1)
        if first is None:
            first = (got.jacobian[:2].cpu().numpy(), own)
            assert nobody or float(np.abs(first[0]).max()) > 1e-3
        helpers.assert_same_bits(got.jacobian[:2].cpu().numpy(), first[0], f"jacobian, {what}")
        helpers.assert_same_bits(own, first[1], f"sums, {what}")
