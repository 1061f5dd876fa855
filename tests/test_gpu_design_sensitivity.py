"""Shape and index sensitivities of the frame on the device (DeviceFrame.sensitivity with Deformation and IndexChange, the
entry point prt_frame_design_sensitivity) against the numpy longdouble restatement (tests/design_reference.py), on frames
the C oracle traced on the CPU.

The error budget is tests/test_gpu_sensitivity.py's, derived the same way and extended; everything in it is taken from the
REFERENCE's geometry, nothing from the device's output.  Device and reference read the same float64 frame and table, so
the difference is the rounding of the device's float64 arithmetic (u = 2^-53 an operation, no contraction) carried through
the ray's interfaces.  Per ray and row:

  state     E bounds the absolute error of |dx| + |dd| after the row's landing, S = max over the parameters of |dx| + |dd|.
            The seventh plane, dnu, is the rate or 0 exactly: it carries no error.
  U         max over the parameters of |u| + |w| + |S|_F at the surfaces the step touches, with u = v + w x r + S r bounded
            by |v + w x r| + |S|_F |r|, r = x - c: the rigid pass's U gains |S|_F (|x - c| + 1); the 1 is the normal of the
            deformed surface, |(I - n n^T) S^T n| <= |S|_F.
  landing   as there: an error e in (do + t dd) comes out as at most (1 + c) e, c = 1 / |n.d|, T = max(1, t).
  interface as there (a, b per kind: refraction a = mu (2 + mu q), b = kappa (mu (1 + mu q) + |gamma|), q = 1 / ct;
            reflection a = 3, b = 4 kappa; undeviated a = 1, b = 0), and the refraction gains the dmu terms,
            dd' += dmu d + (ci dmu + mu (1 - ci^2) dmu / ct) n, of size at most I = (2 + mu q) |dmu| with
            dmu = (dnu - mu dnt) / nt: no carried error (dnu and dnt are exact), but values that the row's own roundings
            are relative to.
  gain      G = (1 + c) T (1 + a + b), E' <= G E + fresh.
  fresh     N_OPS operations, each with relative error u on intermediate values no larger than
            G (S_before + S_after + U + I), times kappa_g where the object point cancels.  N_OPS = 224: the rigid pass's
            128 (64 on the chain from the state to dx, 64 in the row's geometry) and, on the longer chain, two velocities
            S r (3 subtractions, 15 operations of the product, 3 additions: 21 each), the normal of the deformed surface
            (S^T n 15, n.q 5, the projection 6, the subtraction 3: 29) and the index terms (dmu 3, its part of dct 5, of
            dgamma 2, of dd' 12: 22): 128 + 42 + 29 + 22 = 221, rounded up to 224.
  bound     E of the row, for every component of dx.  In the invariance scenes the exact answer is 0 and the bound is
            G N_OPS u kappa_g U.

Every check prints its error / bound ratio before it asserts; the worst one observed is recorded in
profiles/design_sensitivity/README.md.  The sums are held as tests/test_gpu_sensitivity.py's ``check_sums`` holds them."""
import numpy as np
import pytest

import design_reference as ref
import design_scenes as cases
import helpers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
N_OPS = 224


def device_frame(frame, counts):
    from pyrayt_amd.frame import DeviceFrame

    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, list(counts))


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
        before, size_before, moving_before, conditioning = np.zeros(len(here)), np.zeros(len(here)), np.zeros(len(here)), info["conditioning"][here].copy()
        if g > 0:
            p = info["previous"][here]
            kind, mu, q, gamma, kappa = info["kind"][here], info["mu"][here], 1.0 / info["ct"][here], np.abs(info["gamma"][here]), info["kappa"][p]
            a = np.where(kind == 1, mu * (2 + mu * q), np.where(kind == 2, 3.0, 1.0))
            b = np.where(kind == 1, kappa * (mu * (1 + mu * q) + gamma), np.where(kind == 2, 4 * kappa, 0.0))
            index = np.where(kind == 1, (2 + mu * q) * info["dmu"][here], 0.0)
            before, size_before, moving_before = bound[p], size[p], moving[p]
            conditioning = np.maximum(conditioning, info["conditioning"][p])
        gain = (1 + c) * reach * (1 + a + b)
        fresh = N_OPS * U * conditioning * gain * (size_before + size[here] + moving_before + moving[here] + index)
        bound[here] = gain * before + fresh
    return bound


def reference_of(case, parameters=None, frame=None):
    from pyrayt_amd.scene import SceneSnapshot

    parameters = [ref.parameter(m) for m in (case.parameters if parameters is None else parameters)]
    frame = case.frame if frame is None else frame
    info = {}
    dx, dd, count = ref.trace_tangents(frame, ref.table_of(SceneSnapshot(case.parts).prims), parameters, info)
    return dx, dd, count, budget(frame, info, dx, dd, parameters)


def check_sums(got, frame, K, weight_column=1):
    """tests/test_gpu_sensitivity.py's: the device's sums against the longdouble sums of its own Jacobian."""
    jac = got.jacobian.cpu().numpy()
    rows = got.rows().cpu().numpy()
    x, w = frame[rows, 9:12], frame[rows, weight_column]
    own = np.transpose(jac, (0, 2, 1))
    want = ref.group_sums(x, w, own, got.pivots[0])
    size = ref.group_sums(np.abs(x), np.abs(w), np.abs(own), np.zeros(3))
    keep = np.all(np.isfinite(own), axis=(0, 2))
    r = np.abs(x[keep] - got.pivots[0])
    aw = np.abs(w[keep])
    size["wrr"] = (aw * np.sum(r * r, axis=1)).sum()
    size["wrd"] = np.einsum("n,nc,knc->k", aw, r, np.abs(own[:, keep]))
    have = ref.unpack(got.sums[0], K)
    chunks = (len(rows) + 255) // 256
    assert have["count"] == want["count"]
    for name in ("w", "wx", "wrr", "wd", "wrd", "moments"):
        error = np.abs(np.asarray(have[name] - want[name], dtype=float))
        limit = (10 + 6 + 4 + chunks) * U * np.asarray(size[name], dtype=float)
        assert np.all(error <= limit), (name, error, limit)


def check_against_reference(case, parameters=None, surfaces=None, what=""):
    """Every surface of the frame as the selection: the Jacobian against the reference within the budget, NaN where the
    reference has NaN, the four counters, and the sums."""
    parameters = case.parameters if parameters is None else parameters
    dx, dd, count, bound = reference_of(case, parameters)
    frame = device_frame(case.frame, case.counts)
    K = len(parameters)
    for surface in (np.unique(case.frame[:, 5]) if surfaces is None else surfaces):
        got = frame.sensitivity(int(surface), parameters, case.parts)
        rows = got.rows().cpu().numpy()
        assert sorted(rows.tolist()) == np.flatnonzero(case.frame[:, 5] == surface).tolist()
        jac = got.jacobian.cpu().numpy()
        want = np.transpose(dx[:, rows], (0, 2, 1))
        assert np.array_equal(np.isnan(jac), np.isnan(want.astype(float)))
        error = np.abs(jac - want).astype(float)
        ratio = np.nanmax(error / bound[rows][None, None, :]) if error.size and not np.all(np.isnan(error)) else 0.0
        print(f"{case.name}{what} surface {int(surface)}: K {K}, {len(rows)} rows, max error {np.nanmax(error) if error.size else 0:.3e}, "
              f"max bound {bound[rows].max() if len(rows) else 0:.3e}, worst error / bound {ratio:.4f}")
        assert np.all(np.nan_to_num(error) <= bound[rows][None, None, :]), (case.name, int(surface), float(ratio))
        assert (got.n_unknown, got.n_invalid, got.n_unfit, got.n_reflections) == tuple(
            count[name] for name in ("n_unknown", "n_invalid", "n_unfit", "n_reflections"))
        check_sums(got, case.frame, K)
    return dx, bound


# ---- the device against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CLOSED_FORMS)
def test_closed_form_scenes(name):
    case = cases.build(name, 65)
    dx, bound = check_against_reference(case)
    got = device_frame(case.frame, case.counts).sensitivity(case.surface, case.parameters, case.parts)
    jac = got.jacobian.cpu().numpy()
    rows = got.rows().cpu().numpy()
    assert len(rows) > 30
    eps = np.finfo(float).eps
    if getattr(case, "invariant", False):  # (the exact answer is 0: the budget alone, which scales with |u|)
        assert np.all(np.abs(jac) <= bound[rows][None, None, :]) and bound[rows].max() < 1e-8
    if name == "ball_radius":  # (0 on the detector, to the reference's own 64 eps of tests/test_host_design_sensitivity.py)
        assert np.all(np.abs(jac[0]) <= bound[rows][None, :] + 64 * eps)
    if name == "plate":
        t, angle, n = cases.PLATE.thickness, np.radians(cases.PLATE.angle), cases.PLATE.index
        s, c = np.sin(angle), np.cos(angle)
        shift = t * s * (1 - c / np.sqrt(n * n - s * s))
        for k, want in ((0, t * s * c * n * (n * n - s * s) ** -1.5), (1, shift)):
            assert np.all(np.abs(jac[k] - np.array([0.0, want, 0.0])[:, None]) <= bound[rows][None, :] + 32 * eps), k
    if name == "dish_focus":
        d = case.frame[rows, 12:15]
        a = np.asarray(case.parts[1].get_orientation(), dtype=float).reshape(-1)[:3]
        want = (case.axis - d * ((case.axis @ a) / (d @ a))[:, None]).T
        assert np.all(np.abs(jac[0] - want) <= bound[rows][None, :] + 32 * eps)


@pytest.mark.parametrize("name", cases.SYSTEMS)
def test_systems(name):
    case = cases.build(name, 257)
    assert len(case.counts) >= 2
    if name == "stopped":  # (the stop took rays in mid-path: their id slots go stale under a Deformation.radius on the lens)
        from pyrayt_amd import Deformation

        assert case.counts[1] < case.counts[0] and isinstance(case.parameters[0], Deformation)
    if name == "egg":
        from pyrayt_amd.scene import SceneSnapshot

        a = SceneSnapshot(case.parts).prims["minv"][0].reshape(4, 4)[:3, :3]
        assert not np.allclose(a @ a.T, np.eye(3))  # (minv is not rigid)
    if name in ("mirror", "dish"):
        assert reference_of(case)[2]["n_reflections"] == 257
    check_against_reference(case)


def sixteen(case):
    from pyrayt_amd import Deformation, IndexChange, Motion

    lens, det = case.parts
    front, back = lens.surface_ids[0][1], lens.surface_ids[1][1]
    shear = [[0.1, 0.4, 0.0], [-0.3, 0.2, 0.5], [0.0, 0.1, -0.2]]
    every = list(case.parameters)
    every += [Deformation.radius(front), Deformation.radius(back), Deformation.stretch(lens, (1, 0, 0)),
              Deformation.stretch(lens, (0, 1, 0), about=(0, 0.3, 0)), Deformation(lens, linear=shear),
              IndexChange(lens, rate=0.5), Motion(det, translate=(1, 0, 0)), Motion(lens, rotate=(0, 0, 1)),
              Deformation(det, translate=(0, 0, 1), rotate=(0, 0.5, 0), linear=shear, pivot=(1, 0.1, 0)),
              Deformation.stretch(det, (0, 1, 0)), Motion(lens, translate=(1, 0, 0))]
    assert len(every) == 16
    return every


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
@pytest.mark.parametrize("K", [1, 16])
def test_ray_counts_and_parameter_counts(n, K):
    case = cases.build("lens", n)
    every = sixteen(case)
    check_against_reference(case, every if K == 16 else every[3:4], surfaces=[int(case.surface.get_id())], what=f" n={n}")


# ---- bit for bit --------------------------------------------------------------------------------------------------------------
def outputs(got):
    return got.jacobian.cpu().numpy(), np.asarray(got.sums)


def test_a_motion_in_a_mixed_call_has_the_bits_of_a_call_of_motions_alone():
    from pyrayt_amd import Motion

    case = cases.build("lens", 257)
    frame = device_frame(case.frame, case.counts)
    motion = case.parameters[4]
    assert isinstance(motion, Motion)
    mixed = frame.sensitivity(case.surface, [motion, case.parameters[0], case.parameters[3]], case.parts)
    alone = frame.sensitivity(case.surface, [motion], case.parts)
    assert mixed.jacobian.shape == (3, 3, 257) and bool(torch.isfinite(mixed.jacobian).all())
    helpers.assert_same_bits(mixed.jacobian[0].cpu().numpy(), alone.jacobian[0].cpu().numpy(), "the Motion's slice")
    for other in (1, 2):  # (the other two are not it)
        assert np.abs(mixed.jacobian[other].cpu().numpy() - alone.jacobian[0].cpu().numpy()).max() > 1e-3


def test_sixteen_parameters_in_one_call_are_the_same_bits_as_one_at_a_time():
    case = cases.build("lens", 257)
    every = sixteen(case)
    frame = device_frame(case.frame, case.counts)
    all_at_once = frame.sensitivity(case.surface, every, case.parts)
    together, K = all_at_once.jacobian.cpu().numpy(), len(every)
    sums = all_at_once.sums[0]
    for k, one in enumerate(every):
        alone = frame.sensitivity(case.surface, one, case.parts)
        helpers.assert_same_bits(alone.jacobian.cpu().numpy()[0], together[k], f"parameter {k}")
        diagonal = 6 + 4 * K + k * (k + 1) // 2 + k
        shared = np.concatenate([sums[:6], sums[6 + 3 * k:9 + 3 * k], sums[6 + 3 * K + k:7 + 3 * K + k],
                                 sums[diagonal:diagonal + 1]])
        helpers.assert_same_bits(alone.sums[0], shared, f"the sums of parameter {k}")


def test_two_runs_and_a_permutation_of_the_rows_give_the_same_bits():
    case = cases.build("stopped", 1000)
    frame = device_frame(case.frame, case.counts)
    first = frame.sensitivity(case.surface, case.parameters, case.parts)
    again = frame.sensitivity(case.surface, case.parameters, case.parts)
    for a, b, what in zip(outputs(first), outputs(again), ("jacobian", "sums")):
        helpers.assert_same_bits(b, a, f"second run, {what}")
    rng = np.random.default_rng(5)
    shuffled, start = case.frame.copy(), 0
    for count in case.counts:
        shuffled[start:start + count] = case.frame[start + rng.permutation(count)]
        start += count
    assert not np.array_equal(shuffled, case.frame)
    mixed = device_frame(shuffled, case.counts).sensitivity(case.surface, case.parameters, case.parts)
    for a, b, what in zip(outputs(first), outputs(mixed), ("jacobian", "sums")):
        helpers.assert_same_bits(b, a, f"rows permuted, {what}")
    assert np.array_equal(shuffled[mixed.rows().cpu().numpy()], case.frame[first.rows().cpu().numpy()])


# ---- trace_sensitivity ---------------------------------------------------------------------------------------------------------
def test_trace_sensitivity_takes_a_mixed_list_and_its_gradient_is_the_references():
    """On a live RayTracer: trace_sensitivity is sensitivity of the traced frame bit for bit, and its gradient of the mean
    square radius is the reference's on that frame, within what the rows' bounds E allow: the gradient is
    2 sum w (x - centroid).dx / sum w, so an error E in every component of dx moves it by at most
    2 sum w |x - centroid|_1 E / sum w; the device sums about a pivot (the first row's landing point) and the host centres
    in longdouble, so the sums' own roundings are (20 + chunks) u (check_sums' figure) times the terms they add,
    2 (sum w |x - pivot|.|dx| + |centroid - pivot|.sum w |dx|) / sum w."""
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=1000)
    front = lens.surface_ids[0][1]
    mixed = [prt.Motion(det, translate=(1, 0, 0)), prt.Deformation.radius(front, keep=(-0.125, 0, 0)), prt.IndexChange(lens)]
    traced = tracer.trace_sensitivity(det, mixed)
    frame = tracer.trace_device()
    direct = frame.sensitivity(det, mixed, tracer.get_system())
    assert traced.jacobian.shape == (3, 3, 1000)
    for a, b, what in zip(outputs(direct), outputs(traced), ("jacobian", "sums")):
        helpers.assert_same_bits(b, a, what)
    assert torch.equal(traced.rows(), direct.rows())
    host = np.ascontiguousarray(frame.to_numpy(), dtype=np.float64)
    case = type("Case", (), {"parts": [lens, det], "parameters": mixed, "frame": host})
    dx, _, count, bound = reference_of(case)
    assert not any(count.values())
    rows = traced.rows().cpu().numpy()
    x, w = host[rows, 9:12].astype(ref.LD), host[rows, 1].astype(ref.LD)
    centroid = (w[:, None] * x).sum(axis=0) / w.sum()
    r = x - centroid
    want = 2 * np.einsum("n,nc,knc->k", w, r, dx[:, rows]) / w.sum()
    carried = 2 * np.sum(w * np.sum(np.abs(r), axis=1) * bound[rows]) / w.sum()
    pivot = traced.pivots[0].astype(ref.LD)
    terms = np.einsum("n,nc,knc->k", w, np.abs(x - pivot), np.abs(dx[:, rows])) + np.einsum(
        "c,n,knc->k", np.abs(centroid - pivot), w, np.abs(dx[:, rows]))
    summed = 2 * (20 + (len(rows) + 255) // 256) * U * terms / w.sum()
    error = np.abs(traced.mean_square_gradient[0] - want.astype(float))
    print(f"mean_square_gradient {traced.mean_square_gradient[0]}, error {error}, bound {np.asarray(carried + summed, dtype=float)}")
    assert np.all(np.abs(want) > 1e-6) and np.all(error <= np.asarray(carried + summed, dtype=float))


# ---- the entry point's own refusals ------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_what_is_not_finite():
    """Deformation and IndexChange refuse such values themselves; changed afterwards they reach prt_frame_design_sensitivity,
    which checks its arguments before it touches the device."""
    from pyrayt_amd import Deformation, IndexChange

    case = cases.build("lens", 65)
    lens, det = case.parts
    frame = device_frame(case.frame, case.counts)
    bad = Deformation.radius(lens.surface_ids[0][1])
    bad.linear = np.full((3, 3), np.nan)
    with pytest.raises(ValueError, match="linear is not finite"):
        frame.sensitivity(det, [case.parameters[4], bad], case.parts)
    worse = IndexChange(lens)
    worse.rate = float("inf")
    with pytest.raises(ValueError, match="index rate is not finite"):
        frame.sensitivity(det, [worse], case.parts)
