"""Sensitivities of the frame on the device (DeviceFrame.sensitivity, RayTracer.trace_sensitivity) against the numpy
longdouble restatement of the definitions (tests/sensitivity_reference.py), on frames the C oracle traced on the CPU.

The error budget.  Device and reference read the same float64 frame and the same table, so there is no data error: the
difference is the rounding of the device's float64 arithmetic (u = 2^-53 an operation; the library is built without
contraction) carried through the ray's interfaces.  Per ray and row, with everything taken from the REFERENCE's geometry:

  state     the tangent is (dx, dd); E bounds the absolute error of |dx| + |dd| after the row's landing, S = max over the
            parameters of |dx| + |dd| is the state's size, U = max over the parameters of |u| + |w| at the surfaces the
            step touches (0 where nothing moves).
  landing   dx = do + t dd + d dt, dt = n.(u - do - t dd) / (n.d): an error e in (do + t dd) comes out as at most
            (1 + c) e with c = 1 / |n.d|, and do + t dd <= T (|do| + |dd|), T = max(1, t).
  interface dd' = a-part of dd plus b-part of dx, by the formulas of include/prt.h:
              refraction  dd' = mu dd + (mu - mu^2 ci / ct) dci n + gamma dn, |dci| <= |dn| + |dd|, |dn| <= kappa |dx - u|
                          + |w|:  a = mu (2 + mu q), b = kappa (mu (1 + mu q) + |gamma|), q = 1 / ct  (ci <= 1);
              reflection  dd' = dd - 2 [(dd.n + d.dn) n + (d.n) dn]:  a = 3, b = 4 kappa;
              undeviated  a = 1, b = 0;
            kappa = |W|_F of the surface left behind (0 on a flat one).  do' = dx + 1e-6 dd' adds nothing that (1 + a + b)
            does not cover.
  gain      so one row multiplies the error by at most G = (1 + c) T (1 + a + b): E' <= G E + fresh.
  fresh     the roundings of the row itself: N_OPS operations, each with relative error u on intermediate values no
            larger than G (S_before + S_after + U).  N_OPS = 128: about 64 on the chain from the state to dx (normal
            derivative 25, interface 20, landing 15, rounded one by one) and as many again in the row's geometry (object
            point, normal, its length, the direction's normalisation, t), whose relative errors multiply the same values.
            Where the object point A x + b cancels (a surface far from the origin of its own frame) the normal's relative
            error grows by kappa_g = (|A|_F |x| + |b|) / |g| >= 1: the fresh term carries that factor.
  bound     E of the row, for every component of dx.  In the invariance scenes (a sphere about its centre, a cylinder about
            its axis, a plane within itself) the exact answer is 0, S is rounding-small and the bound is G N_OPS u kappa_g U:
            it scales with |u|, as it must.
Nothing in the bound comes from the device's output.  Every check prints its error / bound ratio before it asserts; the
worst one observed is recorded in profiles/sensitivity/README.md.

The sums: the device adds n terms per entry in a fixed tree (six butterfly steps in the wave, four waves, then the
workgroups, at most one after another), each term formed with at most ten rounded operations: against the longdouble sum of the
DEVICE's own Jacobian the error is at most (10 + 6 + 4 + chunks) u sum|term|."""
import numpy as np
import pytest

import sensitivity_reference as ref
import sensitivity_scenes as cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
N_OPS = 128


def device_frame(frame, counts):
    from pyrayt_amd.frame import DeviceFrame

    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, list(counts))


def table_and_parameters(parts, motions):
    from pyrayt_amd.scene import SceneSnapshot

    return ref.table_of(SceneSnapshot(parts).prims), [ref.parameter(m) for m in motions]


def budget(frame, info, dx, dd, parameters):
    """The bound E per row (module docstring), from the reference's dx, dd (K, R, 3) and its per-row geometry."""
    rows = len(frame)
    size = np.nan_to_num(np.max(np.linalg.norm(dx.astype(float), axis=2) + np.linalg.norm(dd.astype(float), axis=2), axis=0))
    moving = np.zeros(rows)
    for v, w, c, ids in parameters:
        on = np.isin(frame[:, 5], list(ids))
        speed = np.linalg.norm(np.asarray(v) + np.cross(np.asarray(w), frame[:, 9:12] - np.asarray(c)), axis=1) + np.linalg.norm(w)
        moving = np.maximum(moving, np.where(on, speed, 0.0))
    bound = np.zeros(rows)
    generation = frame[:, 0].astype(int)
    for g in range(generation.max() + 1 if rows else 0):
        here = np.flatnonzero(generation == g)
        c = 1.0 / np.abs(info["nd"][here])
        reach = np.maximum(1.0, np.abs(info["t"][here]))
        a, b = np.zeros(len(here)), np.zeros(len(here))
        before, size_before, moving_before, conditioning = np.zeros(len(here)), np.zeros(len(here)), np.zeros(len(here)), info["conditioning"][here].copy()
        if g > 0:
            p = info["previous"][here]
            kind, mu, q, gamma, kappa = info["kind"][here], info["mu"][here], 1.0 / info["ct"][here], np.abs(info["gamma"][here]), info["kappa"][p]
            a = np.where(kind == 1, mu * (2 + mu * q), np.where(kind == 2, 3.0, 1.0))
            b = np.where(kind == 1, kappa * (mu * (1 + mu * q) + gamma), np.where(kind == 2, 4 * kappa, 0.0))
            before, size_before, moving_before = bound[p], size[p], moving[p]
            conditioning = np.maximum(conditioning, info["conditioning"][p])
        gain = (1 + c) * reach * (1 + a + b)
        fresh = N_OPS * U * conditioning * gain * (size_before + size[here] + moving_before + moving[here])
        bound[here] = gain * before + fresh
    return bound


def reference_of(case, motions=None, parts=None):
    motions = case.motions if motions is None else motions
    table, parameters = table_and_parameters(case.parts if parts is None else parts, motions)
    info = {}
    dx, dd, count = ref.trace_tangents(case.frame, table, parameters, info)
    return dx, dd, count, budget(case.frame, info, dx, dd, parameters)


def check_against_reference(case, motions=None, surfaces=None, what=""):
    """Every surface of the frame as the selection: the Jacobian against the reference within the budget, NaN where the
    reference has NaN, the counters, and the sums against the longdouble sums of the device's own Jacobian."""
    motions = case.motions if motions is None else motions
    dx, dd, count, bound = reference_of(case, motions)
    frame = device_frame(case.frame, case.counts)
    K = len(motions)
    for surface in (np.unique(case.frame[:, 5]) if surfaces is None else surfaces):
        got = frame.sensitivity(int(surface), motions, case.parts)
        rows = got.rows().cpu().numpy()
        want_rows = np.flatnonzero(case.frame[:, 5] == surface)
        assert sorted(rows.tolist()) == want_rows.tolist()
        order = np.lexsort((case.frame[rows, 4], case.frame[rows, 0]))
        assert np.array_equal(order, np.arange(len(rows)))  # (one group: ordered by generation, then id)
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


def check_sums(got, frame, K, weight_column=1):
    jac = got.jacobian.cpu().numpy()
    rows = got.rows().cpu().numpy()
    x, w = frame[rows, 9:12], (frame[rows, weight_column] if weight_column is not None else np.ones(len(rows)))
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


# ---- the device against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CLOSED_FORMS)
def test_closed_form_scenes(name):
    case = cases.build(name, 65)
    dx, bound = check_against_reference(case)
    got = device_frame(case.frame, case.counts).sensitivity(case.surface, case.motions, case.parts)
    jac = got.jacobian.cpu().numpy()
    rows = got.rows().cpu().numpy()
    if getattr(case, "invariant", False):  # (the exact answer is 0: the budget alone, which scales with |u|)
        assert len(rows) > 30 and np.all(np.abs(jac) <= bound[rows][None, None, :]) and bound[rows].max() < 1e-8
    if name == "detector_shift":
        d = case.frame[rows, 12:15]
        normal = np.asarray(case.parts[0].get_orientation(), dtype=float).reshape(-1)[:3]
        want = (d * ((normal @ case.velocity) / (d @ normal))[:, None]).T
        assert np.all(np.abs(jac[0] - want) <= bound[rows][None, :] + 8 * U * np.abs(want))


@pytest.mark.parametrize("name", cases.SYSTEMS)
def test_systems(name):
    case = cases.build(name, 257)
    assert len(case.counts) >= (2 if name in ("scaled_cylinder", "paraboloid") else 3)
    if name == "stopped":
        assert case.counts[1] < case.counts[0]  # (the stop took rays in mid-path)
    if name == "prism":
        assert reference_of(case)[2]["n_reflections"] > 100  # (a face in total internal reflection)
    if name in ("scaled", "scaled_cylinder"):
        from pyrayt_amd.scene import SceneSnapshot

        a = SceneSnapshot(case.parts).prims["minv"][0].reshape(4, 4)[:3, :3]
        assert not np.allclose(a @ a.T, np.eye(3))  # (minv is not rigid)
    if name in ("scaled_cylinder", "paraboloid"):
        from pyrayt_amd.scene import SceneSnapshot

        kinds = {int(p["surface_id"]): int(p["type"]) for p in SceneSnapshot(case.parts).prims}
        met = [kinds[int(sid)] for sid in np.unique(case.frame[case.frame[:, 0] == 0, 5])]
        assert met == [ref.CYLINDER if name == "scaled_cylinder" else ref.PARABOLOID]  # (the wall, and it reflects)
        assert reference_of(case)[2]["n_reflections"] > 50
    check_against_reference(case)


def sixteen(case):
    from pyrayt_amd import Motion

    lens, det = case.parts
    e = np.eye(3)
    motions = [Motion(lens, translate=tuple(e[k])) for k in range(3)] + [Motion(lens, rotate=tuple(e[k])) for k in range(3)]
    motions += [Motion(det, translate=tuple(e[k])) for k in range(3)] + [Motion(det, rotate=tuple(e[k])) for k in range(3)]
    motions += [Motion(lens, translate=(0.3, -0.2, 0.5), rotate=(0.1, 0.7, -0.4), pivot=(0.5, 0.1, 0.0)),
                Motion(det, translate=(1, 1, 0), rotate=(0, 0.5, 0.5)),
                Motion(lens, rotate=(0, 0, 1), pivot=(-1.0, 0.0, 0.0)),
                Motion(lens.surface_ids[0][0], translate=(0, 1, 0))]
    assert len(motions) == 16
    return motions


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("K", [1, 6, 16])
def test_ray_counts_and_parameter_counts(n, K):
    case = cases.build("config2", n)
    motions = sixteen(case)
    chosen = motions[:K] if K > 1 else motions[4:5]
    check_against_reference(case, chosen, surfaces=[int(case.surface.get_id())], what=f" n={n}")


# ---- bit for bit --------------------------------------------------------------------------------------------------------------
def bits(got):
    return got.jacobian.cpu().numpy().tobytes(), np.asarray(got.sums).tobytes()


def test_two_runs_and_a_permutation_of_the_rows_give_the_same_bits():
    case = cases.build("stopped", 1000)
    frame = device_frame(case.frame, case.counts)
    first = frame.sensitivity(case.surface, case.motions, case.parts)
    again = frame.sensitivity(case.surface, case.motions, case.parts)
    assert bits(first) == bits(again)
    rng = np.random.default_rng(5)
    shuffled, start = case.frame.copy(), 0
    for count in case.counts:
        shuffled[start:start + count] = case.frame[start + rng.permutation(count)]
        start += count
    assert not np.array_equal(shuffled, case.frame)
    mixed = device_frame(shuffled, case.counts).sensitivity(case.surface, case.motions, case.parts)
    assert bits(mixed) == bits(first)
    assert np.array_equal(shuffled[mixed.rows().cpu().numpy()], case.frame[first.rows().cpu().numpy()])


def test_sixteen_parameters_in_one_call_are_the_same_bits_as_one_at_a_time():
    case = cases.build("config2", 257)
    motions = sixteen(case)
    frame = device_frame(case.frame, case.counts)
    all_at_once = frame.sensitivity(case.surface, motions, case.parts)
    together, K = all_at_once.jacobian.cpu().numpy(), len(motions)
    sums = all_at_once.sums[0]
    for k, motion in enumerate(motions):
        one = frame.sensitivity(case.surface, motion, case.parts)
        alone = one.jacobian.cpu().numpy()
        assert alone.shape == (1, 3, 257) and alone[0].tobytes() == together[k].tobytes(), k
        # ... and the sums the parameter has to itself: count, w, w x, w r^2; w dx_k; w r.dx_k; w dx_k.dx_k
        diagonal = 6 + 4 * K + k * (k + 1) // 2 + k
        shared = np.concatenate([sums[:6], sums[6 + 3 * k:9 + 3 * k], sums[6 + 3 * K + k:7 + 3 * K + k],
                                 sums[diagonal:diagonal + 1]])
        assert shared.tobytes() == one.sums[0].tobytes(), k


# ---- edge cases -----------------------------------------------------------------------------------------------------------------
def test_a_surface_left_out_of_system_is_counted_and_its_rays_are_nan_from_there():
    from pyrayt_amd import Motion

    case = cases.build("config2", 257)
    lens, det = case.parts
    frame = device_frame(case.frame, case.counts)
    got = frame.sensitivity(det, [Motion(det, translate=(1, 0, 0))], [det])  # (the lens is met first, and is not there)
    assert got.n_unknown == 257 and got.n_invalid == 0 and got.n_unfit == 0
    assert got.jacobian.shape == (1, 3, 257) and bool(torch.isnan(got.jacobian).all())
    assert got.count[0] == 0 and np.isnan(got.mean_square_gradient).all() and np.isnan(got.step()).all()
    # ... and with the detector left out the rays are good up to it: the lens's rows have numbers, the detector's none
    motion = Motion(lens, translate=(0, 1, 0))
    at_lens = frame.sensitivity(lens.surface_ids[0][0], [motion], [lens])
    assert at_lens.n_unknown == 257 and bool(torch.isfinite(at_lens.jacobian).all())  # (lost later, at the detector)
    at_det = frame.sensitivity(det, [motion], [lens])
    assert at_det.n_unknown == 257 and bool(torch.isnan(at_det.jacobian).all())


def test_a_parameter_that_moves_nothing_the_rays_meet_gives_exact_zeros_and_an_empty_selection_is_empty():
    import pyrayt_amd as prt

    case = cases.build("config2", 257)
    lens, det = case.parts
    far = prt.components.baffle((1, 1)).move(0, 50, 0)
    system = [lens, det, far]
    frame = device_frame(case.frame, case.counts)
    got = frame.sensitivity(det, [prt.Motion(far, translate=(1, 2, 3), rotate=(0.1, 0.2, 0.3)), case.motions[0]], system)
    jac = got.jacobian.cpu().numpy()
    assert jac.shape == (2, 3, 257) and not jac[0].any() and np.abs(jac[1]).max() > 0.1
    assert not got.centroid_gradient[0, 0].any() and got.mean_square_gradient[0, 0] == 0
    empty = frame.sensitivity(far, case.motions, system)
    assert empty.jacobian.shape == (3, 3, 0) and len(empty.rows()) == 0 and empty.count.tolist() == [0]
    assert np.isnan(empty.mean_square_gradient).all() and np.isnan(empty.centroid_gradient).all()
    assert np.isnan(empty.rms_radius_gradient).all() and np.isnan(empty.step()).all()
    assert len(empty.to_pandas()) == 0 and list(got.to_pandas().columns[:4]) == ["row", "dx_0", "dy_0", "dz_0"]


def test_groups_by_source_and_a_fixed_reference():
    case = cases.build("config2", 257)
    frame = device_frame(case.frame, case.counts)
    whole = frame.sensitivity(case.surface, case.motions, case.parts, weights=None, reference=(1.0, 0.0, 0.0))
    halves = frame.sensitivity(case.surface, case.motions, case.parts, weights=None, reference=(1.0, 0.0, 0.0),
                               rays_per_source=128)
    assert halves.sums.shape[0] == 3 and halves.count.tolist() == [128, 128, 1] and whole.count.tolist() == [257]
    rows = whole.rows().cpu().numpy()
    assert np.array_equal(halves.rows().cpu().numpy(), rows)
    x = case.frame[rows, 9:12]
    own = np.transpose(whole.jacobian.cpu().numpy(), (0, 2, 1))
    for g, part in enumerate((slice(0, 128), slice(128, 256), slice(256, 257))):
        want = ref.group_sums(x[part], np.ones(len(x[part])), own[:, part], (1.0, 0.0, 0.0))
        gradient = 2 * np.asarray(want["wrd"] / want["w"], dtype=float)
        assert np.allclose(halves.mean_square_gradient[g], gradient, rtol=1e-12, atol=1e-15)
        assert np.allclose(halves.normal_matrix[g], np.asarray(want["moments"] / want["w"], dtype=float), rtol=1e-12, atol=1e-15)


# ---- step() ------------------------------------------------------------------------------------------------------------------
def symmetric_rays():
    """A collimated beam along x on rings of radius 0.05 to 0.2, each ray with its mirror images in y and z: the spot of
    the centred lens is centred, and the mean square radius about the axis point is even in the decentre."""
    starts = []
    for radius in (0.05, 0.1, 0.15, 0.2):
        for angle in np.radians([10, 35, 60, 80]):
            y, z = radius * np.cos(angle), radius * np.sin(angle)
            starts += [(-1.0, y, z), (-1.0, -y, z), (-1.0, y, -z), (-1.0, -y, -z)]
    starts = np.array(starts)
    return cases.directed_rays(starts, np.tile([1.0, 0.0, 0.0], (len(starts), 1)))


def best_focus():
    """The plane x = const where the centred lens's spot has the least mean square radius, from the oracle's trace: the
    last segments (p, s = direction / its x part) give sum |p + t s|^2, least at t = -sum p.s / sum s.s."""
    import pyrayt_amd as prt

    if "focus" not in cases._CACHE:
        lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
        det = prt.components.baffle((1, 1)).move_x(3.0)
        frame, _ = cases.trace([lens, det], symmetric_rays())
        last = frame[frame[:, 5] == det.get_id()]
        p, s = last[:, 10:12], last[:, 13:15] / last[:, 12:13]
        cases._CACHE["focus"] = 3.0 - float(np.sum(p * s) / np.sum(s * s))
    return cases._CACHE["focus"]


def decentred(shift):
    import pyrayt_amd as prt

    focus = best_focus()
    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1).move_y(shift)
    det = prt.components.baffle((1, 1)).move_x(focus)
    frame, counts = cases.trace([lens, det], symmetric_rays())
    assert counts == [64, 64, 64]
    return device_frame(frame, counts).sensitivity(det, prt.Motion(lens, translate=(0, 1, 0)), [lens, det], weights=None,
                                                   reference=(focus, 0.0, 0.0))


def test_step_returns_a_decentred_lens():
    """A collimated beam brought to its focus on the detector, which stands in the plane of the least spot (best_focus):
    there the landing points have next to no residual about the axis point, Gauss-Newton is Newton's method but for the
    aberrations, and what one step leaves of a decentre of 1e-3 is of second order.  The bound on it is measured, not
    fixed: the next iteration's step.  With the reference's arithmetic on the CPU: step 1 = -1.000002010e-3, which
    leaves -2.0101e-9; step 2 = +2.0101e-9, larger than what was left by 6e-15 (the third step)."""
    first = decentred(1e-3)
    p1 = float(first.step()[0, 0])
    residual = 1e-3 + p1
    second = decentred(residual)
    p2 = float(second.step()[0, 0])
    print(f"step 1 {p1:.9e} (residual {residual:.6e}), step 2 {p2:.6e}, |residual| / |step 2| {abs(residual) / abs(p2):.9f}, "
          f"mean square {first.mean_square[0]:.9e} -> {second.mean_square[0]:.9e}")
    assert abs(residual) <= abs(p2)
    assert second.mean_square[0] <= first.mean_square[0]
    assert float(decentred(1e-3).step(damping=1.0)[0, 0]) == pytest.approx(p1 / 2, rel=1e-12)


# ---- trace_sensitivity ---------------------------------------------------------------------------------------------------------
def test_trace_sensitivity_is_sensitivity_of_the_traced_frame_bit_for_bit():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=1000)
    motions = [prt.Motion(lens, translate=(0, 1, 0)), prt.Motion(lens, rotate=(0, 0, 1)), prt.Motion(det, translate=(1, 0, 0))]
    traced = tracer.trace_sensitivity(det, motions)
    frame = tracer.trace_device()
    direct = frame.sensitivity(det, motions, tracer.get_system())
    assert traced.jacobian.shape == (3, 3, 1000) and bits(traced) == bits(direct)
    assert torch.equal(traced.rows(), direct.rows())
