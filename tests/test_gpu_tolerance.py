"""Monte Carlo tolerancing on the device (Sensitivity.tolerance, the entry points prt_frame_tolerance and
prt_frame_tolerance_moments, the kernels of prt_tolerance.hpp) against the longdouble reference of
tests/tolerance_reference.py, every Strehl ratio, amplitude and moment held to the error budget derived there: at the edges
of the LDS tile, the ray slices, the trial tiles and the column instantiations; the bit contracts; the zero trial against
``psf_gradient()``; compensators; one-hot trials against ``dstrehl``.  Each test prints its largest deviation / bound."""
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import helpers
import tolerance_reference as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
UNIT = 1000.0


def on(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    return DeviceFrame(on(np.asarray(frame, dtype=np.float64).T), counts)


def sensitivity_of(case, frame=None, rows=None, columns=None):
    """A Sensitivity that holds the case's designed wavefront and synthetic derivatives for its selected rows: what
    ``tolerance`` reads.  ``columns``: (K, n) in place of the case's dopd."""
    from pyrayt_amd.frame import Sensitivity

    dopd = case.dopd if columns is None else columns
    n_par, G = len(dopd), case.n_groups
    device = device_frame(case.frame if frame is None else frame)
    first = np.searchsorted(case.group, np.arange(G + 1)).astype(np.int64)
    inp = case.inputs(np.zeros(1), np.zeros(1))
    made = Sensitivity(on(np.zeros((n_par, 3, len(case.rows)))), on(case.rows if rows is None else rows),
                       np.zeros((G, 6 + 4 * n_par + n_par * (n_par + 1) // 2)), np.zeros((G, 3)), True, (0, 0, 0, 0),
                       [f"p{k}" for k in range(n_par)],
                       launch=dict(slopes=None, rows=device._contiguous_rows(), weights="intensity", group_first=first))
    made.wavefront = SimpleNamespace(reference=np.zeros((G, 3)), radius=inp.radius, pivot=np.zeros(G),
                                     pupil_radius=np.nan_to_num(inp.rho, nan=1.0), n_rays=np.diff(first), terms=0,
                                     _made_of=dict(axes=R.default_axes()))
    made.dopd, made.dfield, made.dpupil = on(dopd), on(dopd), on(np.zeros((n_par, 2, len(case.rows))))
    made.opd, made.pupil = on(inp.opd), on(inp.pupil)
    return made


def among_other_rows(case, filler, seed=17):
    """The case's frame with ``filler`` rows of another surface shuffled in: (frame, the selected rows' new numbers)."""
    rng = np.random.default_rng(seed)
    n = len(case.frame)
    at = np.sort(rng.permutation(n + filler)[:n])
    frame = np.zeros((n + filler, 15))
    frame[:, 1], frame[:, 2], frame[:, 3], frame[:, 5] = 1.0, 0.55, 1.0, R.ELSEWHERE
    frame[:, 4] = 10 ** 7 + np.arange(n + filler)
    frame[:, 9:12], frame[:, 12] = rng.normal(0, 1.0, (n + filler, 3)), 1.0
    frame[at] = case.frame
    return frame, at[case.rows]


def hold(family, what, got, re, im, bound):
    """|got - reference| <= bound at every value (NaN where, and only where, the reference is NaN); the figures printed."""
    got, bound = np.asarray(got), np.asarray(bound, dtype=np.float64)
    assert got.shape == re.shape == bound.shape, (family, what, got.shape, re.shape, bound.shape)
    nan = np.isnan(re.astype(np.float64))
    assert np.array_equal(np.isnan(np.real(got)), nan), (family, what, "NaN pattern")
    if nan.all():
        return 0.0
    deviation = T.deviation(got, re, im)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | ((deviation == 0) & (bound == 0)), 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[tolerance] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, {got.size} values)")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(case, trials, **kw):
    """``tolerance`` without compensators on per-group trials (G, M, C) that are the same for every group."""
    options = {k: kw.pop(k) for k in ("compensators", "follow") if k in kw}
    return sensitivity_of(case, **kw).tolerance(trials, world_unit_um=UNIT, **options)


def check(family, case, got, trials, columns=None):
    """The device's ToleranceRun (no compensators) against the reference on the same inputs: the counts exact, every
    amplitude, Strehl ratio and moment within its bound; the nominal trial is the all-zero one."""
    inp = case.tolerance_inputs(columns)
    G, L = case.n_groups, len(inp.wavelengths)
    handed = np.broadcast_to(np.vstack([trials, np.zeros((1, trials.shape[1]))])[None], (G, len(trials) + 1, trials.shape[1]))
    ref = T.tolerance_reference(inp, handed, n_slices=T.slices(len(case.rows), G * L, cus()))
    for name in ("n_rays", "n_missed", "n_unfollowed"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), (family, name, getattr(got, name), getattr(ref, name))
    amplitude = np.concatenate([got.amplitude, got.nominal.amplitude[:, :, None]], axis=2)
    strehl = np.concatenate([got.strehl, got.nominal.strehl[:, None]], axis=1)
    worst = hold(family, "amplitude", amplitude, *ref.amplitude, ref.amplitude_bound)
    worst = max(worst, hold(family, "strehl", strehl, ref.strehl, None, ref.strehl_bound))
    moments, bound = T.moments_reference(inp)
    worst = max(worst, hold(family, "moments", got.moments, moments, None, bound))
    assert np.array_equal(got.moments[:, :3], moments[:, :3].astype(float))
    # sum a and (s sum a)^2: sqrt(w), then ``depth`` additions (a thread's rays, the tree, the slices), the product, the square
    n_slices = T.slices(len(case.rows), G * L, cus())
    depth = -(-int(ref.n_rays.max()) // (n_slices * R.K.kPsfBlock)) + int(np.log2(R.K.kPsfBlock)) + n_slices
    hold(family, "record sum a and D", got.record[:, :, 3:], ref.record[:, :, 3:], None,
         (2 * depth + 10) * R.U64 * np.abs(ref.record[:, :, 3:]).astype(float))
    return ref, worst


def outputs(got):
    return dict(strehl=got.strehl, amplitude=got.amplitude, nominal=got.nominal.strehl, record=got.record,
                moments=got.moments, rms_opd=got.rms_opd)


def assert_same_bits(got, want, what):
    parts = lambda x: np.ascontiguousarray(x).view(np.float64) if np.iscomplexobj(x) else np.ascontiguousarray(x)  # noqa: E731
    helpers.assert_same_bits(parts(got), parts(want), what)


def same_bits(a, b, what):
    for key, value in outputs(a).items():
        assert_same_bits(value, outputs(b)[key], f"{what}: {key}")


# ---- the kernels against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.SIZES)
def test_ray_tiles_and_slices_alone_and_among_other_rows(n):
    """Rays of a bucket about the LDS tile (kTolRays = 128), the moments' tile (64) and the slice (kTolMinSlice = 2048;
    4097 rays are two slices of 2049 and 2048, and three chunks of the moments): alone in the frame and among 4196 rows
    of another surface, which change nothing -- the partition follows the selection alone -- so the same bits."""
    assert (T.K.kTolRays, T.K.kTolMinSlice, T.K.kTolMomentChunk) == (128, 2048, 2048)
    assert T.slices(n, 1, cus()) == (2 if n == 4097 else 1)
    case = T.tolerance_case([[n]], 3, seed=100 + n)
    trials = T.random_trials(1, 5, 3, seed=n)[0]
    got = run(case, trials)
    check(f"{n} rays", case, got, trials)
    frame, rows = among_other_rows(case, 2 * 2048 + 100)
    other = run(case, trials, frame=frame, rows=rows)
    same_bits(got, other, f"{n} rays among other rows")


@pytest.mark.parametrize("n_trials", T.TRIAL_COUNTS)
def test_trial_counts(n_trials):
    """M about the trials of a thread (kTolTrials = 2) and of a workgroup (kTolTile = 512), 1 024 and 1 025: ``tolerance``
    appends the nominal trial, so the kernel runs M + 1 -- 2, 3, 4, 511 .. 514, 1 025 and 1 026; its own n_trials = 1 is
    test_one_trial_through_the_entry_point_itself."""
    assert (T.K.kTolTrials, T.K.kTolTile) == (2, 512)
    case = T.tolerance_case([[257]], 3, seed=30 + n_trials % 97)
    trials = T.random_trials(1, n_trials, 3, seed=n_trials)[0]
    got = run(case, trials)
    assert got.strehl.shape == (1, n_trials) and got.amplitude.shape == (1, 1, n_trials)
    check(f"M = {n_trials}", case, got, trials)


@pytest.mark.parametrize("n_columns", T.COLUMN_COUNTS)
def test_column_counts(n_columns):
    """C about the steps of k_tol_sum<CP> (4, 8, 12, 16, 20): 1 and 3 in <4> with empty columns, 4 whole, 5 in <8>, 16 whole,
    19 and 20 in <20>; the moments' entries grow to 253, a thread each."""
    assert T.template_columns(n_columns) == {1: 4, 3: 4, 4: 4, 5: 8, 16: 16, 19: 20, 20: 20}[n_columns]
    case = T.tolerance_case([[300]], n_columns, seed=60 + n_columns)
    trials = T.random_trials(1, 7, n_columns, scale=0.4 / np.sqrt(n_columns), seed=n_columns)[0]
    got = run(case, trials)
    assert got.moments.shape == (1, 3 + (n_columns + 2) * (n_columns + 3) // 2)
    check(f"C = {n_columns}", case, got, trials)


def test_two_wavelengths_two_groups_one_empty_and_rays_left_out():
    """Two groups, the second without rays (NaN), two wavelengths; per bucket 3 rays with a NaN OPD (n_missed) and 4 with
    a NaN in one column (n_unfollowed): out for every column and trial, counted, and the sums as the reference has them
    without those rays."""
    case = T.tolerance_case([[300, 170], [0, 0]], 5, seed=81, wavelengths=(0.45, 0.65), missed=3, unfollowed=4)
    trials = T.random_trials(1, 9, 5, seed=4)[0]
    got = run(case, trials)
    check("buckets", case, got, trials)
    assert got.n_missed.tolist() == [[3, 3], [0, 0]] and got.n_unfollowed.tolist() == [[4, 4], [0, 0]]
    assert got.n_rays.tolist() == [[293, 163], [0, 0]]
    assert np.all(np.isfinite(got.strehl[0])) and np.all(np.isfinite(got.amplitude[0])) and np.all(np.isfinite(got.rms_opd[0]))
    for value in (got.strehl[1], got.amplitude[1], got.rms_opd[1], got.nominal.strehl[1:]):
        assert np.all(np.isnan(value))
    assert got.moments[:, :3].tolist() == [[456, 6, 8], [0, 0, 0]] and np.isnan(got.yield_()[1])
    table = got.to_pandas()
    assert len(table) == 18 and list(table.columns[:5]) == ["source_id", "trial", "strehl", "rms_opd", "rms_radius"]


def test_one_trial_through_the_entry_point_itself():
    """prt_frame_tolerance called directly with M = 1 (``tolerance`` never does: it appends the nominal trial): one lane of
    one wave busy.  Held to the bound, and the same bits as the trial has in a ``tolerance`` run."""
    from pyrayt_amd import engine

    case = T.tolerance_case([[300, 170]], 3, seed=83, wavelengths=(0.45, 0.65))
    trials = T.random_trials(1, 1, 3, seed=12)
    sens = sensitivity_of(case)
    rows, first = sens._launch["rows"], np.ascontiguousarray(sens._launch["group_first"], dtype=np.int64)
    lam = np.array([0.45, 0.65])
    n, C, M, L = len(case.rows), 3, 1, 2
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=rows.device)  # noqa: E731
    strehl, amplitude, record, handed = f64(1, M), f64(1, L, M, 2), f64(1, L, 5), on(trials)
    lib = engine.library()
    work = torch.empty(int(engine._check(lib.prt_frame_tolerance_workspace_bytes(n, 1, C, L, M))), dtype=torch.uint8,
                       device=rows.device)
    opd, columns = sens.opd.contiguous(), sens.dopd.contiguous()
    engine._check(lib.prt_frame_tolerance(0, rows.data_ptr(), rows.stride(0), rows.shape[1], sens._selected.data_ptr(), n,
                                          first.ctypes.data, 1, 1, opd.data_ptr(), columns.data_ptr(), C, lam.ctypes.data, L,
                                          UNIT, handed.data_ptr(), M, strehl.data_ptr(), amplitude.data_ptr(),
                                          record.data_ptr(), work.data_ptr(), engine._stream_ptr(torch, rows.device)))
    ref = T.tolerance_reference(case.tolerance_inputs(), trials, n_slices=1)
    pair = amplitude.cpu().numpy()
    hold("M = 1, direct", "amplitude", pair[..., 0] + 1j * pair[..., 1], *ref.amplitude, ref.amplitude_bound)
    hold("M = 1, direct", "strehl", strehl.cpu().numpy(), ref.strehl, None, ref.strehl_bound)
    through = sens.tolerance(trials[0], world_unit_um=UNIT)
    assert_same_bits(strehl.cpu().numpy(), through.strehl, "M = 1 directly and through tolerance()")
    assert record.cpu().numpy()[0, :, 0].tolist() == [300, 170]


def test_rays_of_negative_and_infinite_weight_are_missed():
    """The PSF's rule on the weight: a ray whose weight is negative, infinite or NaN is left out and counted as missed,
    in both entries; the sums are the reference's without it."""
    case = T.tolerance_case([[200]], 2, seed=84)
    weight = case.tolerance_inputs().weight.copy()
    frame = case.frame.copy()
    for k, bad in zip((5, 77, 140), (-1.0, np.inf, np.nan)):
        weight[k] = bad
        frame[case.rows[k], 1] = bad
    trials = T.random_trials(1, 3, 2, seed=13)[0]
    got = run(case, trials, frame=frame)
    inp = case.tolerance_inputs(weight=weight)
    ref = T.tolerance_reference(inp, np.vstack([trials, np.zeros((1, 2))])[None])
    assert got.n_missed.tolist() == [[3]] and got.n_rays.tolist() == [[197]] and got.moments[0, :3].tolist() == [197, 3, 0]
    hold("weights", "strehl", np.concatenate([got.strehl, got.nominal.strehl[:, None]], axis=1), ref.strehl, None, ref.strehl_bound)
    moments, bound = T.moments_reference(inp)
    hold("weights", "moments", got.moments, moments, None, bound)


# ---- the bit contracts ------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    case = T.tolerance_case([[2500, 1700], [300, 0]], 9, seed=97, wavelengths=(0.5, 0.6), missed=2)
    trials = T.random_trials(1, 40, 9, scale=0.15, seed=5)[0]
    first = run(case, trials, compensators=("tilt", 2))
    second = run(case, trials, compensators=("tilt", 2))
    same_bits(first, second, "run to run")
    assert_same_bits(first.compensation, second.compensation, "run to run: compensation")


def test_a_trial_alone_has_the_bits_it_has_among_1025_and_at_any_place():
    """A trial's arithmetic does not depend on the other trials, on its thread or on its workgroup: alone (M = 1, and
    the nominal trial behind it), among 1 025 at place 700 (the second tile, the second trial of a thread) and moved to
    place 3 (the first tile, the first of another thread)."""
    case = T.tolerance_case([[700]], 5, seed=56)
    trials = T.random_trials(1, 1025, 5, seed=6)[0]
    among = run(case, trials)
    alone = run(case, trials[700:701])
    moved = trials.copy()
    moved[[3, 700]] = moved[[700, 3]]
    elsewhere = run(case, moved)
    for name in ("strehl", "amplitude"):
        value = getattr(among, name)[..., 700]
        assert_same_bits(getattr(alone, name)[..., 0], value, f"a trial alone: {name}")
        assert_same_bits(getattr(elsewhere, name)[..., 3], value, f"a trial moved: {name}")
        assert_same_bits(getattr(elsewhere, name)[..., 5:700], getattr(among, name)[..., 5:700], f"the others: {name}")
    assert_same_bits(alone.nominal.strehl, among.nominal.strehl, "the nominal trial")


@pytest.mark.parametrize("n_columns", (3, 4, 16))
def test_a_zero_column_appended_changes_no_bit(n_columns):
    """A finite column whose trial values are all 0.0: fma(e, 0, phi) is phi.  From 4 to 5 and from 16 to 17 columns the
    call also moves to the next instantiation of k_tol_sum, whose own empty columns are the same zeros."""
    case = T.tolerance_case([[300]], n_columns, seed=70 + n_columns)
    trials = T.random_trials(1, 11, n_columns, scale=0.2, seed=7)[0]
    got = run(case, trials)
    extra = np.random.default_rng(8).normal(0.0, 1e-3, (1, len(case.rows)))
    wider = run(case, np.hstack([trials, np.zeros((11, 1))]), columns=np.vstack([case.dopd, extra]))
    for name in ("strehl", "amplitude", "record"):
        assert_same_bits(getattr(wider, name), getattr(got, name), f"a zero column: {name}")
    assert_same_bits(wider.nominal.strehl, got.nominal.strehl, "a zero column: the nominal trial")


# ---- against the passes that were there ---------------------------------------------------------------------------------------
def test_the_zero_trial_is_psf_gradients_strehl():
    """``nominal.strehl`` without compensators against ``psf_gradient().strehl`` of the same Sensitivity: that one is summed
    with fp64 sincospi, so the bound is this kernel's alone (and the fp64 sum's own, ``gradient_reference``'s)."""
    import psf_gradient_reference as P

    case = T.tolerance_case([[2500, 1200], [64, 0]], 3, seed=33, wavelengths=(0.5, 0.6))
    sens = sensitivity_of(case)
    got = sens.tolerance(np.zeros((1, 3)), world_unit_um=UNIT)
    grad = sens.psf_gradient(world_unit_um=UNIT, pixels=(1, 1), pixel_size=(1e-3, 1e-3))
    inp = case.tolerance_inputs()
    ref = T.tolerance_reference(inp, np.zeros((2, 1, 3)), n_slices=T.slices(len(case.rows), 4, cus()))
    fp64 = P.gradient_reference(case.inputs(np.zeros(1), np.zeros(1)), case.dopd, None,
                                slices=P.slices(len(case.rows), 4, 1, cus()))
    hold("zero trial", "strehl against psf_gradient()", got.nominal.strehl, grad.strehl.astype(LD), None,
         ref.strehl_bound[:, 0] + fp64.strehl_bound)
    assert_same_bits(got.strehl[:, 0], got.nominal.strehl, "the zero trial and the nominal one")
    assert np.array_equal(got.n_rays, grad.n_rays)


def covariance_bound(moments, bound, C):
    """Entrywise bound of the covariance ``moment_covariance`` forms from moments that are within ``bound`` (one group)."""
    n = C + 1
    sw, b_w = float(moments[3]), bound[3]
    mean, b_mean = (moments[4:4 + n] / moments[3]).astype(float), bound[4:4 + n]
    lower, b_lower = np.zeros((n, n)), np.zeros((n, n))
    lower[np.tril_indices(n)] = moments[4 + n:].astype(float)
    b_lower[np.tril_indices(n)] = bound[4 + n:]
    second, b_second = lower + np.tril(lower, -1).T, b_lower + np.tril(b_lower, -1).T
    d_mean = (b_mean + np.abs(mean) * b_w) / sw
    return ((b_second + np.abs(second) / sw * b_w) / sw + np.outer(np.abs(mean), d_mean) + np.outer(d_mean, np.abs(mean))
            + np.outer(d_mean, d_mean)) * 1.01


def test_tilt_trials_are_taken_out_by_the_tilt_compensator():
    """Two parameters that ARE tilts (dopd = -p1 / R and -p2 / R): a trial (du, dv) moves the image off P.  With
    compensators=("tilt",) the Strehl ratio returns to ``nominal`` within the bound and the compensation is the nominal
    one less the applied shift -- to the conditioning of the 2 x 2 solve: first-order perturbation of A q = -b by the
    moments' own bound, in the columns scaled to unit variance.  Without compensators the Strehl ratio does not return."""
    from pyrayt_amd.frame import moment_covariance

    case = T.tolerance_case([[900]], 2, seed=44)
    inp0 = case.inputs(np.zeros(1), np.zeros(1))
    tilt = -(inp0.pupil * inp0.rho[case.group][:, None] / inp0.radius[case.group][:, None]).T
    lam_f = 0.55e-3 * 10.0
    rng = np.random.default_rng(9)
    angle, size = rng.uniform(0, 2 * np.pi, 12), rng.uniform(0.8, 1.5, 12)  # (shifts of 0.8 to 1.5 lambda F: off the core)
    trials = np.stack([size * np.cos(angle), size * np.sin(angle)], axis=1) * lam_f
    plain = run(case, trials, columns=tilt)
    got = run(case, trials, columns=tilt, compensators=("tilt",))
    assert got.compensation.shape == (1, 12, 2) and got.compensators == ("tilt",)
    inp = case.tolerance_inputs(np.vstack([tilt, tilt]))
    q = np.concatenate([np.hstack([trials, got.compensation[0]]), np.hstack([np.zeros((1, 2)), got.nominal.compensation])])
    ref = T.tolerance_reference(inp, q[None], n_slices=1)
    strehl = np.concatenate([got.strehl, got.nominal.strehl[:, None]], axis=1)
    hold("tilt", "strehl at the device's compensation", strehl, ref.strehl, None, ref.strehl_bound)
    back = np.abs(got.strehl[0] - got.nominal.strehl[0])
    # (both within their bounds of the reference, whose own values differ by what the solve's rounding leaves)
    allowed = ref.strehl_bound[0, :-1] + ref.strehl_bound[0, -1] + np.abs(ref.strehl[0, :-1] - ref.strehl[0, -1]).astype(float)
    print(f"[tolerance] tilt: |strehl - nominal| <= {back.max():.3e} compensated (allowed {allowed.min():.3e}), "
          f"{np.abs(plain.strehl[0] - plain.nominal.strehl[0]).min():.3e} at the least without")
    assert np.all(back <= allowed)
    assert np.all(np.abs(plain.strehl[0] - plain.nominal.strehl[0]) > 0.05)
    # the compensation: nominal - shift, within cond * (what the moments' bound leaves in A and b)
    moments, bound = T.moments_reference(inp)
    cov = moment_covariance(moments[0], 4).astype(float)
    d_cov = covariance_bound(moments[0], bound[0], 4)
    free = [3, 4]
    scale = 1 / np.sqrt(np.diag(cov)[free])
    a = cov[np.ix_(free, free)] * np.outer(scale, scale)
    d_a = d_cov[np.ix_(free, free)] * np.outer(scale, scale)
    total = np.abs(got.nominal.compensation[0]).max() + np.abs(trials).max()
    d_b = (d_cov[free, 0] + d_cov[np.ix_(free, [1, 2])].sum(axis=1) * np.abs(trials).max()) * scale
    slack = 2 * np.linalg.norm(np.linalg.inv(a), 2) * (np.linalg.norm(d_b) + np.linalg.norm(d_a) * np.linalg.norm(total / scale)) * scale.max()
    miss = np.abs(got.compensation[0] - (got.nominal.compensation[0] - trials))
    print(f"[tolerance] tilt: cond {np.linalg.cond(a):.2f}, |compensation - (nominal - shift)| <= {miss.max():.3e}, "
          f"allowed {slack:.3e} of shifts up to {np.abs(trials).max():.3e}")
    assert slack < 1e-6 * np.abs(trials).max() and np.all(miss <= slack)


def test_rms_opd_is_the_sample_statistic_on_the_moved_opds():
    """``rms_opd`` (the quadratic form of the device's moments at the compensated coefficients) against the reference's
    weighted standard deviation of OPD + sum_c q_c x_c over the kept rays, q the coefficients the run itself reports;
    the bound: the moments' own, through the form, |d var| <= sum |v_i| |v_j| dCov_ij, over 2 rms."""
    from pyrayt_amd.frame import moment_covariance

    case = T.tolerance_case([[1500, 900], [40, 0]], 4, seed=45, wavelengths=(0.5, 0.6), missed=2, unfollowed=1)
    trials = T.random_trials(1, 10, 4, scale=0.3, seed=10)[0]
    got = run(case, trials, compensators=(1, "tilt", "focus"))
    assert got.compensation.shape == (2, 10, 4) and np.all(np.isnan(got.rms_radius))
    inp0 = case.inputs(np.zeros(1), np.zeros(1))
    p = inp0.pupil * inp0.rho[case.group][:, None]
    radius = inp0.radius[case.group]
    p3 = -np.sqrt(radius ** 2 - (p * p).sum(axis=1))  # (the rays run towards +x: u.a > 0)
    columns = np.vstack([case.dopd, (-p / radius[:, None]).T, (-p3 / radius)[None, :]])
    inp = case.tolerance_inputs(columns)
    q = np.zeros((2, 11, 7))
    q[:, :10, :4] = trials
    comp = np.concatenate([got.compensation, got.nominal.compensation[:, None]], axis=1)
    q[:, :, 1] += comp[:, :, 0]
    q[:, :, 4:] = comp[:, :, 1:]
    want = T.rms_opd_reference(inp, q)
    moments, bound = T.moments_reference(inp)
    allowed = np.zeros((2, 11))
    for g in range(2):
        v = np.abs(np.concatenate([np.ones((11, 1)), q[g]], axis=1))
        d_var = np.einsum("mi,ij,mj->m", v, covariance_bound(moments[g], bound[g], 7), v)
        allowed[g] = d_var / (2 * want[g].astype(float)) + 4 * R.U64 * want[g].astype(float)
    rms = np.concatenate([got.rms_opd, got.nominal.rms_opd[:, None]], axis=1)
    hold("rms_opd", "against the sample statistic", rms, want, None, allowed)
    assert np.all(got.rms_opd[0] <= sensitivity_of(case).tolerance(trials, world_unit_um=UNIT).rms_opd[0] * (1 + 1e-12))


def test_one_hot_trials_follow_dstrehl():
    """(strehl(h) - strehl(-h)) / 2h of one-hot trials against ``psf_gradient().dstrehl``, inside the Richardson gap of
    h and h / 2 (the rule of test_gpu_psf_gradient.richardson): |dstrehl - D(h/2)| <= |D(h) - D(h/2)| + floor, the gap
    under 1 % of the largest |dstrehl| and ten times the floor, floor = what the fp32 phasors leave in the two
    differences (the Strehl bounds over h and over h / 2)."""
    case = T.tolerance_case([[1500]], 3, seed=47)
    sens = sensitivity_of(case)
    grad = sens.psf_gradient(world_unit_um=UNIT, pixels=(1, 1), pixel_size=(1e-3, 1e-3))
    h = 2.0 ** -7  # (the largest power of two at which the reference's own gap is under 1 %; ten times the floor holds from 2^-9 up)
    trials = np.zeros((12, 3))
    for k in range(3):
        trials[4 * k:4 * k + 4, k] = (h, -h, h / 2, -h / 2)
    got = sens.tolerance(trials, world_unit_um=UNIT)
    ref = T.tolerance_reference(case.tolerance_inputs(), trials[None], n_slices=1)
    s, b = got.strehl[0].reshape(3, 4), ref.strehl_bound[0].reshape(3, 4)
    coarse, fine = (s[:, 0] - s[:, 1]) / (2 * h), (s[:, 2] - s[:, 3]) / h
    floor = (b[:, 0] + b[:, 1]) / (2 * h) + (b[:, 2] + b[:, 3]) / h
    gap, miss, scale = np.abs(coarse - fine), np.abs(grad.dstrehl[0] - fine), np.abs(grad.dstrehl[0]).max()
    print(f"[tolerance] one-hot: dstrehl {grad.dstrehl[0]}, gap {gap}, floor {floor}, |dstrehl - D(h/2)| {miss}")
    assert np.all(miss <= gap + floor)
    assert gap.max() <= 0.01 * scale and gap.max() >= 10 * floor.max()


# ---- the tracer ---------------------------------------------------------------------------------------------------------------
def test_trace_tolerance_is_trace_sensitivity_then_tolerance():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=257)
    parameters = [prt.Motion(lens, translate=(0, 1, 0)), prt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)),
                  prt.IndexChange(lens)]
    tolerances = prt.Tolerances([2e-3, 1e-3, 5e-4], "normal", seed=3)
    tracer.trace()
    before = tracer.get_results().copy()
    got = tracer.trace_tolerance(det, parameters, tolerances, trials=50, world_unit_um=UNIT)
    assert tracer.get_results().equals(before)  # (the tracer's last result is left as it was)
    sens = tracer.trace_sensitivity(det, parameters, wavefront=True)
    want = sens.tolerance((tolerances, 50), world_unit_um=UNIT, compensators=("tilt", "focus"))
    assert isinstance(got, prt.ToleranceRun) and got.strehl.shape == (1, 50) and got.compensation.shape == (1, 50, 3)
    same_bits(got, want, "trace_tolerance")
    assert_same_bits(got.compensation, want.compensation, "trace_tolerance: compensation")
    assert np.array_equal(got.trials, tolerances.sample(50)) and got.parameters == tuple(parameters)
    assert got.n_rays.sum() == 257 and np.all(np.isfinite(got.strehl)) and np.all(np.isnan(got.rms_radius))
    assert np.all((got.strehl > 0) & (got.strehl <= 1 + 1e-6)) and 0.0 <= got.yield_(0.8)[0] <= 1.0
    free = sens.tolerance((tolerances, 50), world_unit_um=UNIT)
    assert np.all(np.isfinite(free.rms_radius)) and np.all(got.rms_opd <= free.rms_opd * (1 + 1e-9))
    table = tracer.trace_tolerance(det, parameters, None, trials=tolerances.sensitivity_table(), world_unit_um=UNIT,
                                   compensators=()).table()
    assert sorted(table["parameter"].tolist()) == [0, 1, 2] and np.all(np.diff(table["worst"]) >= 0)
    with pytest.raises(ValueError, match="wavefront="):
        tracer.trace_sensitivity(det, parameters).tolerance((tolerances, 5), world_unit_um=UNIT)
    with pytest.raises(ValueError, match="WavelengthChange"):
        tracer.trace_tolerance(det, parameters + [prt.WavelengthChange()], [1e-3] * 4, trials=5, world_unit_um=UNIT)


# ---- end to end: the linear ray model against re-traced systems -----------------------------------------------------------------
# micrometres per world unit, as tests/test_gpu_psf_gradient.py takes them for the same scenes
E2E_UNIT = {"singlet": 1000.0, "two_fields": 1000.0, "dish_axial": 1e6}


@pytest.mark.parametrize("name", ("singlet", "two_fields", "dish_axial"))
def test_end_to_end_the_error_of_the_linear_ray_model_is_of_second_order(name):
    """4 trials with every parameter that can be applied to a built system non-zero at once (an IndexChange cannot:
    tests/tolerance_scenes.py), against the Strehl ratio ``psf()`` gives on the C oracle's re-trace of each perturbed
    system with P and R held.  The linear ray model's error is of second order in the trial, so the test is on its
    order: with e(h) = max |device - oracle| over the trials scaled by h, e(h/2) <= e(h) / 3 (pure second order gives
    1 / 4; the margin is for the third-order terms) and e(h) >= 10 x the device's bound, so that e is not rounding.  h
    comes from the sensitivity pass alone: every parameter is scaled by the spread of its own dopd, the four sign
    patterns are drawn, and h puts the largest phase change of a ray (about its group's mean) at 0.4 rad.  Printed
    beside e(h), not asserted: the error of the linearised merit strehl + dstrehl . p on the same trials.  The
    longdouble reference alone meets both conditions against the oracle on the CPU, with the same figures
    (tests/test_host_tolerance.py, the test of the same name); no parameter but the IndexChange had to be left out.
    Observed (MI355X): e(h/2) / e(h) 0.225, 0.216 and 0.126; e(h) 9.0e-6, 2.1e-6 and 1.1e-3, 16 to 1 100 times the bound; the
    linearised merit misses by 3.0e-4, 3.3e-4 and 3.1e-2."""
    import opd_scenes
    import tolerance_scenes
    from test_gpu_psf_gradient import traced_frame

    case = opd_scenes.build(name, 257)
    per_source = getattr(case, "rays_per_source", None)
    kw = dict(rays_per_source=per_source, n_groups=2) if per_source else {}
    G = 2 if per_source else 1
    dev = traced_frame(case)
    wave = dev.wavefront(case.surface, weights="intensity", **kw)
    sens = dev.sensitivity(case.surface, list(case.parameters), case.parts, wavefront=wave, **kw)
    assert not (sens.n_unknown or sens.n_invalid or sens.n_unfit)
    lam, unit = float(np.unique(case.frame[:, 2])[0]), E2E_UNIT[name]
    s = unit / lam
    dopd = sens.dopd.cpu().numpy()
    rows = sens.rows().cpu().numpy()
    group = np.floor(case.frame[rows, 4] / per_source).astype(int) if per_source else np.zeros(len(rows), int)
    K, live = len(case.parameters), tolerance_scenes.applicable(case.parameters)
    assert len(live) >= 2

    def spread(x):
        return max(np.abs(x[group == g] - x[group == g].mean()).max() for g in range(G))

    signs = np.random.default_rng(11).choice([-1.0, 1.0], (4, len(live)))
    direction = np.zeros((4, K))
    direction[:, live] = signs / np.array([spread(dopd[k]) for k in live])
    h = 0.4 / (2 * np.pi * s * max(spread(direction[m] @ dopd) for m in range(4)))
    grad = sens.psf_gradient(world_unit_um=unit, pixels=(1, 1))

    def error(scale):
        trials = direction * (h * scale)
        got = sens.tolerance(trials, world_unit_um=unit)
        want = np.empty((G, 4))
        for m in range(4):
            moved = tolerance_scenes.build(name, 257, trials[m])
            assert moved.counts == case.counts, f"trial {m} at {scale} h: rays were lost or gained"
            want[:, m] = traced_frame(moved).psf(moved.surface, reference=wave.reference, radius=wave.radius,
                                                 world_unit_um=unit, pixels=1, **kw).strehl
        linear = grad.strehl[:, None] + grad.dstrehl @ trials.T
        return np.abs(got.strehl - want).max(), np.abs(linear - want).max(), got, trials

    (e1, l1, got, trials), (e2, l2, _, _) = error(1.0), error(0.5)
    inp = T.tolerance_inputs(group, case.frame[rows, 2], sens.opd.cpu().numpy(), case.frame[rows, 1], dopd, [lam], unit, G)
    ref = T.tolerance_reference(inp, np.broadcast_to(trials[None], (G, 4, K)), n_slices=1)
    hold(f"{name} traced", "strehl", got.strehl, ref.strehl, None, ref.strehl_bound)
    bound = float(ref.strehl_bound.max())
    print(f"[tolerance] {name}: h puts 0.4 rad on the worst ray; e(h) {e1:.3e}, e(h/2) {e2:.3e} (ratio {e2 / e1:.3f}), device "
          f"bound {bound:.3e}; strehl + dstrehl . p misses by {l1:.3e} at h and {l2:.3e} at h / 2")
    assert e1 >= 10 * bound, (name, e1, bound)
    assert e2 <= e1 / 3, (name, e1, e2)
