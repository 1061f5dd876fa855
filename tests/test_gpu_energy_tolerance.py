"""Monte Carlo tolerancing of the enclosed energy on the device (Sensitivity.energy_tolerance, the entry point
prt_frame_energy_tolerance, the kernels of prt_energy_tolerance.hpp) against tests/energy_tolerance_reference.py: every
count and radius held to the exact integer inequalities derived there, at radii where no ray lies in its band, so the counts
are compared for equality; at the edges of the LDS tile, the ray slices, the trial tiles, the instantiations, the output
chunks and the fraction tiles; exact arithmetic with ties on a dyadic lattice; the bit contracts; the moments against
mtf_tolerance(); the nominal trial against enclosed_energy(); the tracer; and, end to end, against the enclosed energy of
the C oracle's re-traces of the perturbed systems."""
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import energy_tolerance_reference as ET
import mtf_tolerance_reference as T
from test_gpu_mtf_gradient import among_other_rows, assert_same_bits, device_frame, sensitivity_of, traced_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
FRACTIONS = (0.5, 0.8, 0.9)
FOCUS = (0.0, 0.05)
KEYS = ("count", "energy", "radius", "moments", "focus_shift", "record", "total")


def entry(sens, trials, radii, fractions=FRACTIONS, focus=FOCUS, shape="circle", follow=True, compensate=False, centre=None):
    """prt_frame_energy_tolerance itself on ``trials`` (G, M, K) as they are (no nominal trial appended)."""
    from pyrayt_amd import energy_tolerance
    from pyrayt_amd.frame import _group_points, pupil_axes

    head = sens._selected_rows()
    trials = np.array(trials, dtype=np.float64, order="C")
    centres = None if centre is None else _group_points(centre, head.n_groups, head.rows.device, "centre")
    as_array = lambda v: np.zeros(0) if v is None else np.asarray(v, dtype=np.float64)  # noqa: E731
    count, energy, radius, moments, shift, record = energy_tolerance.device_run(
        head, sens.jacobian, sens.slopes, centres, pupil_axes(None, None), shape, follow, as_array(radii), as_array(fractions),
        np.asarray(focus, dtype=np.float64), trials, compensate)
    return SimpleNamespace(count=count, energy=energy, radius=radius, moments=moments, focus_shift=shift,
                           record=record[:, :7], total=record[:, 7].copy().view(np.uint64))


def whole(run):
    """An EnergyToleranceRun's arrays with the nominal trial last, as the entry point wrote them."""
    join = lambda name: np.concatenate([getattr(run, name), getattr(run.nominal, name)[:, None]], axis=1)  # noqa: E731
    return SimpleNamespace(count=join("count"), energy=join("energy"), radius=join("radius"), moments=run.moments,
                           focus_shift=join("focus_shift"), record=run.record, total=run.total)


def same_bits(a, b, what, keys=KEYS):
    for key in keys:
        assert_same_bits(getattr(a, key), getattr(b, key), f"{what}: {key}")


def radii_for(case, trials, count, focus=FOCUS, shape="circle", follow=True, centre=None, compensate=False, **more):
    """``count`` clear radii from the reference on its own moments and focus shifts (the device's differ from them by
    roundings, a millionth of the gap: ``check`` asserts on the device's own that no ray lies in a band)."""
    ref = ET.reference_of(case, trials, focus, shape, follow, centre=centre, compensate=compensate, **more)
    return ET.clear_radii(ref, count)


def check(family, case, got, trials, radii, fractions=FRACTIONS, focus=FOCUS, shape="circle", follow=True, centre=None,
          **more):
    """The device's numbers against the reference about the centre the device used, at the focus shift it applied and,
    with follow_centroid, on the moments it wrote: W equal; no ray in a band, so the counts equal; the energy the counts'
    quotient; every radius under its two count conditions.  The figures are printed."""
    ref = ET.reference_of(case, trials, focus, shape, follow, centre=got.record[:, :3] if centre is None else centre,
                          moments=got.moments, focus_shift=got.focus_shift, **more)
    assert np.array_equal(np.nan_to_num(got.record[:, 4:7]).astype(np.int64),
                          np.stack([ref.n_rays, ref.n_missed, ref.n_unfollowed], axis=1)), (family, got.record[:, 4:7])
    radii = np.zeros(0) if radii is None else np.asarray(radii, dtype=np.float64)
    fractions = np.zeros(0) if fractions is None else np.asarray(fractions, dtype=np.float64)
    cells = 0
    for g, grp in enumerate(ref.groups):
        if grp is None or grp.W == 0:
            assert got.total[g] == 0 and not got.count[g].any(), (family, g)
            assert np.all(np.isnan(got.energy[g])) and np.all(np.isnan(got.radius[g])), (family, g)
            continue
        assert int(got.total[g]) == grp.W, (family, g, int(got.total[g]), grp.W)
        if len(radii):
            lower, upper = ET.count_bounds(grp, radii)
            assert np.all(lower <= got.count[g]) and np.all(got.count[g] <= upper), (family, g)
            assert np.array_equal(lower, upper), (family, g, "a ray lies in the band of a radius", ET.undecided(grp, radii))
            assert np.array_equal(got.count[g], lower), (family, g)
            assert_same_bits(got.energy[g], got.count[g].astype(np.float64) / np.float64(grp.W), f"{family}: energy")
            assert np.all(np.diff(got.count[g].astype(np.int64), axis=-1) >= 0)
            cells += lower.size
        if len(fractions):
            below, reached = ET.radius_conditions(grp, fractions, got.radius[g])
            assert np.all(below) and np.all(reached), (family, g, float(np.mean(below)), float(np.mean(reached)))
            cells += below.size
    print(f"[energy tolerance] {family}: {cells} cells exact, undecided share 0")
    return ref


def run_and_check(family, case, trials, n_radii=5, fractions=FRACTIONS, focus=FOCUS, shape="circle", follow=True,
                  compensators=(), centre=None, frame=None, rows=None):
    """``Sensitivity.energy_tolerance`` on (M, K) trials, checked with the nominal trial appended."""
    full = np.vstack([trials, np.zeros((1, trials.shape[1]))])
    radii = radii_for(case, full, n_radii, focus, shape, follow, centre=None if centre is None else np.asarray(centre),
                      compensate=bool(compensators)) if n_radii else None
    run = sensitivity_of(case, frame=frame, rows=rows).energy_tolerance(
        trials, radii, fractions=fractions, shape=shape, focus=focus, compensators=compensators, follow_centroid=follow,
        centre=None if centre is None else centre[0])
    check(family, case, whole(run), full, radii, fractions, focus, shape, follow, centre=centre)
    return run, radii


# ---- the kernels against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ET.SIZES)
def test_ray_tiles_and_slices_alone_and_among_other_rows(n):
    """Rays of a group about the LDS tile (64) and the slice (2048): one slice until 2049 rows give two and 3 * 2048 + 1
    four; without and with the focus compensator; alone in the frame and among 4196 rows of another surface, with the
    same bits."""
    assert T.slices(n, 1, 256) == {2049: 2, 3 * 2048 + 1: 4}.get(n, 1) and T.K.kMtftRays == 64
    case = ET.tolerance_case([n], 3, seed=100 + n)
    trials = ET.random_trials(3, 3)
    frame, rows = among_other_rows(case, ET.FILLER)
    # (one ray lies on its own centroid, its distance nothing but the centroid's rounding: it is measured from a held point)
    follow, centre = (n > 1), (None if n > 1 else np.zeros((1, 3)))
    for compensators in ((), ("focus",)):
        if n == 1 and compensators:
            continue  # (one ray has no spread of slopes to refocus by)
        got, radii = run_and_check(f"{n} rays {compensators}", case, trials, compensators=compensators, follow=follow,
                                   centre=centre)
        other = sensitivity_of(case, frame=frame, rows=rows).energy_tolerance(
            trials, radii, fractions=FRACTIONS, focus=FOCUS, compensators=compensators, follow_centroid=follow,
            centre=None if centre is None else centre[0])
        same_bits(whole(got), whole(other), f"{n} rays among {ET.FILLER} other rows")


@pytest.mark.parametrize("n_trials", ET.TRIAL_COUNTS)
def test_trial_counts_through_the_entry_point(n_trials):
    """M about a thread's trial and the tile of 256: 1, 255 to 257 and 4 * 256 + 1, each handed to the entry point as it
    is, two groups, the focus compensated."""
    case = ET.tolerance_case([90, 40], 5, seed=200 + n_trials)
    t = ET.random_trials(n_trials, 5, seed=n_trials)
    radii = radii_for(case, t, 3, (0.02,), compensate=True)
    trials = np.broadcast_to(t[None], (2,) + t.shape)
    got = entry(sensitivity_of(case), trials, radii, (0.5, 0.9), (0.02,), compensate=True)
    assert got.count.shape == (2, n_trials, 1, 3) and got.radius.shape == (2, n_trials, 1, 2)
    check(f"M = {n_trials}", case, got, t, radii, (0.5, 0.9), (0.02,))


@pytest.mark.parametrize("n_parameters", ET.PARAMETER_COUNTS)
def test_parameter_counts_at_every_instantiation(n_parameters):
    """K = 1, 4 | 5, 8 | 9, 12 | 13, 16: the instantiations of 4, 8, 12 and 16 columns, full and with zero columns."""
    assert T.template_columns(n_parameters) in (4, 8, 12, 16)
    case = ET.tolerance_case([300], n_parameters, seed=40 + n_parameters)
    trials = ET.random_trials(4, n_parameters, 2e-3 / np.sqrt(n_parameters))
    run_and_check(f"K = {n_parameters}", case, trials, focus=(0.0, -0.04), compensators=("focus",), shape="square")


@pytest.mark.parametrize("shape", ET.OUTPUT_COUNTS, ids=lambda s: "x".join(str(v) for v in s))
def test_output_chunks(shape):
    """(planes x radii) about the chunk of 8 plane-major outputs: chunks of one plane, of several, and ones that begin
    inside a plane; radii alone (no fractions)."""
    planes, n_radii = shape
    case = ET.tolerance_case([300], 2, seed=70 + planes * n_radii)
    focus = tuple(np.linspace(-0.04, 0.06, planes)) if planes > 1 else (0.07,)
    got, _ = run_and_check(f"{planes} planes x {n_radii} radii", case, ET.random_trials(3, 2), n_radii, None, focus)
    assert got.radius.shape == (1, 3, planes, 0) and got.energy.shape == (1, 3, planes, n_radii)


@pytest.mark.parametrize("n_fractions", ET.FRACTION_COUNTS)
def test_fraction_tiles(n_fractions):
    """Fractions about the select's tile of 4: 1, 4, 5 and 16, fractions alone (no radii), about the held centre."""
    case = ET.tolerance_case([200, 31], 2, seed=20 + n_fractions)
    fractions = tuple(np.linspace(0.05, 1.0, n_fractions)) if n_fractions > 1 else (0.8,)
    got, _ = run_and_check(f"{n_fractions} fractions", case, ET.random_trials(3, 2), 0, fractions, (0.0, 0.03, -0.02),
                           follow=False)
    assert got.energy.shape == (2, 3, 3, 0) and got.radius.shape == (2, 3, 3, n_fractions)
    assert np.all(np.diff(got.radius, axis=-1) >= 0)


def test_an_empty_group_a_group_without_weight_and_rays_left_out():
    """Three groups: rays (3 left out, 5 not followed), none but 3 that are left out, and rows whose weights are all zero:
    NaN and counts of 0 where there is nothing; the integer weights take B from the selected rows."""
    case = ET.tolerance_case([200, 0, 150], 5, seed=81, left_out=3, unfollowed=5)
    frame = case.frame.copy()
    frame[case.rows[case.group == 2], 1] = 0.0
    case.frame = frame
    trials = ET.random_trials(3, 5)
    for compensators, follow in (((), True), (("focus",), False)):
        got, _ = run_and_check(f"empty groups {compensators}", case, trials, compensators=compensators, follow=follow)
        assert got.n_rays.tolist() == [195, 0, 146] and got.n_missed.tolist() == [3, 3, 2]
        assert got.n_unfollowed.tolist() == [5, 0, 5] and got.total[1:].tolist() == [0, 0] and got.total[0] > 0
        assert np.all(np.isfinite(got.energy[0])) and np.all(np.isnan(got.energy[1:])) and np.all(np.isnan(got.radius[1:]))
        assert np.all(np.isnan(got.yield_(0.5)[1:])) and np.isfinite(got.yield_(0.5)[0])
    run_and_check("empty groups, fixed centre", case, trials, centre=np.zeros((3, 3)), follow=False)


def test_launches_of_trials_outputs_and_items_under_the_slab_cap_leave_no_trace_in_the_bits():
    """4096 groups are 4096 slices at the least: the cap leaves room for one tile of 256 trials, 32 outputs and one
    select item a launch, so 257 trials of 5 planes x 8 radii and 2 fractions run as 2 x (2 + 5 x 21) launches.  Two
    groups hold rays; their outputs are, bit for bit, those of a call with these two groups alone."""
    G_ = 4096
    cap, cell = T.K.kMtftSlabBytes, 224
    assert cap // (G_ * cell) // 256 * 256 == 256 and cap // (G_ * 256 * 8) // 8 * 8 == 32 and cap // (G_ * 256 * cell) == 1
    assert cap // (2 * cell) // 256 * 256 >= 512
    case = ET.tolerance_case([50] + [0] * (G_ - 2) + [30], 2, seed=7)
    t = ET.random_trials(257, 2, seed=8)
    focus, fractions = (0.0, 0.01, 0.02, -0.01, -0.02), (0.5, 0.9)
    pair = SimpleNamespace(frame=case.frame, rows=case.rows, group=(case.group > 0).astype(np.int64), n_groups=2,
                           jacobian=case.jacobian, slopes=case.slopes, n_parameters=2, rays_per_source=case.rays_per_source)
    radii = radii_for(pair, t, 8, focus, compensate=True)
    many = entry(sensitivity_of(case), np.broadcast_to(t[None], (G_, 257, 2)), radii, fractions, focus, compensate=True)
    alone = entry(sensitivity_of(pair), np.broadcast_to(t[None], (2, 257, 2)), radii, fractions, focus, compensate=True)
    check("two groups of 4096", pair, alone, t, radii, fractions, focus)
    lit = np.array([0, G_ - 1])
    for key in KEYS:
        assert_same_bits(getattr(many, key)[lit], getattr(alone, key), f"among 4096 groups: {key}")
    dark = np.setdiff1d(np.arange(G_), lit)
    assert np.all(np.isnan(many.energy[dark])) and np.all(np.isnan(many.radius[dark])) and not many.count[dark].any()
    assert not many.total[dark].any()


# ---- exact arithmetic with ties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ET.SHAPES)
def test_a_dyadic_lattice_is_counted_exactly_with_rays_on_the_radii(shape):
    """Lattice inputs about the held centre (0, 0, 0): every fma is exact and plain float64 numpy is the truth.  Many rays
    lie exactly on a radius (d <= R inclusive) and share distances, the weights are unequal: counts and radii bit for
    bit, for 2049 rays (two slices)."""
    case, trials, focus = ET.lattice_case(2049)
    radii = np.array([0.0, 0.5, 1.0, 1.25, 2.0, 2.5, 3.0, 5.0, 8.0])
    fractions = (0.1, 0.5, 0.8, 0.9, 1.0)
    run = sensitivity_of(case).energy_tolerance(trials, radii, fractions=fractions, shape=shape, focus=focus,
                                                follow_centroid=False, centre=(0.0, 0.0, 0.0))
    got = whole(run)
    full = np.vstack([trials, np.zeros((1, 3))])
    ref = ET.reference_of(case, full, focus, shape, False, centre=np.zeros((1, 3)))
    import energy_reference as E

    grp = ref.groups[0]
    P, S = grp.P.astype(np.float64), grp.S.astype(np.float64)
    assert np.all(P.astype(LD) == grp.P) and np.all(S.astype(LD) == grp.S), "the lattice is not exact in float64"
    # (plain float64 numpy on the moved points: exact up to the circle's root, which is correctly rounded on both sides)
    d = np.array([[E.distances(P[m].T, S[m].T, delta, np.zeros(2), shape) for delta in focus] for m in range(len(P))])
    grp = SimpleNamespace(d=d.astype(LD), q=grp.q, W=grp.W)
    on_a_radius = np.isin(d, radii).sum()
    assert on_a_radius > 200 and len(np.unique(d)) < d.size // 4, (on_a_radius, len(np.unique(d)), d.size)
    assert int(got.total[0]) == grp.W and len(set(grp.q.tolist())) == 4
    assert np.array_equal(got.count[0], ET.counts_in_float64(grp, radii))
    assert_same_bits(got.energy[0], got.count[0].astype(np.float64) / np.float64(grp.W), "lattice energy")
    assert_same_bits(got.radius[0], ET.radius_in_float64(grp, fractions), "lattice radius")


# ---- the bit contracts --------------------------------------------------------------------------------------------------------
def test_two_runs_a_trial_alone_among_1025_at_another_index_and_a_zero_column_give_the_same_bits():
    case = ET.tolerance_case([700, 90], 4, seed=61)
    focus = (0.0, 0.03, -0.02)
    sens = sensitivity_of(case)
    t = ET.random_trials(1025, 4, seed=62)
    many = np.broadcast_to(t[None], (2,) + t.shape)
    radii = radii_for(case, t[:16], 6, focus, compensate=True)  # (clear of the first trials; only bits are compared)
    among = entry(sens, many, radii, FRACTIONS, focus, compensate=True)
    again = entry(sens, many, radii, FRACTIONS, focus, compensate=True)
    same_bits(among, again, "run to run")
    alone = entry(sens, many[:, 7:8], radii, FRACTIONS, focus, compensate=True)
    for key in KEYS[:5]:
        assert_same_bits(getattr(alone, key)[:, 0], getattr(among, key)[:, 7], f"trial 7 alone: {key}")
    same_bits(alone, among, "trial 7 alone", ("record", "total"))
    order = np.random.default_rng(63).permutation(1025)
    order[np.flatnonzero(order == 7)[0]], order[300] = order[300], 7
    permuted = entry(sens, many[:, order], radii, FRACTIONS, focus, compensate=True)
    for key in KEYS[:5]:
        assert_same_bits(getattr(permuted, key), getattr(among, key)[:, order], f"permuted trials: {key}")
    wide_j = np.concatenate([case.jacobian, np.ones_like(case.jacobian[:1])])
    wide_s = np.concatenate([case.slopes, np.zeros_like(case.slopes[:1])])
    wide = entry(sensitivity_of(case, jacobian=wide_j, slopes=wide_s),
                 np.concatenate([many[:, :5], np.zeros((2, 5, 1))], axis=2), radii, FRACTIONS, focus, compensate=True)
    for key in KEYS[:5]:
        assert_same_bits(getattr(wide, key), getattr(among, key)[:, :5], f"a zero column appended: {key}")
    check("the first 16 of 1025", case, SimpleNamespace(**{k: (getattr(among, k)[:, :16] if k in KEYS[:5] else
                                                              getattr(among, k)) for k in KEYS}), t[:16], radii,
          FRACTIONS, focus)


def test_moments_focus_shift_and_record_have_mtf_tolerances_bits():
    case = ET.tolerance_case([2500, 300], 9, seed=97, left_out=2)
    trials = ET.random_trials(5, 9, 7e-4)
    sens = sensitivity_of(case)
    for compensators in ((), ("focus",)):
        mine = sens.energy_tolerance(trials, fractions=(0.8,), focus=(-0.03, 0.0), compensators=compensators)
        mtf = sens.mtf_tolerance(trials, (10.0,), azimuths=(0.0,), focus=(-0.03, 0.0), compensators=compensators)
        for key in ("moments", "record", "focus_shift", "best_focus", "rms_radius", "centroid", "centre", "sum_weights"):
            assert_same_bits(getattr(mine, key), getattr(mtf, key), f"{compensators}: {key}")
        assert_same_bits(mine.nominal.focus_shift, mtf.nominal.focus_shift, "nominal focus shift")


# ---- the nominal trial against enclosed_energy(), monotonicity ----------------------------------------------------------------
@pytest.mark.parametrize("follow", (True, False), ids=("centroid", "held"))
def test_the_zero_trial_is_enclosed_energy_of_the_same_rows(follow):
    """The zero trial without a compensator against frame.enclosed_energy() of the same selection (no row left out, so the
    integer weights are the same): counts equal at clear radii; each of its radii under the two count conditions, the
    bands widened by the distance between the two passes' centres (their sums have different trees)."""
    case = ET.tolerance_case([700, 300], 2, seed=99)
    zero = np.zeros((1, 2))
    focus = (0.0, 0.04)
    radii = radii_for(case, zero, 6, focus, follow=follow)
    run = sensitivity_of(case).energy_tolerance(zero, radii, fractions=FRACTIONS, focus=focus, follow_centroid=follow)
    plain = device_frame(case.frame).enclosed_energy(R.SURFACE, radii, fractions=FRACTIONS, focus=focus, reference=run.centre,
                                                     follow_centroid=follow, rays_per_source=case.rays_per_source,
                                                     n_groups=case.n_groups)
    ref = check("zero trial", case, whole(run), np.zeros((2, 2)), radii, FRACTIONS, focus, follow=follow)
    assert_same_bits(run.nominal.energy, plain.energy, "nominal energy against enclosed_energy()")
    assert_same_bits(run.energy[:, 0], plain.energy, "the zero trial's energy against enclosed_energy()")
    for g, grp in enumerate(ref.groups):
        theirs = plain.centroid_shift[g, 0][None, :] + np.asarray(focus)[:, None] * plain.centroid_shift[g, 1][None, :]
        apart = np.abs(theirs - grp.centres[0]).sum(axis=1) if follow else np.zeros(2)  # (F)
        wide = SimpleNamespace(d=grp.d[:1], eps=grp.eps[:1] + apart[None, :, None], q=grp.q, W=grp.W)
        below, reached = ET.radius_conditions(wide, FRACTIONS, plain.radius[g][None])
        assert np.all(below) and np.all(reached), (g, apart)


def test_energy_is_monotone_in_the_radius_and_reaches_the_fraction_at_the_returned_radius():
    case = ET.tolerance_case([500], 3, seed=33)
    trials = ET.random_trials(6, 3)
    sens = sensitivity_of(case)
    first = sens.energy_tolerance(trials, fractions=FRACTIONS, focus=FOCUS, compensators=("focus",))
    assert np.all(np.diff(first.radius, axis=-1) >= 0)
    for m in range(6):  # (the radii a trial returned, handed back as radii: its energy there is at least the fraction)
        for f in range(2):
            edges = np.unique(first.radius[0, m, f])
            again = sens.energy_tolerance(trials, edges, fractions=None, focus=FOCUS, compensators=("focus",))
            assert np.all(np.diff(again.energy, axis=-1) >= 0)
            at = np.searchsorted(edges, first.radius[0, m, f])
            assert np.all(again.energy[0, m, f, at] >= np.asarray(FRACTIONS)), (m, f)


# ---- the tracer ---------------------------------------------------------------------------------------------------------------
def test_trace_energy_tolerance_is_trace_sensitivity_then_energy_tolerance():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=257)
    parameters = [prt.Motion(lens, translate=(0, 1, 0)), prt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)),
                  prt.IndexChange(lens)]
    tolerances = prt.Tolerances([0.01, 0.02, 0.05])
    tracer.trace()
    before = tracer.get_results().copy()
    options = dict(fractions=(0.5, 0.8), focus=(0.0, 0.01), compensators=("focus",), shape="square")
    got = tracer.trace_energy_tolerance(det, parameters, tolerances, [0.01, 0.02, 0.05], trials=40, **options)
    assert tracer.get_results().equals(before)  # (the tracer's last result is left as it was)
    sens = tracer.trace_sensitivity(det, parameters, slopes=True)
    want = sens.energy_tolerance((tolerances, 40), [0.01, 0.02, 0.05], **options)
    assert isinstance(got, prt.EnergyToleranceRun) and got.energy.shape == (1, 40, 2, 3) and got.radius.shape == (1, 40, 2, 2)
    same_bits(whole(got), whole(want), "trace_energy_tolerance")
    assert got.n_rays[0] == 257 and np.all(np.isfinite(got.energy)) and got.parameters == tuple(parameters)
    assert got.count.dtype == np.uint64 and np.array_equal(got.trials, tolerances.sample(40))
    assert np.array_equal(got.yield_(0.5, radius=1), want.yield_(0.5, radius=1)) and 0.0 <= got.yield_(0.5)[0] <= 1.0
    assert 0.0 <= got.yield_radius(0.02, fraction=0)[0] <= 1.0
    assert got.percentiles((10, 90), fraction=1).shape == (1, 2) and len(got.to_pandas()) == 40
    table = tracer.trace_energy_tolerance(det, parameters, None, trials=tolerances.sensitivity_table()).table()
    assert sorted(table["parameter"].tolist()) == [0, 1, 2] and np.all(np.diff(table["worst"]) <= 0)
    with pytest.raises(ValueError, match="sensitivity_table"):
        got.table()
    with pytest.raises(ValueError, match="slopes=True"):
        tracer.trace_sensitivity(det, parameters).energy_tolerance(np.zeros((1, 3)), [0.1])
    with pytest.raises(ValueError, match="compensators"):
        sens.energy_tolerance(np.zeros((1, 3)), [0.1], compensators=("tilt",))
    with pytest.raises(ValueError, match="radii"):
        sens.energy_tolerance(np.zeros((1, 3)), None, fractions=None)
    with pytest.raises(ValueError, match="shape"):
        sens.energy_tolerance(np.zeros((1, 3)), [0.1], shape="hexagon")
    with pytest.raises(ValueError, match="needs tolerances"):
        tracer.trace_energy_tolerance(det, parameters, None, [1.0], trials=10)


# ---- end to end: the device against the enclosed energy of the oracle's re-traces ---------------------------------------------
@pytest.mark.parametrize("name", ("singlet", "two_fields"))
def test_end_to_end_the_error_of_the_linear_ray_model_is_of_second_order(name):
    """The device's run of 4 trials with every applicable parameter moved at once (no compensator, planes 0 and 0.5,
    about the held nominal centroid) against ``traced_frame(tolerance_scenes.build(name, 257, trial)).enclosed_energy``
    of the re-trace about the same point.  With eps(h) = max_r |d_lin,r - d_retraced,r| over the rays an order statistic
    moves by no more than its largest element: |radius_lin - radius_retraced| <= eps(h) and EE_retraced(R - eps) <=
    EE_lin(R) <= EE_retraced(R + eps), each widened by the band; and eps(h / 2) <= eps(h) / 3.  The scenes, planes and the
    rule for h are tests/test_host_energy_tolerance.py's, which holds the reference alone to the same on the CPU."""
    import energy_reference as E
    import opd_scenes
    import tolerance_scenes
    from test_host_energy_tolerance import E2E_FRACTIONS, E2E_PLANES, E2E_TOP, e2e_radii
    from test_host_mtf_tolerance import e2e_trials

    case = opd_scenes.build(name, 257)
    per = getattr(case, "rays_per_source", None)
    n_groups = 2 if per else 1
    kw = dict(rays_per_source=per, n_groups=n_groups) if per else {}
    sens = traced_frame(case).sensitivity(case.surface, list(case.parameters), case.parts, slopes=True, **kw)
    assert not (sens.n_unknown or sens.n_invalid or sens.n_unfit)
    rows = sens.rows().cpu().numpy()
    group = np.floor(case.frame[rows, 4] / per).astype(int) if per else np.zeros(len(rows), int)
    f = case.frame
    jacobian, slopes = sens.jacobian.cpu().numpy(), sens.slopes.cpu().numpy()
    rays, rec = T.staged(f[rows, 9:12], f[rows, 12:15], f[rows, 1], group, n_groups, jacobian, slopes)
    dp = np.concatenate([ray.dp.astype(float) for ray in rays], axis=2)
    n_par, live = len(case.parameters), tolerance_scenes.applicable(case.parameters)
    direction, h = e2e_trials(dp, group, n_groups, live, n_par, E2E_TOP)
    centre = rec.centre.astype(np.float64)
    radii = e2e_radii(rays)

    def error(scale):
        trials = direction * (h * scale)
        got = sens.energy_tolerance(trials, radii, fractions=E2E_FRACTIONS, focus=E2E_PLANES, follow_centroid=False,
                                    centre=centre)
        ref = ET.energy_tolerance_reference(f[rows, 9:12], f[rows, 12:15], f[rows, 1], group, n_groups, jacobian, slopes,
                                            trials, E2E_PLANES, "circle", False, centre=centre)
        worst = 0.0
        for m in range(4):
            moved = tolerance_scenes.build(name, 257, trials[m])
            assert moved.counts == case.counts and np.array_equal(moved.frame[:, 4], case.frame[:, 4]), "rays lost or gained"
            assert np.array_equal(moved.frame[rows, 1], f[rows, 1])
            staged = E.stage(moved.frame[rows], None, rays_per_source=per, n_groups=n_groups, reference=centre)
            eps = np.zeros(n_groups)
            for g, (p, s, _, _, used, _) in enumerate(staged):
                assert used == rec.n_rays[g]
                for k, delta in enumerate(E2E_PLANES):
                    d = E.distances(p, s, delta, np.zeros(2), "circle")
                    # (1e-12: the roundings of the two stagings and distances, far below a band of 1e-5)
                    eps[g] = max(eps[g], float(np.abs(ref.groups[g].d[m, k].astype(np.float64) - d).max()
                                               + ref.groups[g].eps[m, k].max()) + 1e-12)
            worst = max(worst, eps.max())
            frame = traced_frame(moved)
            common = dict(focus=E2E_PLANES, reference=centre, follow_centroid=False, **kw)
            want = frame.enclosed_energy(moved.surface, fractions=E2E_FRACTIONS, **common)
            assert np.all(np.abs(got.radius[:, m] - want.radius) <= eps[:, None, None]), (name, m)
            for g in range(n_groups):
                inside = radii - eps[g] >= 0  # (a radius below eps: nothing lies within R - eps < 0, the bound is 0)
                if inside.any():
                    inner = frame.enclosed_energy(moved.surface, (radii - eps[g])[inside], fractions=None, **common)
                    assert np.all(inner.energy[g] <= got.energy[g, m][:, inside]), (name, m)
                outer = frame.enclosed_energy(moved.surface, radii + eps[g], fractions=None, **common)
                assert np.all(got.energy[g, m] <= outer.energy[g]), (name, m)
        return worst

    e1, e2 = error(1.0), error(0.5)
    print(f"[energy tolerance] {name} on the device: h {h:.4f}, eps(h) {e1:.3e}, eps(h/2) {e2:.3e} (ratio {e2 / e1:.3f})")
    assert e2 <= e1 / 3, (name, e1, e2)
