"""MTF sensitivities on the device (Sensitivity.mtf_gradient, the entry point prt_frame_mtf_gradient, the kernels of
prt_mtf_gradient.hpp) against the longdouble reference of tests/mtf_gradient_reference.py, every output and parameter held
to the error budget derived there: at the edges of the LDS tile, the ray slices, the output tiles and the parameter
chunks; the bit contracts; ``sensitivity(slopes=True)``; and, end to end on frames the C oracle traced, against central
differences of the longdouble OTF of the oracle's own re-traces.  Each test prints its largest deviation / bound ratio."""
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import helpers
import mtf_gradient_reference as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
SMALL = dict(frequencies=(0.0, 40.0, 150.0, 300.0), azimuths=(0.0, 90.0), focus=(0.0, 0.05))


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def sensitivity_of(case, frame=None, rows=None, jacobian=None, slopes=None):
    """A Sensitivity that holds the case's synthetic jacobian and slopes for its selected rows: what mtf_gradient reads."""
    from pyrayt_amd.frame import Sensitivity

    jacobian = case.jacobian if jacobian is None else jacobian
    slopes = case.slopes if slopes is None else slopes
    n_par, G = len(jacobian), case.n_groups
    device = device_frame(case.frame if frame is None else frame)
    first = np.searchsorted(case.group, np.arange(G + 1)).astype(np.int64)
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    return Sensitivity(on(jacobian), on(case.rows if rows is None else rows),
                       np.zeros((G, 6 + 4 * n_par + n_par * (n_par + 1) // 2)), np.zeros((G, 3)), True, (0, 0, 0, 0),
                       [f"p{k}" for k in range(n_par)],
                       launch=dict(slopes=on(slopes), rows=device._contiguous_rows(), weights="intensity", group_first=first))


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
    assert np.array_equal(np.isnan(got), nan), (family, what, "NaN pattern")
    if nan.all():
        return 0.0
    deviation = M.deviation(got, re, im)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | ((deviation == 0) & (bound == 0)), 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[mtf gradient] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, {got.size} values)")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


def check(family, case, got, options, centre=None, jacobian=None, slopes=None):
    """The device's MTFGradient against the reference with the centre the device used."""
    ref = M.reference_of(case, centre=got.centre if centre is None else centre, jacobian=jacobian, slopes=slopes, **options)
    n_par = ref.n_parameters
    assert np.array_equal(got.n_rays, ref.n_rays) and np.array_equal(got.n_missed, ref.n_missed)
    assert np.array_equal(got.n_unfollowed, ref.n_unfollowed)
    with np.errstate(invalid="ignore"):
        usable = (ref.n_rays > 0) & (ref.sum_weights.astype(float) > 0)
    if centre is None:  # (the device's own centroid, apart from the sums)
        assert np.all(np.abs(got.centre[usable].astype(LD) - ref.centroid[usable]) <= ref.centre_bound[usable])
    else:
        assert np.array_equal(got.centre, np.broadcast_to(np.asarray(centre, dtype=float), got.centre.shape))
    hold(family, "otf", got.otf, ref.re, ref.im, ref.otf_bound)
    hold(family, "dotf", got.dotf, ref.dre[:, :n_par], ref.dim[:, :n_par], ref.dbound[:, :n_par])
    hold(family, "dotf_dfocus", got.dotf_dfocus, ref.dre[:, n_par], ref.dim[:, n_par], ref.dbound[:, n_par])
    hold(family, "centroid_gradient", got.centroid_gradient, ref.dcentroid, np.zeros_like(ref.dcentroid), ref.dcentroid_bound)
    with np.errstate(invalid="ignore"):
        assert np.all(got.sum_weights[~usable] == 0)
        assert np.all(np.abs(got.sum_weights[usable] - ref.sum_weights[usable].astype(float))
                      <= 64 * R.U64 * ref.sum_weights[usable].astype(float))
    return ref


def outputs(got):
    return dict(otf=got.otf, dotf=got.dotf, dotf_dfocus=got.dotf_dfocus, record=got.record)


def assert_same_bits(got, want, what):
    """helpers.assert_same_bits on real arrays; a complex array as its (re, im) pairs of float64."""
    parts = lambda x: np.ascontiguousarray(x).view(np.float64) if np.iscomplexobj(x) else x  # noqa: E731
    helpers.assert_same_bits(parts(got), parts(want), what)


def same_bits(a, b, what):
    for key, value in outputs(a).items():
        assert_same_bits(value, outputs(b)[key], f"{what}: {key}")


# ---- the kernel against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
def test_ray_tiles_and_slices_alone_and_among_other_rows(n):
    """Rays of a group about the LDS tile (kMtfgTile = 128) and the slice (kMtfgMinSlice = 2048): one slice until
    3 * 2048 + 1 rows give four; alone in the frame and among 4196 rows of another surface, which change nothing -- the
    partition follows the selected rows alone -- so the two runs give the same bits."""
    assert (M.K.kMtfgTile, M.K.kMtfgMinSlice) == (128, 2048)
    assert M.slices(n, 1, 16) == {1: 1, 2049: 2, 3 * 2048 + 1: 4}.get(n, 1)
    case = M.gradient_case([n], 3, seed=100 + n)
    got = sensitivity_of(case).mtf_gradient(**SMALL)
    check(f"{n} rays", case, got, SMALL)
    frame, rows = among_other_rows(case, M.FILLER)
    other = sensitivity_of(case, frame=frame, rows=rows).mtf_gradient(**SMALL)
    same_bits(got, other, f"{n} rays among {M.FILLER} other rows")


@pytest.mark.parametrize("n_parameters", M.PARAMETER_COUNTS)
def test_parameter_chunks(n_parameters):
    """K = 1, 7, 8, 9 and 16 about the chunk of kMtfgParams = 8 accumulator sets: one launch of the instantiation of 1, of
    8 with an empty column, of 8 whole, 8 and then 1, and two chunks of 8 in one launch."""
    assert M.K.kMtfgParams == 8
    case = M.gradient_case([300], n_parameters, seed=40 + n_parameters)
    options = dict(frequencies=(0.0, 25.0, 180.0), azimuths=(0.0, 90.0), focus=(0.0, -0.04))
    got = sensitivity_of(case).mtf_gradient(**options)
    assert got.dotf.shape == (1, n_parameters, 2, 2, 3)
    check(f"K = {n_parameters}", case, got, options)


def test_a_parameter_alone_has_the_bits_it_has_among_sixteen():
    """Every ray is followed, so the kept set is the same: parameter k alone (the instantiation of 1) against parameter k
    among sixteen (two chunks of 8), and the OTF and the focus derivative of both calls."""
    case = M.gradient_case([300], 16, seed=56)
    among = sensitivity_of(case).mtf_gradient(**SMALL)
    for k in range(16):
        alone = sensitivity_of(case, jacobian=case.jacobian[k:k + 1], slopes=case.slopes[k:k + 1]).mtf_gradient(**SMALL)
        assert_same_bits(alone.dotf[:, 0], among.dotf[:, k], f"parameter {k} alone: dotf")
        assert_same_bits(alone.centroid_gradient[:, 0], among.centroid_gradient[:, k], f"parameter {k} alone: dC")
        assert_same_bits(alone.otf, among.otf, f"parameter {k} alone: otf")
        assert_same_bits(alone.dotf_dfocus, among.dotf_dfocus, f"parameter {k} alone: dotf_dfocus")


@pytest.mark.parametrize("shape", M.OUTPUT_COUNTS, ids=lambda s: "x".join(str(v) for v in s))
def test_output_tiles(shape):
    """planes x azimuths x frequencies on both sides of the output tile of each lane count: 127, 128 | 129 (lanes 4 | 2),
    256 | 257 (lanes 2 | 1), 512 | 513 (one tile | two)."""
    planes, azimuths, frequencies = shape
    n_out = planes * azimuths * frequencies
    assert -(-n_out // M.tile(n_out)) == (2 if n_out == 513 else 1)
    options = dict(focus=np.linspace(-0.04, 0.06, planes) if planes > 1 else (0.07,),  # (a lone plane with delta != 0)
                   azimuths=tuple(np.linspace(0.0, 170.0, azimuths)), frequencies=np.linspace(0.0, 400.0, frequencies))
    case = M.gradient_case([300], 2, seed=70 + n_out)
    got = sensitivity_of(case).mtf_gradient(**options)
    check(f"{n_out} outputs", case, got, options)


def test_an_empty_group_and_a_group_without_weight_are_nan_with_their_counts():
    """Three groups: rays, none at all, and 150 rays whose weights are all zero (sum w = 0): NaN, the counts right."""
    case = M.gradient_case([200, 0, 150], 2, seed=81, left_out=0)
    frame = case.frame.copy()
    frame[case.rows[case.group == 2], 1] = 0.0
    case.frame = frame
    got = sensitivity_of(case).mtf_gradient(**SMALL)
    check("empty groups", case, got, SMALL)
    fixed = sensitivity_of(case).mtf_gradient(centre=(0.0, 0.0, 0.0), **SMALL)
    check("empty groups, fixed centre", case, fixed, SMALL, centre=np.zeros((3, 3)))
    for made in (got, fixed):
        assert made.n_rays.tolist() == [200, 0, 150] and not made.n_missed.any() and not made.n_unfollowed.any()
        assert np.all(np.isnan(made.otf[1:])) and np.all(np.isnan(made.dotf[1:])) and np.all(np.isnan(made.dotf_dfocus[1:]))
        assert np.all(np.isnan(made.centroid_gradient[1:])) and np.all(made.sum_weights[1:] == 0)
        assert np.all(np.isnan(made.dmtf[1:])) and np.all(np.isfinite(made.dotf[0]))
    assert np.all(np.isnan(got.centre[1:])) and np.all(fixed.centre == 0)


def test_phases_of_thousands_of_cycles():
    """About a centre five units away, at up to 1000 cycles per unit: phases of 5000 cycles, reduced in fp64."""
    options = dict(frequencies=(0.0, 333.0, 1000.0), azimuths=R.FAR_AZIMUTHS, focus=(0.0, 0.05))
    case = M.gradient_case([400], 3, seed=90)
    got = sensitivity_of(case).mtf_gradient(centre=R.FAR_REFERENCE, **options)
    check("far centre", case, got, options, centre=np.array([R.FAR_REFERENCE]))
    p = case.frame[case.rows, 9:12] - np.asarray(R.FAR_REFERENCE)
    assert np.abs(1000.0 * p[:, 1:]).max() > 3000.0  # (cycles, at the highest frequency)


def test_rays_left_out_and_rays_not_followed():
    """Per group 3 rays the MTF leaves out (n_missed) and 5 with a NaN in one parameter's Jacobian (n_unfollowed): out for
    every parameter, and the others as the reference has them without those rays."""
    case = M.gradient_case([300, 170], 5, seed=95, left_out=3, unfollowed=5)
    got = sensitivity_of(case).mtf_gradient(**SMALL)
    ref = check("rays left out", case, got, SMALL)
    assert got.n_missed.tolist() == [3, 3] and got.n_unfollowed.tolist() == [5, 5] and got.n_rays.tolist() == [300 - 5, 170 - 5]
    assert np.all(np.isfinite(got.dotf)) and ref.n_unfollowed.tolist() == [5, 5]
    # the same rays taken out of the selection altogether: the sums see the same terms, zeros apart
    keep = ~case.spoiled & R.mtf_kept(case.frame[case.rows, 9:12], case.frame[case.rows, 12:15], case.frame[case.rows, 1],
                                      R.default_axes())
    fewer = SimpleNamespace(frame=case.frame, rows=case.rows[keep], group=case.group[keep], n_groups=2,
                            jacobian=case.jacobian[:, :, keep], slopes=case.slopes[:, :, keep])
    without = sensitivity_of(fewer).mtf_gradient(centre=got.centre, **SMALL)
    check("rays left out, taken out", fewer, without, SMALL, centre=got.centre)
    again = sensitivity_of(case).mtf_gradient(centre=got.centre, **SMALL)
    # (other tiles and slices, so other roundings of the same sums: n u of them, far under 1e-9)
    assert np.abs(without.dotf - again.dotf).max() <= 1e-9 * np.abs(got.dotf).max()


def test_two_runs_give_the_same_bits():
    case = M.gradient_case([2500, 300], 9, seed=97, left_out=2)
    options = dict(frequencies=np.linspace(0.0, 300.0, 11), azimuths=(0.0, 45.0, 90.0), focus=(-0.03, 0.0, 0.03, 0.06))
    first = sensitivity_of(case).mtf_gradient(**options)
    second = sensitivity_of(case).mtf_gradient(**options)
    same_bits(first, second, "run to run")
    centred = sensitivity_of(case).mtf_gradient(reference="centroid", **options)
    assert_same_bits(centred.otf, first.otf, "reference='centroid' is composed on the host: otf")
    ref = M.reference_of(case, centre=first.centre, **options)
    dre, dim = M.follow_centroid(ref, options["frequencies"], options["azimuths"])
    kc, ks = (np.abs(x) for x in R.frequency_table(options["frequencies"], options["azimuths"]))
    # the composition's own budget: the three terms' bounds, the centroid's gradient held to its own
    shift = ref.dcentroid_bound[..., 1, None, None] * kc + ref.dcentroid_bound[..., 2, None, None] * ks
    bound = (ref.dbound[:, :9] + 2 * np.pi * shift[:, :, None] * np.abs(ref.otf)[:, None]
             + 2 * np.pi * (np.abs(ref.dcentroid[..., 1, None, None].astype(float)) * kc
                            + np.abs(ref.dcentroid[..., 2, None, None].astype(float)) * ks)[:, :, None] * ref.otf_bound[:, None]
             + ref.dcentroid_bound[..., 0, None, None, None] * np.abs(ref.dotf[:, 9])[:, None]
             + np.abs(ref.dcentroid[..., 0, None, None, None].astype(float)) * ref.dbound[:, 9][:, None])
    hold("follows the centroid", "dotf", centred.dotf, dre, dim, bound)


def test_otf_is_the_mtf_passes_within_the_budget():
    """otf of mtf_gradient against the reference and against frame.mtf(reference=centre) of the same rows: within
    otf_bound; the bits are not promised (mtf() sorts the rows by group in row order, this pass takes the selection's)."""
    case = M.gradient_case([700, 300], 2, seed=99, left_out=2)
    options = dict(frequencies=np.linspace(0.0, 300.0, 9), azimuths=(0.0, 60.0), focus=(0.0, 0.04))
    got = sensitivity_of(case).mtf_gradient(**options)
    ref = check("otf", case, got, options)
    plain = device_frame(case.frame).mtf(R.SURFACE, reference=got.centre, rays_per_source=case.rays_per_source,
                                         n_groups=case.n_groups, **options)
    apart = np.abs(plain.otf - got.otf)
    print(f"[mtf gradient] otf against mtf(): largest difference {apart.max():.3e}, difference / bound "
          f"{(apart / ref.otf_bound).max():.3f}")
    assert np.all(apart <= ref.otf_bound)
    assert np.array_equal(plain.n_rays, got.n_rays) and np.array_equal(plain.n_missed, got.n_missed)


# ---- sensitivity(slopes=True) -----------------------------------------------------------------------------------------------
def traced_frame(case):
    from test_gpu_design_sensitivity import device_frame as traced

    return traced(case.frame, case.counts)


def scene(kind):
    """One scene of each family at n = 257, frames from the C oracle: (case, parameters, keywords of sensitivity())."""
    import design_scenes
    import launch_scenes
    import opd_scenes
    import sensitivity_scenes

    if kind == "motions":
        case = sensitivity_scenes.build("config2", 257)
        return case, list(case.motions), {}
    if kind == "design":
        case = design_scenes.build("lens", 257)
        return case, list(case.parameters), {}
    if kind == "wavefront":
        case = opd_scenes.build("singlet", 257)
        return case, list(case.parameters), dict(wavefront=True)
    case = launch_scenes.build("fields", 257)
    return case, list(case.parameters), dict(rays_per_source=257, n_groups=3)


@pytest.mark.parametrize("kind", ("motions", "design", "wavefront"))
def test_slopes_true_leaves_every_other_output_its_bits(kind):
    """slopes=True sends a call without launch parameters through prt_frame_launch_sensitivity with all flags 0: jacobian,
    sums and the wavefront outputs are bit for bit what the call's own entry point gives; slopes come with them."""
    case, parameters, kw = scene(kind)
    dev = traced_frame(case)
    plain = dev.sensitivity(case.surface, parameters, case.parts, **kw)
    got = dev.sensitivity(case.surface, parameters, case.parts, slopes=True, **kw)
    assert plain.slopes is None and got.slopes is not None and got.slopes.shape == got.jacobian.shape
    assert torch.equal(plain.rows(), got.rows())
    assert_same_bits(got.jacobian.cpu().numpy(), plain.jacobian.cpu().numpy(), f"{kind}: jacobian")
    assert_same_bits(np.asarray(got.sums), np.asarray(plain.sums), f"{kind}: sums")
    assert (got.n_unknown, got.n_invalid, got.n_unfit, got.n_reflections) == (
        plain.n_unknown, plain.n_invalid, plain.n_unfit, plain.n_reflections)
    if kind == "wavefront":
        for name in ("dfield", "dopd", "dpupil", "opd", "pupil"):
            assert_same_bits(getattr(got, name).cpu().numpy(), getattr(plain, name).cpu().numpy(), f"{kind}: {name}")
        assert_same_bits(np.asarray(got.opd_sums), np.asarray(plain.opd_sums), f"{kind}: opd_sums")
    slopes, jacobian = got.slopes.cpu().numpy(), got.jacobian.cpu().numpy()
    assert np.array_equal(np.isnan(slopes), np.isnan(jacobian))
    with pytest.raises(ValueError, match="slopes=True"):
        plain.mtf_gradient([10.0])


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_slopes_of_a_motion_against_the_retraced_directions():
    """slopes of the lens's tilt (a Motion) on the config-2 lens against central differences of the unit directions of the
    oracle's re-traces, held as tests/test_host_launch_sensitivity.py holds the reference's: h the first power of four at
    which the oracle's own Richardson estimate (4/3 |D(h) - D(h/2)|) is truncation and not rounding (its median at least
    ten times the floor 4 eps / h), the bound that estimate plus the floor."""
    from test_host_sensitivity import moved_trace

    case, parameters, _ = scene("motions")
    got = traced_frame(case).sensitivity(case.surface, parameters, case.parts, slopes=True)
    rows = got.rows().cpu().numpy()
    slopes = got.slopes.cpu().numpy()
    eps = 2.0 ** -52
    for k in (0, 1):
        for exponent in range(-12, -1):
            h = 4.0 ** exponent
            values = []
            for step in (h, h / 2):
                (plus, counts_p, _), (minus, counts_m, _) = moved_trace(case, k, step), moved_trace(case, k, -step)
                assert counts_p == case.counts and counts_m == case.counts, f"h = 4^{exponent}: rays changed their path"
                values.append((unit(plus[rows, 12:15]) - unit(minus[rows, 12:15])) / (2 * step))
            coarse, fine = values
            floor = 4 * eps / h
            estimate = (4.0 / 3.0) * np.abs(coarse - fine)
            if np.any(estimate > 0) and np.median(estimate[estimate > 0]) >= 10 * floor:
                break
        else:
            raise AssertionError("the oracle's differences never rose above their rounding floor")
        error, bound = np.abs(slopes[k].T - fine), estimate + floor
        print(f"[mtf gradient] slopes of motion {k}: h = 2^{int(np.log2(h))}, max |D| {np.abs(fine).max():.3e}, error "
              f"{error.max():.3e}, worst error / bound {np.max(error / bound):.3f}")
        assert np.abs(fine).max() > 1e-3 and np.all(error <= bound)


# ---- end to end: the device against central differences of the OTF of the oracle's re-traces -------------------------------
# Steps chosen on the CPU from the oracle and the longdouble reference alone (never from the device's output): for each
# parameter the power of two at which |D(h) - D(h/2)| is under 1 % of the largest |dOTF| and, at every output, at least
# 2.2 times |reference - D(h/2)| plus the budget of the device's own rounding; at none of them does a ray change its
# surfaces.  parameter: (h with the centre fixed, h with the centre following the centroid) -- a parameter that moves the
# image as a whole has a small derivative about the centroid, the remainder of two large terms, so the device's budget
# stays what it is while the differences' own error shrinks, and the step there is larger.  A parameter that is not listed
# is one whose re-trace the scene's builder does not offer.
E2E_OPTIONS = dict(frequencies=(0.0, 20.0, 50.0), azimuths=(20.0, 110.0), focus=(0.0, 0.02))
E2E_STEPS = {"motions": {0: (2.0 ** -9, 2.0 ** -4), 1: (2.0 ** -7, 2.0 ** -5)},
             "design": {0: (2.0 ** -6, 2.0 ** -6), 1: (2.0 ** -6, 2.0 ** -6), 2: (2.0 ** -6, 2.0 ** -6), 3: (2.0 ** -8, 2.0 ** -8)},
             "launch": {0: (2.0 ** -8, 2.0 ** -8), 2: (2.0 ** -12, 2.0 ** -7), 4: (2.0 ** -6, 2.0 ** -6), 5: (2.0 ** -12, 2.0 ** -7)}}
_E2E = {}


def retraced(kind, case, k, amount):
    """The oracle's frame of the system changed by parameter k, every ray on its unchanged sequence of surfaces, and the
    detector's id in it (a system built afresh draws new ids: the sequences are compared through the ids' order)."""
    import design_scenes
    import launch_scenes
    from test_host_sensitivity import moved_trace

    if kind == "motions":
        frame, counts, _ = moved_trace(case, k, amount)
    elif kind == "design":
        changed = design_scenes.build("lens", 257, change=(k, amount))
        frame, counts = changed.frame, changed.counts
    else:
        frame, counts = launch_scenes.retrace(case, k, amount)
    rank = lambda f: np.searchsorted(np.unique(f[:, 5]), f[:, 5])  # noqa: E731
    assert counts == case.counts, f"parameter {k}, {amount}: rays were lost or gained"
    assert np.array_equal(rank(frame), rank(case.frame)) and np.array_equal(frame[:, 4], case.frame[:, 4]), (
        f"parameter {k}, {amount}: a ray changed its surfaces")
    surface = np.unique(frame[:, 5])[np.searchsorted(np.unique(case.frame[:, 5]), case.surface.get_id())]
    return frame, surface


def e2e_differences(kind):
    """Per listed parameter (D(h), D(h / 2)) of the longdouble OTF, central differences over the oracle's re-traces: about
    the fixed centre (the unchanged frame's centroid, rounded to fp64) and about each re-trace's own centroid.  Computed
    once and shared."""
    if kind in _E2E:
        return _E2E[kind]
    case, parameters, kw = scene(kind)
    per_source, G = kw.get("rays_per_source"), kw.get("n_groups", 1)
    rows, group = M.selection(case.frame, case.surface.get_id(), per_source, G)
    f = case.frame
    centre = np.array([np.average(f[rows[group == g], 9:12], axis=0, weights=f[rows[group == g], 1]) for g in range(G)])

    def otf(frame, surface, about):
        at, groups = M.selection(frame, surface, per_source, G)
        return R.mtf_reference(frame[at, 9:12], frame[at, 12:15], frame[at, 1], groups, G, centre=about, **E2E_OPTIONS)

    out = {}
    for k, steps in E2E_STEPS[kind].items():
        pair = {}
        for (name, about), h in zip((("fixed", centre), ("centroid", None)), steps):
            values = []
            for step in (h, h / 2):
                plus, minus = (otf(*retraced(kind, case, k, s), about) for s in (step, -step))
                values.append(((plus.re - minus.re) / (2 * LD(step)), (plus.im - minus.im) / (2 * LD(step))))
            pair[name] = values
        out[k] = pair
    _E2E[kind] = (case, parameters, kw, centre, out)
    return _E2E[kind]


def richardson(what, got, coarse, fine):
    """|got - D(h/2)| <= |D(h) - D(h/2)| at every output, and |D(h) - D(h/2)| <= 1 % of the largest |dOTF|."""
    gap = np.hypot(coarse[0] - fine[0], coarse[1] - fine[1]).astype(float)
    miss = M.deviation(got, fine[0], fine[1])
    scale = float(np.abs(got).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(miss > 0, miss / gap, 0.0)
    print(f"[mtf gradient] {what}: largest |dOTF| {scale:.3e}, |D(h) - D(h/2)| <= {gap.max():.3e} ({gap.max() / scale:.2e} "
          f"of it), |device - D(h/2)| <= {miss.max():.3e}, worst |device - D(h/2)| / |D(h) - D(h/2)| {ratio.max():.3f}")
    assert np.all(miss <= gap), (what, float(ratio.max()))
    assert gap.max() <= 0.01 * scale, (what, gap.max(), scale)


@pytest.mark.parametrize("kind", ("motions", "design", "launch"))
def test_end_to_end_against_central_differences_of_the_oracle(kind):
    """sens.mtf_gradient on the device, from the one trace, against the differences of the re-traced systems: the centre
    held fixed, and following the centroid (the centre recomputed in every re-trace)."""
    case, parameters, kw, centre, differences = e2e_differences(kind)
    sens = traced_frame(case).sensitivity(case.surface, parameters, case.parts, slopes=True, **kw)
    assert not (sens.n_unknown or sens.n_invalid or sens.n_unfit)
    fixed = sens.mtf_gradient(centre=centre, **E2E_OPTIONS)
    follows = sens.mtf_gradient(reference="centroid", **E2E_OPTIONS)
    assert not fixed.n_missed.any() and not fixed.n_unfollowed.any() and fixed.n_rays.sum() == len(sens.rows())
    for k, pair in differences.items():
        richardson(f"{kind} parameter {k} ({type(parameters[k]).__name__}), fixed centre", fixed.dotf[:, k], *pair["fixed"])
        richardson(f"{kind} parameter {k} ({type(parameters[k]).__name__}), centroid", follows.dotf[:, k], *pair["centroid"])
    # the kernel's numbers on the traced frame are the reference's on the device's own jacobian and slopes
    rows = sens.rows().cpu().numpy()
    G = kw.get("n_groups", 1)
    group = np.floor(case.frame[rows, 4] / kw["rays_per_source"]).astype(int) if kw.get("rays_per_source") else np.zeros(len(rows), int)
    traced = SimpleNamespace(frame=case.frame, rows=rows, group=group, n_groups=G, jacobian=sens.jacobian.cpu().numpy(),
                             slopes=sens.slopes.cpu().numpy())
    check(f"{kind} traced", traced, fixed, E2E_OPTIONS, centre=centre)


def test_a_detector_moved_along_its_normal_changes_no_otf():
    """The config-2 detector shifted along x, its normal: every ray slides along itself, dQ = lambda u and duh = 0, so
    |dotf| is within the bound of zero (the focus derivative is not: the plane stays where the centre is)."""
    case, parameters, _ = scene("motions")
    sens = traced_frame(case).sensitivity(case.surface, [parameters[2]], case.parts, slopes=True)
    got = sens.mtf_gradient(**E2E_OPTIONS)
    rows = sens.rows().cpu().numpy()
    jacobian, slopes = sens.jacobian.cpu().numpy(), sens.slopes.cpu().numpy()
    assert np.abs(jacobian).max() > 0.5 and not slopes.any()
    traced = SimpleNamespace(frame=case.frame, rows=rows, group=np.zeros(len(rows), int), n_groups=1, jacobian=jacobian,
                             slopes=slopes)
    ref = check("detector along its normal", traced, got, E2E_OPTIONS)
    size = np.abs(got.dotf)
    print(f"[mtf gradient] detector along its normal: largest |dotf| {size.max():.3e}, bound there "
          f"{ref.dbound[:, :1].ravel()[size.argmax()]:.3e}; largest |dotf_dfocus| {np.abs(got.dotf_dfocus).max():.3e}")
    assert np.all(size <= ref.dbound[:, :1]) and np.abs(got.dotf_dfocus).max() > 1e6 * size.max()


# ---- the tracer ---------------------------------------------------------------------------------------------------------------
def test_trace_mtf_gradient_is_trace_sensitivity_then_mtf_gradient():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=257)
    parameters = [prt.Motion(lens, translate=(0, 1, 0)), prt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)),
                  prt.IndexChange(lens)]
    tracer.trace()
    before = tracer.get_results().copy()
    options = dict(azimuths=(0.0, 45.0), focus=(0.0, 0.01))
    got = tracer.trace_mtf_gradient(det, parameters, [0.0, 10.0, 30.0], reference="centroid", **options)
    assert tracer.get_results().equals(before)  # (the tracer's last result is left as it was)
    sens = tracer.trace_sensitivity(det, parameters, slopes=True)
    want = sens.mtf_gradient([0.0, 10.0, 30.0], reference="centroid", **options)
    assert isinstance(got, prt.MTFGradient) and got.dotf.shape == (1, 3, 2, 2, 3) and got.reference == "centroid"
    same_bits(got, want, "trace_mtf_gradient")
    assert_same_bits(got.dmtf, want.dmtf, "trace_mtf_gradient: dmtf")
    assert got.n_rays[0] == 257 and np.all(np.isfinite(got.dotf)) and got.parameters == tuple(parameters)
    step = want.step(damping=1e-3)
    assert step.shape == (1, 3) and np.all(np.isfinite(step))
    with pytest.raises(ValueError, match="slopes=True"):
        tracer.trace_sensitivity(det, parameters).mtf_gradient([10.0])
