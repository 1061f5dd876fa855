"""PSF sensitivities on the device (Sensitivity.psf_gradient, the entry point prt_frame_psf_gradient, the kernels of
prt_psf_gradient.hpp) against the longdouble reference of tests/psf_gradient_reference.py, every output and parameter held
to the error budget derived there: at the edges of the LDS tile, the ray slices, the pixel tiles and the parameter chunks;
the bit contracts; closed forms (piston, tilt); and, end to end on frames the C oracle traced, against central differences of
``psf()`` over the oracle's own re-traces.  Each test prints its largest deviation / bound ratio."""
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import helpers
import psf_gradient_reference as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
GRID = dict(pixels=(3, 5), pixel_size=(2.5e-3, 3.0e-3), centre=(1e-3, -2e-3))
UNIT = 1000.0


def on(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    return DeviceFrame(on(np.asarray(frame, dtype=np.float64).T), counts)


def sensitivity_of(case, frame=None, rows=None, pick=None, opd=None, pupil=None):
    """A Sensitivity that holds the case's designed wavefront and synthetic derivatives for its selected rows: what
    psf_gradient reads.  ``pick``: the parameters kept."""
    from pyrayt_amd.frame import Sensitivity

    pick = slice(None) if pick is None else pick
    dopd, dfield, dpupil = case.dopd[pick], case.dfield[pick], case.dpupil[pick]
    n_par, G = len(dopd), case.n_groups
    device = device_frame(case.frame if frame is None else frame)
    first = np.searchsorted(case.group, np.arange(G + 1)).astype(np.int64)
    inp = case.inputs(np.zeros(1), np.zeros(1))
    made = Sensitivity(on(np.zeros((n_par, 3, len(case.rows)))), on(case.rows if rows is None else rows),
                       np.zeros((G, 6 + 4 * n_par + n_par * (n_par + 1) // 2)), np.zeros((G, 3)), True, (0, 0, 0, 0),
                       [f"p{k}" for k in range(n_par)],
                       launch=dict(slopes=None, rows=device._contiguous_rows(), weights="intensity", group_first=first))
    made.wavefront = SimpleNamespace(reference=np.zeros((G, 3)), radius=inp.radius, pivot=np.zeros(G),
                                     pupil_radius=np.nan_to_num(inp.rho, nan=1.0), n_rays=np.diff(first), terms=0)
    made.dopd, made.dfield, made.dpupil = on(dopd), on(dfield), on(dpupil)
    made.opd, made.pupil = on(inp.opd if opd is None else opd), on(inp.pupil if pupil is None else pupil)
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
    assert np.array_equal(np.isnan(got), nan), (family, what, "NaN pattern")
    if nan.all():
        return 0.0
    deviation = P.deviation(got, re, im)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | ((deviation == 0) & (bound == 0)), 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[psf gradient] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, {got.size} values)")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check(family, case, got, follow="ray", pick=None):
    """The device's PSFGradient against the reference on the same inputs, every output within its bound."""
    pick = slice(None) if pick is None else pick
    dphase, dpoint = (case.dopd[pick], case.dpupil[pick]) if follow == "ray" else (case.dfield[pick], None)
    inp = case.inputs(got.u, got.v)
    buckets = case.n_groups * len(inp.wavelengths)
    ref = P.gradient_reference(inp, dphase, dpoint, slices=P.slices(len(case.rows), buckets, len(got.u) * len(got.v), cus()))
    for name in ("n_rays", "n_missed", "n_unfollowed"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), (family, name, getattr(got, name), getattr(ref, name))
    hold(family, "amplitude", got.amplitude, *ref.amplitude, ref.amplitude_bound)
    hold(family, "damplitude", got.damplitude, *ref.damplitude, ref.damplitude_bound)
    hold(family, "image_by_wavelength", got.image_by_wavelength, ref.image_by_wavelength, None, ref.bound_by_wavelength)
    hold(family, "dimage_by_wavelength", got.dimage_by_wavelength, ref.dimage_by_wavelength, None, ref.dbound_by_wavelength)
    hold(family, "image", got.image, ref.image, None, ref.bound)
    hold(family, "dimage", got.dimage, ref.dimage, None, ref.dbound)
    hold(family, "strehl", got.strehl, ref.strehl, None, ref.strehl_bound)
    hold(family, "dstrehl", got.dstrehl, ref.dstrehl, None, ref.dstrehl_bound)
    return ref


def outputs(got):
    return dict(amplitude=got.amplitude, damplitude=got.damplitude, image=got.image_by_wavelength,
                dimage=got.dimage_by_wavelength, strehl=got.strehl, dstrehl=got.dstrehl, record=got.record)


def assert_same_bits(got, want, what):
    parts = lambda x: np.ascontiguousarray(x).view(np.float64) if np.iscomplexobj(x) else np.ascontiguousarray(x)  # noqa: E731
    helpers.assert_same_bits(parts(got), parts(want), what)


def same_bits(a, b, what):
    for key, value in outputs(a).items():
        assert_same_bits(value, outputs(b)[key], f"{what}: {key}")


def gradient_of(case, **kw):
    options = dict(world_unit_um=UNIT, **GRID)
    options.update({k: kw.pop(k) for k in ("pixels", "pixel_size", "centre", "follow") if k in kw})
    return sensitivity_of(case, **kw).psf_gradient(**options)


# ---- the kernels against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.SIZES)
def test_ray_tiles_and_slices_alone_and_among_other_rows(n):
    """Rays of a bucket about the LDS tile (kPsfBlock = 256) and the slice (kPsfgMinSlice = 2048; 4097 rays are two slices
    of 2049 and 2048): alone in the frame and among 4196 rows of another surface, which change nothing -- the partition
    follows the selection alone -- so the two runs give the same bits."""
    assert (R.K.kPsfBlock, P.K.kPsfgMinSlice) == (256, 2048)
    assert P.slices(n, 1, 15, cus()) == (2 if n == 4097 else 1)
    case = P.gradient_case([[n]], 3, seed=100 + n)
    got = gradient_of(case)
    check(f"{n} rays", case, got)
    frame, rows = among_other_rows(case, 2 * 2048 + 100)
    other = gradient_of(case, frame=frame, rows=rows)
    same_bits(got, other, f"{n} rays among other rows")


@pytest.mark.parametrize("grid", P.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_pixel_tiles(grid):
    """Pixel grids about the tile of 1024 pixels: one pixel, a small odd grid, one tile exactly, one short, two tiles."""
    assert -(-grid[0] * grid[1] // R.K.kPsfTile) == (2 if grid == (33, 32) else 1)
    case = P.gradient_case([[257]], 2, seed=40 + grid[0] * grid[1])
    got = gradient_of(case, pixels=grid, pixel_size=(4e-4, 5e-4))
    assert got.dimage.shape == (1, 2) + grid
    check(f"{grid[0]}x{grid[1]} pixels", case, got)


@pytest.mark.parametrize("n_parameters", P.PARAMETER_COUNTS)
def test_parameter_chunks(n_parameters):
    """K = 1, 3, 4, 5, 9 and 16 about the chunk of kPsfgParams = 4 accumulator sets: the instantiation of 1, of 4 with
    an empty column, of 4 whole, 4 and then 1, two chunks in one launch and then 1, four chunks in one launch."""
    assert P.K.kPsfgParams == 4
    case = P.gradient_case([[300]], n_parameters, seed=60 + n_parameters)
    got = gradient_of(case)
    assert got.dimage.shape == (1, n_parameters, 3, 5) and got.dstrehl.shape == (1, n_parameters)
    check(f"K = {n_parameters}", case, got)


@pytest.mark.parametrize("follow", ("ray", "pupil"))
def test_two_wavelengths_two_groups_one_empty_and_rays_left_out(follow):
    """Two groups, the second without rays (NaN), two wavelengths; per bucket 3 rays with a NaN OPD (n_missed) and 4 with
    a NaN derivative of one parameter (n_unfollowed): out for every parameter, counted, and the sums as the reference
    has them without those rays."""
    case = P.gradient_case([[300, 170], [0, 0]], 5, seed=81, wavelengths=(0.45, 0.65), missed=3, unfollowed=4)
    got = gradient_of(case, follow=follow)
    check(f"buckets, follow={follow}", case, got, follow=follow)
    assert got.n_missed.tolist() == [[3, 3], [0, 0]] and got.n_unfollowed.tolist() == [[4, 4], [0, 0]]
    assert got.n_rays.tolist() == [[293, 163], [0, 0]] and got.follow == follow
    assert np.all(np.isfinite(got.dimage[0])) and np.all(np.isfinite(got.dstrehl[0])) and np.all(np.isfinite(got.damplitude[0]))
    for value in (got.image[1], got.dimage[1], got.amplitude[1], got.damplitude[1], got.strehl[1], got.dstrehl[1]):
        assert np.all(np.isnan(value))
    np.testing.assert_array_equal(got.image, got.image_by_wavelength.sum(axis=1))
    table = got.to_pandas()
    assert table["n_rays"].tolist() == [456, 0] and table["n_unfollowed"].tolist() == [8, 0]


def test_two_runs_give_the_same_bits():
    case = P.gradient_case([[2500, 1700], [300, 0]], 9, seed=97, wavelengths=(0.5, 0.6), missed=2)
    first = gradient_of(case, pixels=(9, 7))
    second = gradient_of(case, pixels=(9, 7))
    same_bits(first, second, "run to run")


def test_a_parameter_alone_has_the_bits_it_has_among_sixteen():
    """Every ray is followed, so the kept set is the same: parameter k alone (the instantiation of 1) against parameter k
    among sixteen (four chunks of 4), and the image and the Strehl ratio of both calls."""
    case = P.gradient_case([[300]], 16, seed=56)
    among = gradient_of(case)
    for k in range(16):
        alone = gradient_of(case, pick=slice(k, k + 1))
        assert_same_bits(alone.dimage_by_wavelength[:, 0], among.dimage_by_wavelength[:, k], f"parameter {k} alone: dimage")
        assert_same_bits(alone.damplitude[:, 0], among.damplitude[:, k], f"parameter {k} alone: damplitude")
        assert_same_bits(alone.dstrehl[:, 0], among.dstrehl[:, k], f"parameter {k} alone: dstrehl")
        assert_same_bits(alone.image_by_wavelength, among.image_by_wavelength, f"parameter {k} alone: image")
        assert_same_bits(alone.strehl, among.strehl, f"parameter {k} alone: strehl")


def test_image_is_the_psf_passes_within_the_two_budgets():
    """image of psf_gradient against frame.psf() of the same rays, the wavefront's own opd and pupil handed over: within
    the two passes' budgets added; the bits are not promised (psf() sorts the rows in row order, this pass takes the
    selection's).  The Strehl ratios likewise."""
    case = P.gradient_case([[700, 300], [400, 250]], 2, seed=99, wavelengths=(0.5, 0.6))
    options = dict(case.options, pixels=(9, 7), pixel_size=(4e-4, 5e-4), centre=(1e-4, 0.0))
    plain = device_frame(case.frame).psf(R.SURFACE, **options)
    order = case.to_selection
    opd, pupil = plain.wavefront.opd.cpu().numpy()[order], plain.wavefront.pupil.cpu().numpy()[order]
    made = sensitivity_of(case, opd=opd, pupil=pupil)
    made.wavefront.radius, made.wavefront.pupil_radius = plain.wavefront.radius, plain.wavefront.pupil_radius
    got = made.psf_gradient(world_unit_um=UNIT, pixels=(9, 7), pixel_size=(4e-4, 5e-4), centre=(1e-4, 0.0))
    inp = R.psf_inputs(case.group, case.inputs(got.u, got.v).wavelength, opd, pupil, case.inputs(got.u, got.v).weight,
                       plain.wavefront.radius, plain.wavefront.pupil_radius, got.wavelengths, UNIT, got.u, got.v, 2)
    ref = R.psf_reference(inp)
    apart = np.abs(plain.image_by_wavelength - got.image_by_wavelength)
    print(f"[psf gradient] image against psf(): largest difference {apart.max():.3e}, difference / (2 bound) "
          f"{(apart / (2 * ref.bound_by_wavelength)).max():.3f}")
    assert np.all(apart <= 2 * ref.bound_by_wavelength)
    assert np.all(np.abs(plain.strehl - got.strehl) <= 2 * ref.strehl_bound)
    assert np.array_equal(plain.record[:, :, 0].astype(int), got.n_rays)


def test_a_piston_changes_no_image():
    """dphase constant over the rays and dpoint zero: dU = 2 pi i e U, a turn of the amplitude's phase, so dimage and
    dstrehl are within their bounds of zero while damplitude is not small."""
    case = P.gradient_case([[400, 300]], 3, seed=31, wavelengths=(0.5, 0.6), piston=1)
    got = gradient_of(case, pixels=(9, 7), pixel_size=(4e-4, 5e-4))
    ref = check("piston", case, got)
    size, dsize = np.abs(got.dimage[:, 1]), np.abs(got.dstrehl[:, 1])
    print(f"[psf gradient] piston: largest |dimage| {size.max():.3e} (bound there {ref.dbound[:, 1].ravel()[size.argmax()]:.3e}), "
          f"|dstrehl| {dsize.max():.3e} (bound {ref.dstrehl_bound[:, 1].max():.3e}); largest |damplitude| {np.abs(got.damplitude[:, 1]).max():.3e}")
    assert np.all(size <= ref.dbound[:, 1]) and np.all(dsize <= ref.dstrehl_bound[:, 1])
    assert np.abs(got.damplitude[:, 1]).max() > 1e6 * size.max()


def test_a_tilt_shifts_the_image():
    """dphase = -(t.p) / R with dpoint zero adds to every ray's phase what moving the pixel by t adds to first order in
    rho / R: dimage = -(shift).grad(image) with the shift -t, that is t.grad(image).  The slope is the image's own central
    difference on a fine grid, at the spacing h and at h / 2 (every second pixel of one grid of spacing h / 2); the
    derivative is held within that difference's Richardson gap, to which the rounding the differences themselves carry
    (2 psf_bound / (h / 2), and the derivative's own bound) is added; the gap must be ten times that rounding."""
    t = (0.8, -0.6)
    case = P.gradient_case([[500]], 2, seed=33, tilt=(0, t))
    # h / 2.  The Airy radius is 1.22 lambda R / (2 rho) = 6.7e-3: the gap, about (2 pi h / 1.1e-2)^2 / 8 of the slope, is
    # 0.6 % of it at h = 3e-4, and the rounding of the differences themselves, 2 psf_bound / (h / 2), thirty times less
    half = 1.5e-4
    got = gradient_of(case, pixels=(13, 13), pixel_size=(half, half), centre=(1.5e-3, 1e-3))
    image, dimage = got.image[0], got.dimage[0, 0]

    def slope(step):
        inner = image[2:-2, 2:-2]
        du = (image[2 + step:image.shape[0] - 2 + step, 2:-2] - image[2 - step:image.shape[0] - 2 - step, 2:-2]) / (2 * step * half)
        dv = (image[2:-2, 2 + step:image.shape[1] - 2 + step] - image[2:-2, 2 - step:image.shape[1] - 2 - step]) / (2 * step * half)
        assert du.shape == dv.shape == inner.shape
        return t[0] * du + t[1] * dv

    coarse, fine = slope(2), slope(1)
    gap, miss = np.abs(coarse - fine), np.abs(dimage[2:-2, 2:-2] - fine)
    ref = check("tilt", case, got)
    noise = 2 * (ref.bound[0, 2:-2, 2:-2].max() / half) + ref.dbound[0, 0].max()  # (the differences' own rounding)
    print(f"[psf gradient] tilt: largest |dimage| {np.abs(dimage).max():.3e}, gap <= {gap.max():.3e}, miss <= {miss.max():.3e}, "
          f"worst miss / (gap + noise) {(miss / (gap + noise)).max():.3f}, noise {noise:.3e}")
    assert gap.max() <= 0.01 * np.abs(dimage).max() and gap.max() >= 10 * noise
    assert np.all(miss <= gap + noise)


def test_step_recovers_a_known_change():
    """step(0, image + dimage . delta) returns delta: the normal equations of an exactly linear target, to their
    conditioning (cond(J^T J) times fp64's unit roundoff)."""
    case = P.gradient_case([[600]], 3, seed=35)
    got = gradient_of(case, pixels=(9, 9), pixel_size=(6e-4, 6e-4))
    delta = np.array([[2e-3, -1e-3, 1.5e-3]])
    target = got.image + np.einsum("gkij,gk->gij", got.dimage, delta)
    jac = got.dimage[0].reshape(3, -1).T
    cond = np.linalg.cond(jac.T @ jac)
    step = got.step(0.0, target)
    print(f"[psf gradient] step: cond(J^T J) {cond:.3e}, |step - delta| {np.abs(step - delta).max():.3e}")
    assert cond < 1e8
    assert np.abs(step - delta).max() <= 16 * cond * 2.0 ** -53 * np.abs(delta).max()


# ---- end to end: the device against central differences of psf() over the oracle's re-traces -------------------------------
def traced_frame(case):
    from test_gpu_design_sensitivity import device_frame as traced

    return traced(case.frame, case.counts)


def richardson(what, got, coarse, fine, floor):
    """The rule of tests/test_gpu_mtf_gradient.py: |got - D(h/2)| <= |D(h) - D(h/2)| at every value, and
    |D(h) - D(h/2)| <= 1 % of the largest |derivative|.  The differences here come from ``psf()``, whose fp32 phasors
    leave ``floor`` = psf_bound / h + psf_bound / (h / 2) in the gap of a value: it is added to that value's gap, so
    that a value whose own truncation is under the differences' rounding (a pixel where the third derivative passes
    through zero) is held to that rounding; the caller asserts that the largest gap is ten times the largest floor.
    Returns the worst |got - D(h/2)| / (gap + floor)."""
    gap = np.abs(coarse - fine) + floor
    miss = np.abs(got - fine)
    scale = float(np.abs(got).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(miss > 0, miss / gap, 0.0)
    print(f"[psf gradient] {what}: largest |d| {scale:.3e}, |D(h) - D(h/2)| <= {gap.max():.3e} ({gap.max() / scale:.2e} of it), "
          f"|device - D(h/2)| <= {miss.max():.3e}, worst |device - D(h/2)| / |D(h) - D(h/2)| {ratio.max():.3f}")
    assert np.all(miss <= gap), (what, float(ratio.max()))
    assert gap.max() <= 0.01 * scale, (what, gap.max(), scale)
    return float(ratio.max())


E2E_PIXELS = (3, 3)
# micrometres per world unit: the scenes have no unit of their own.  The dish's beam is slow (NA 1e-3) and its detector 0.002
# wide, so a step that turns the phase by 0.1 rad keeps every ray on the detector only where a world unit is a metre
E2E_UNIT = {"singlet": 1000.0, "two_fields": 1000.0, "dish_axial": 1e6}


@pytest.mark.parametrize("name", ("singlet", "two_fields", "dish_axial"))
def test_end_to_end_against_central_differences_of_the_oracle(name):
    """follow="ray" dimage and dstrehl from the one trace against central differences of ``psf()`` over the C oracle's
    re-traces at h and h / 2, with P, R and the pixel grid held fixed.  The Strehl ratio is the image at P: it is held
    as one more pixel of the image, so that the rule's 1 % is taken of the largest derivative over the grid and P (a
    Strehl ratio at its extremum, as the dish's is along its axis, has no scale of its own).  h is chosen from ``psf()`` and the sensitivity
    pass alone, never from the gradient: starting where the largest phase change, 2 pi s h max|dopd_k - its group's
    mean| (a piston changes no image), is between 0.25 and 0.5 rad, h is halved until the truncation gap
    |D(h) - D(h/2)| is under 0.8 % of the largest |D(h/2)|, and then scaled so that the gap, which falls as h^2, is
    0.7 % -- about the largest h the rule's 1 % admits, while what psf()'s fp32 phasors leave in a difference,
    psf_bound / h, rises as 1 / h.  The test asserts that the largest gap is at least ten times the largest floor, so a
    gap made of noise cannot pass.  Observed (MI355X): |device - D(h/2)| / gap is 0.33 to 0.35, pure truncation, at
    every value whose gap is above the floor."""
    import opd_scenes

    case = opd_scenes.build(name, 257)
    per_source = getattr(case, "rays_per_source", None)
    kw = dict(rays_per_source=per_source, n_groups=2) if per_source else {}
    dev = traced_frame(case)
    centred = dev.wavefront(case.surface, weights="intensity", **kw)
    lam, unit = float(np.unique(case.frame[:, 2])[0]), E2E_UNIT[name]
    f_number = float(np.min(centred.radius / (2 * centred.pupil_radius)))
    side = lam / unit * f_number / 2
    # P a third of a pixel off the centroid, so that no derivative at P vanishes by the scene's symmetry (the dish's is
    # even in a translation across its axis: at the centroid the differences of the Strehl ratio would be zero bar rounding)
    wave = dev.wavefront(case.surface, weights="intensity", radius=centred.radius,
                         reference=centred.reference + np.array([0.0, 0.3 * side, -0.2 * side]), **kw)
    sens = dev.sensitivity(case.surface, list(case.parameters), case.parts, wavefront=wave, **kw)
    assert not (sens.n_unknown or sens.n_invalid or sens.n_unfit)
    grid = dict(world_unit_um=unit, pixels=E2E_PIXELS, pixel_size=(side, side), centre=(0.3 * side, -0.2 * side))
    got = sens.psf_gradient(**grid)
    assert not got.n_missed.any() and not got.n_unfollowed.any() and got.n_rays.sum() == len(sens.rows())
    s = unit / lam
    dopd = sens.dopd.cpu().numpy()
    rows = sens.rows().cpu().numpy()
    group = np.floor(case.frame[rows, 4] / per_source).astype(int) if per_source else np.zeros(len(rows), int)
    G = 2 if per_source else 1
    worst = 0.0

    def differences(k, step):
        """(D(step) of the image and of the Strehl ratio, psf_bound / step of the two images) over the re-traces."""
        sides = []
        for sign in (1, -1):
            moved = opd_scenes.build(name, 257, change=(k, sign * step))
            assert moved.counts == case.counts, f"parameter {k}, {sign * step}: rays were lost or gained"
            sides.append(traced_frame(moved).psf(moved.surface, reference=wave.reference, radius=wave.radius, **grid, **kw))
        floor = np.maximum(*(R.psf_bound(p.image, 1.0, R.EPS_TRIG + 2 * np.pi * R.F32_TURN) for p in sides)) / step
        floor = np.concatenate([floor.reshape(G, -1), np.zeros((G, 1))], axis=1)  # (the Strehl ratio's sums are fp64)
        with_p = lambda p: np.concatenate([p.image.reshape(G, -1), p.strehl[:, None]], axis=1)  # noqa: E731
        return (with_p(sides[0]) - with_p(sides[1])) / (2 * step), floor

    for k in range(len(case.parameters)):
        spread = max(np.abs(dopd[k, group == g] - dopd[k, group == g].mean()).max() for g in range(G))
        h = 2.0 ** np.floor(np.log2(0.5 / (2 * np.pi * s * spread)))
        coarse = differences(k, h)
        for _ in range(4):  # (from a phase change of 0.25 to 0.5 rad down: the largest h whose gap is under 1 %)
            fine = differences(k, h / 2)
            if np.abs(coarse[0] - fine[0]).max() <= 0.008 * np.abs(fine[0]).max():
                break
            h, coarse = h / 2, fine
        # ... and from there the h at which the gap, which falls as h^2, is 0.7 %
        share = np.abs(coarse[0] - fine[0]).max() / np.abs(fine[0]).max()
        h = h * min(2.0, float(np.sqrt(0.007 / share)))
        coarse, fine = differences(k, h), differences(k, h / 2)
        floor = fine[1]
        gap = np.abs(coarse[0] - fine[0])
        print(f"[psf gradient] {name} parameter {k} ({type(case.parameters[k]).__name__}): h = {h:.3e}, "
              f"gap {gap.max():.3e}, floor psf_bound / h {floor.max():.3e}")
        assert gap.max() >= 10 * floor.max(), (name, k, gap.max(), floor.max())
        mine = np.concatenate([got.dimage[:, k].reshape(G, -1), got.dstrehl[:, k, None]], axis=1)
        worst = max(worst, richardson(f"{name} parameter {k} dimage and dstrehl", mine, coarse[0], fine[0], coarse[1] + fine[1]))
    print(f"[psf gradient] {name}: worst |device - D(h/2)| / |D(h) - D(h/2)| {worst:.3f}")
    # the kernel's numbers on the traced frame are the reference's on the device's own wavefront and derivatives
    traced = SimpleNamespace(
        rows=rows, n_groups=G, dopd=dopd, dfield=sens.dfield.cpu().numpy(), dpupil=sens.dpupil.cpu().numpy(),
        inputs=lambda u, v: R.psf_inputs(group, case.frame[rows, 2], sens.opd.cpu().numpy(), sens.pupil.cpu().numpy(),
                                         case.frame[rows, 1], wave.radius, wave.pupil_radius, [lam], unit, u, v, G))
    check(f"{name} traced", traced, got)


# ---- the tracer ---------------------------------------------------------------------------------------------------------------
def test_trace_psf_gradient_is_trace_sensitivity_then_psf_gradient():
    import pyrayt_amd as prt

    lens = prt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    det = prt.components.baffle((1, 1)).move_x(1)
    source = prt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    tracer = prt.RayTracer(source, [lens, det], rays_per_source=257)
    parameters = [prt.Motion(lens, translate=(0, 1, 0)), prt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)),
                  prt.IndexChange(lens)]
    tracer.trace()
    before = tracer.get_results().copy()
    options = dict(world_unit_um=UNIT, pixels=(5, 4), centre=(0.0, 1e-4))
    got = tracer.trace_psf_gradient(det, parameters, follow="pupil", **options)
    assert tracer.get_results().equals(before)  # (the tracer's last result is left as it was)
    sens = tracer.trace_sensitivity(det, parameters, wavefront=True)
    want = sens.psf_gradient(follow="pupil", **options)
    assert isinstance(got, prt.PSFGradient) and got.dimage.shape == (1, 3, 5, 4) and got.follow == "pupil"
    same_bits(got, want, "trace_psf_gradient")
    assert got.n_rays.sum() == 257 and np.all(np.isfinite(got.dimage)) and got.parameters == tuple(parameters)
    step = want.step(damping=1e-3, target=np.zeros_like(want.image))
    assert step.shape == (1, 3) and np.all(np.isfinite(step))
    with pytest.raises(ValueError, match="wavefront="):
        tracer.trace_sensitivity(det, parameters).psf_gradient(world_unit_um=UNIT)
    with pytest.raises(ValueError, match="WavelengthChange"):
        tracer.trace_psf_gradient(det, parameters + [prt.WavelengthChange()], world_unit_um=UNIT)
