"""The longdouble reference of the through-focus PSF (tests/psf_focus_reference.py) against closed forms, the mutations
its error budget must tell apart on the named cases the GPU tests run, PSFScan on the host and the argument refusals."""
import numpy as np
import pytest

import diffraction_reference as R
import psf_focus_reference as F

LD = np.longdouble


def designed(case, centre=None, pixel_size=None):
    """psf_inputs of a case's designed wavefront with u / v as offsets from a plane's centre, its p3 and its centre."""
    options = case.options
    step = options.get("pixel_size", 0.4 * R.LAMBDA_F) if pixel_size is None else pixel_size
    u, v = R.pixel_centres(options["pixels"], step, (0.0, 0.0))
    inp = case.inputs(u, v)
    return inp, F.sphere_axial(inp), tuple(options["centre"]) if centre is None else centre


def reference(inp, axial, focus, centre, track=True, **kw):
    """The reference with the line and the centres formed as the device forms them (longdouble line, rounded)."""
    line = F.chief_line(inp, axial)[0].astype(np.float64) if track else np.zeros((inp.n_groups, 2))
    return F.psf_focus_reference(inp, axial, focus, F.centres_of(line, focus, centre), line, **kw), line


def largest_ratio(mutated, ref):
    with np.errstate(invalid="ignore"):
        image = np.nanmax(np.abs(mutated.image - ref.image).astype(float) / ref.bound)
        strehl = np.nanmax(np.abs(mutated.strehl - ref.strehl).astype(float) / ref.strehl_bound)
    return float(image), float(strehl)


def test_the_plane_zero_is_the_psf_reference_exactly():
    case = R.psf_bucket_case()
    inp, axial, centre = designed(case)
    ref, line = reference(inp, axial, (0.0,), centre)
    absolute = case.inputs(centre[0] + inp.u, centre[1] + inp.v)
    want = R.psf_reference(absolute)
    assert np.array_equal(ref.image_by_wavelength[:, 0], want.image_by_wavelength, equal_nan=True)
    assert np.array_equal(ref.image[:, 0], want.image, equal_nan=True)
    assert np.array_equal(ref.strehl[:, 0], want.strehl, equal_nan=True)
    assert np.array_equal(ref.n_rays, want.n_rays) and np.array_equal(ref.n_missed, want.n_missed)
    # the budget has R's terms and more: it is never the smaller one
    finite = np.isfinite(want.bound)
    assert np.all(ref.bound[:, 0][finite] >= want.bound[finite])
    assert np.all(ref.strehl_bound[:, 0][finite.any(axis=(1, 2))] >= want.strehl_bound[finite.any(axis=(1, 2))])


def test_a_converging_wave_has_strehl_one_where_it_converges():
    n = 4096
    inp, axial, centre = designed(F.converging_case(n))
    ref, line = reference(inp, axial, (F.DELTA0, 0.0), centre, track=False)
    eps = float(np.finfo(LD).eps)
    assert abs(float(ref.strehl[0, 0] - 1)) <= 8 * n * eps
    # (the uniform disk's axial intensity is sinc^2 of the defocus, 0.480 here; the rays' obliquity makes it 0.495)
    assert abs(float(ref.strehl[0, 1]) - 0.495) < 0.002
    # the signs: near the axis the plane of convergence is bright, and a flipped delta or p3 is not that plane
    near = F.psf_focus_reference(inp, axial, (F.DELTA0,), np.array([[[0.3 * R.LAMBDA_F, 0.0]]]), np.zeros((1, 2)))
    flipped = F.psf_focus_reference(inp, -axial, (F.DELTA0,), np.array([[[0.3 * R.LAMBDA_F, 0.0]]]), np.zeros((1, 2)))
    mid = (inp.u.size // 2, inp.v.size // 2)
    assert float(near.image[0, 0][mid]) > 0.7 and float(flipped.image[0, 0][mid]) < 0.2


def test_a_ring_without_opd_has_on_axis_intensity_one_on_every_plane():
    t = (np.arange(360) + 0.5) / 360 * 2 * np.pi
    case = R.psf_case([[360]], pupil=(0.4 * np.cos(t), 0.4 * np.sin(t)), opd=np.zeros(360),
                      weights=lambda rng, n: np.ones(n))
    inp, axial, centre = designed(case)
    focus = np.linspace(-0.3, 0.3, 7)
    ref, line = reference(inp, axial, focus, centre, track=False, strehl_only=True)
    # (p1^2 + p2^2 and p3 are one number each only to fp64's rounding of cos and sin: R / lambda ulps of phase)
    assert np.abs(ref.strehl[0].astype(float) - 1).max() < 1e-9


def test_the_chief_line_follows_the_image():
    """A perfect wave from a displaced pupil converges at P.  One depth of focus on, its image has moved along the line
    through P and the mean sphere point: brighter there than at the mirrored point and than on the axis line."""
    case = F.offaxis_case(offsets=((0.25, -0.15),), n=800)
    inp, axial, centre = designed(case)
    inp.opd[:] = 0.0
    line = F.chief_line(inp, axial)[0].astype(np.float64)
    # (the mean of 800 random points of a disk of radius 0.3 lies within a few per cent of the offset)
    assert line[0, 0] == pytest.approx(0.25 / -10.0, rel=0.1) and line[0, 1] == pytest.approx(-0.15 / -10.0, rel=0.1)
    delta = (3 * F.DEPTH_OF_FOCUS,)
    at = [float(F.psf_focus_reference(inp, axial, delta, np.zeros((1, 1, 2)), t, strehl_only=True).strehl[0, 0])
          for t in (line, -line, np.zeros((1, 2)))]
    assert at[0] > 0.5 and at[0] > 2 * at[1] and at[0] > 1.5 * at[2]


MUTATED = {"ray slices": lambda: R.psf_slice_case(2049, R.PSF_FILLER), "buckets": R.psf_bucket_case,
           "converging": lambda: F.converging_case(1024)}


@pytest.mark.parametrize("name", sorted(MUTATED))
def test_the_bound_tells_the_mutations_apart(name):
    """On the cases the GPU tests run, at their shifts: a flipped delta, a flipped p3 and one ray dropped from a bucket
    each move the reference by more than the bound somewhere (in the image and in the Strehl ratio)."""
    inp, axial, centre = designed(MUTATED[name]())
    ref, line = reference(inp, axial, F.SHIFTS, centre)
    centres = F.centres_of(line, F.SHIFTS, centre)
    shifts = np.asarray(F.SHIFTS)
    last = int(np.flatnonzero(ref.n_rays.ravel())[-1])  # (a bucket with rays)
    mutations = {
        "delta flipped": F.psf_focus_reference(inp, axial, -shifts, centres, line),
        "p3 flipped": F.psf_focus_reference(inp, -axial, shifts, centres, line),
        "one ray dropped": F.psf_focus_reference(inp, axial, shifts, centres, line,
                                                 select=lambda b, n: np.arange(n)[1:] if b == last else np.arange(n)),
    }
    for what, mutated in mutations.items():
        image, strehl = largest_ratio(mutated, ref)
        print(f"[mutations] {name}, {what}: image {image:.3g} x bound, strehl {strehl:.3g} x bound")
        if ref.n_rays.ravel()[last] > 1:  # (a bucket of one ray dropped leaves |U| = 0: the share moves, not the shape)
            assert image > 1 and strehl > 1, (name, what, image, strehl)
    assert float(np.nanmax(ref.bound)) < 1e-5 and float(np.nanmax(ref.strehl_bound)) < 1e-9


def test_the_bound_tells_an_ignored_track_apart():
    inp, axial, centre = designed(F.offaxis_case())
    ref, line = reference(inp, axial, F.SHIFTS, centre)
    untracked, zero = reference(inp, axial, F.SHIFTS, centre, track=False)
    assert np.all(np.abs(line) > 0.004) and not zero.any()
    image, strehl = largest_ratio(untracked, ref)
    assert image > 1 and strehl > 1
    # the plane 0.0 is the same either way
    assert np.array_equal(untracked.image[:, 1], ref.image[:, 1]) and np.array_equal(untracked.strehl[:, 1], ref.strehl[:, 1])


def test_the_budget_refuses_what_it_does_not_count():
    inp, axial, centre = designed(R.psf_slice_case(255, 0))
    with pytest.raises(AssertionError, match="not what the budget counts"):
        reference(inp, axial, (4.0,), centre)  # (|delta| |p3| ~ 0.4 R^2)
    assert F.fused(0.1, 3.0, -0.3) != 0.1 * 3.0 - 0.3 and F.fused(0.0, float("nan"), 1.0) != F.fused(0.0, 2.0, 1.0)


# ---- PSFScan on the host ------------------------------------------------------------------------------------------------------
def scan_of(strehl, focus, centres=None, line=None):
    from pyrayt_amd.frame import PSFScan

    strehl = np.atleast_2d(np.asarray(strehl, dtype=float))
    G, n = strehl.shape
    image = np.broadcast_to(strehl[:, :, None, None, None], (G, n, 1, 3, 2)).copy()
    image[:, :, :, 1, 1] *= 2.0
    record = np.tile(np.array([10.0, 1.0, 10.0, 5.0]), (G, 1, 1))
    centres = np.zeros((G, n, 2)) if centres is None else centres
    return PSFScan(image, strehl, record, None, np.zeros((G, 2)) if line is None else line, centres, focus, [0.55], 1000.0,
                   (3, 2), (0.1, 0.2), (0.0, 0.0), np.full(G, 10.0), None)


def test_psfscan_best_focus_planes_and_tables():
    import pyrayt_amd
    from pyrayt_amd.frame import PSF

    assert pyrayt_amd.PSFScan is scan_of([[1.0]], [0.0]).__class__
    focus = np.array([0.3, -0.1, 0.1, -0.3, 0.0, 0.2, -0.2])  # (in no order)
    vertex = 0.07
    scan = scan_of([0.9 - 2.0 * (focus - vertex) ** 2, np.full(7, np.nan)], focus)
    best = scan.best_focus()
    assert best[0] == pytest.approx(vertex, abs=1e-12) and np.isnan(best[1])
    assert scan_of([[0.1, 0.5, 0.9]], [0.0, 0.1, 0.2]).best_focus()[0] == 0.2  # (at an end of the scan: the sample)
    table = scan.to_pandas()
    assert list(table.columns) == ["source_id", "focus", "strehl", "peak"] and len(table) == 14
    assert np.array_equal(table["focus"].to_numpy()[:7], focus) and table["peak"][0] == 2 * table["strehl"][0]
    assert scan.image.shape == (2, 7, 3, 2) and scan.u.tolist() == pytest.approx([-0.1, 0.0, 0.1]) and scan.n_rays.tolist() == [10, 10]
    one = scan.plane(0.1)
    assert isinstance(one, PSF) and one.image.shape == (2, 3, 2) and one.strehl[0] == scan.strehl[0, 2]
    assert one.to_pandas().shape[0] == 2 and one.encircled_energy(1.0)[0] == 1.0
    with pytest.raises(ValueError, match="not one of the sampled"):
        scan.plane(0.15)
    centres = np.zeros((2, 7, 2))
    centres[1, :, 0] = 0.5 * focus
    tracked = scan_of(scan.strehl, focus, centres)
    with pytest.raises(ValueError, match="group="):
        tracked.plane(0.1)
    assert tracked.plane(0.0).image.shape == (2, 3, 2)  # (the plane 0.0: one centre)
    mine = tracked.plane(0.2, group=1)
    assert mine.image.shape == (1, 3, 2) and mine.centre == (0.1, 0.0) and mine.u[1] == pytest.approx(0.1)


def test_focus_arguments_are_checked_before_the_gpu():
    from pyrayt_amd.frame import DeviceFrame, Fresnel

    frame = DeviceFrame(np.zeros((15, 3)), [3])
    for bad in ((), np.zeros(257), (0.0, np.nan), (np.inf,), "abc", np.zeros((2, 2))):
        with pytest.raises(ValueError, match="focus"):
            frame.psf(5.0, world_unit_um=1000.0, focus=bad)
    for bad in ("axis", 0, True, "Chief"):
        with pytest.raises(ValueError, match="track"):
            frame.psf(5.0, world_unit_um=1000.0, focus=(0.0,), track=bad)
    with pytest.raises(ValueError, match="fresnel= or group="):
        frame.psf(5.0, world_unit_um=1000.0, focus=(0.0,), group=object())
    with pytest.raises(ValueError, match="fresnel= or group="):
        frame.psf(5.0, world_unit_um=1000.0, focus=(0.0,), fresnel=object.__new__(Fresnel))
    with pytest.raises(NotImplementedError):  # (without focus the call is what it was)
        frame.psf(5.0, world_unit_um=1000.0, group=object(), track="anything")
