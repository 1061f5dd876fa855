"""The polarised diffraction PSF (DeviceFrame.psf(fresnel=), k_vpsf_huygens, k_vpsf_strehl, k_vpsf_fold) against the
longdouble reference of tests/vector_psf_reference.py: every pixel of the five Stokes planes, both Strehl ratios and the
throughput held to the budget derived there, at the edges of the LDS tile, the ray slices and the pixel tiles, over
states, wavelengths and groups.  The fields are synthetic tensors handed to a Fresnel; each test prints its largest
deviation and its ratio to the bound."""
import numpy as np
import pytest

import diffraction_reference as R
import vector_psf_reference as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
K = V.K
E1 = V.world_field(np.array([1.0, 0.0, 0.0]))


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def fresnel_of(device, field, polarised):
    """A Fresnel of ``device`` with the given (6, n_rows) field, as fresnel(fields=True) would hold it."""
    from pyrayt_amd.frame import Fresnel

    n = field.shape[1]
    return Fresnel(device, torch.ones(n, dtype=torch.float64, device="cuda:0"), torch.from_numpy(field).to("cuda:0"),
                   np.zeros(6, dtype=np.int64), polarization=np.array([0.0, 1.0, 0.0]) if polarised else None)


def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


def hold(family, what, got, want, bound):
    """|got - want| <= bound at every element (NaN where, and only where, the reference is NaN); the figures printed."""
    got, bound = np.asarray(got, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (family, what, got.shape, want.shape, bound.shape)
    nan = np.isnan(want.astype(np.float64))
    assert np.array_equal(np.isnan(got), nan), (family, what, "NaN pattern")
    if nan.all():
        return 0.0
    deviation = np.abs(got.astype(LD) - want).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | (deviation == 0), 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[vector psf] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, {got.size} values)")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


def planes_of(got):
    """(G, L, 5, nx, ny): S0..S3 and axial, by wavelength."""
    return np.concatenate([got.stokes_by_wavelength, got.axial_by_wavelength[:, :, None]], axis=2)


def run(family, case, field, polarised, missed=0):
    device = device_frame(case.frame)
    got = device.psf(R.SURFACE, weights="intensity", fresnel=fresnel_of(device, field, polarised), **case.options)
    G, rps = case.options["n_groups"], case.options["rays_per_source"]
    inp = R.psf_inputs_from(case.frame, got, R.SURFACE, rps, G)
    rows = V.selected_rows(case.frame, R.SURFACE, rps, G)
    states = 1 if polarised else 2
    nx, ny = len(got.u), len(got.v)
    slices = V.vpsf_slices(case.n_rows, G * len(got.wavelengths), states, nx * ny, compute_units())
    ref = V.vector_psf_reference(inp, V.field_of_rows(field, rows), states, slices=slices)
    assert got.n_states == states and got.record.shape == (G, len(got.wavelengths), states, 6)
    for state in range(states):
        assert np.array_equal(got.record[:, :, state, 0], ref.n_rays) and np.array_equal(got.record[:, :, state, 1], ref.n_missed)
    assert np.array_equal(got.n_rays, ref.n_rays.sum(axis=1)) and np.array_equal(got.n_missed, ref.n_missed.sum(axis=1))
    assert int(ref.n_missed.sum()) == missed and int(ref.n_rays.sum()) == int(case.counts.sum()) - missed
    hold(family, "stokes_by_wavelength", planes_of(got), ref.stokes_by_wavelength, ref.bound_by_wavelength)
    hold(family, "stokes", np.concatenate([got.stokes, got.axial[:, None]], axis=1), ref.stokes, ref.bound)
    hold(family, "image_by_wavelength", got.image_by_wavelength, ref.image_by_wavelength, ref.image_bound_by_wavelength)
    hold(family, "image", got.image, ref.image, ref.image_bound)
    hold(family, "strehl", got.strehl, ref.strehl, ref.strehl_bound)
    hold(family, "strehl_apodized", got.strehl_apodized, ref.strehl_apodized, ref.strehl_apodized_bound)
    hold(family, "throughput", got.throughput, ref.throughput, ref.throughput_bound)
    return got, ref, slices, inp


@pytest.mark.parametrize("filler", (0, R.PSF_FILLER), ids=("alone", "among_other_rows"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 2047, 2048, 2049))
def test_rays_of_a_bucket_about_the_lds_tile_and_the_slice(n, filler):
    """Rays of a bucket about the LDS tile (kPsfBlock = 256 rays of 72 bytes) and the slice (kPsfMinSlice = 2048): alone
    in the frame (one slice), and among 4196 rows of another surface, which raise n_rows and with it the slices (2 or 3)
    over the same rays; at one ray a slice that starts where the bucket ends.  Unpolarised complex fields."""
    assert (K.kPsfBlock, K.kPsfMinSlice) == (256, 2048)
    case = R.psf_slice_case(n, filler)
    got, ref, slices, _ = run("ray slices", case, V.random_field(case.n_rows, True, 200 + n), polarised=False)
    assert slices == max(1, (n + filler) // K.kPsfMinSlice)
    if filler:
        assert slices >= 2


@pytest.mark.parametrize("grid", R.PSF_GRIDS + R.PSF_GRIDS_WITHIN_THE_CAP, ids=lambda g: f"{g[0]}x{g[1]}")
def test_pixel_tiles(grid):
    """The pixels of a workgroup, kPsfBlock * kVpsfPix: one pixel, one short of a tile, a whole tile, one past it, five
    tiles with the last partial; a side of 1025 is refused as the scalar PSF refuses it, so a whole tile as one row and
    as one column, and 1026 pixels in two rows / two columns, stand in.  Off-centre, du != dv.  A real polarised field."""
    assert K.kVpsfTile == K.kPsfBlock * K.kVpsfPix == 1024
    case = R.psf_tile_case(grid)
    field = V.random_field(case.n_rows, False, 300 + grid[0])
    if max(grid) > 1024:
        device = device_frame(case.frame)
        with pytest.raises(ValueError, match="1..1024"):
            device.psf(R.SURFACE, weights="intensity", fresnel=fresnel_of(device, field, True), **case.options)
        return
    got, ref, slices, _ = run("pixel tiles", case, field, polarised=True)
    assert slices == 1 and got.stokes.shape == (1, 4) + grid and got.axial.shape == (1,) + grid


@pytest.mark.parametrize("wavelengths", (1, 3))
@pytest.mark.parametrize("polarised", (True, False), ids=("one_state", "two_states"))
def test_states_wavelengths_and_groups(polarised, wavelengths):
    """Two groups: three wavelengths with buckets of 1, 300 and 4000 rays and a second group without rays (NaN), or one
    wavelength with 300 rays and none.  Random complex fields; every output against the reference."""
    if wavelengths == 3:
        case = R.psf_bucket_case()
    else:
        case = R.psf_case([[300], [0]], pixels=(9, 7), pixel_size=0.4 * R.LAMBDA_F, centre=(0.0, 0.2 * R.LAMBDA_F),
                          opd_waves=0.1, filler=10_000, seed=6)
    got, ref, slices, _ = run("states, wavelengths, groups", case, V.random_field(case.n_rows, True, 17), polarised)
    assert slices == case.n_rows // (2 * wavelengths * K.kPsfMinSlice) == 2
    assert np.all(np.isnan(got.stokes[1])) and np.isnan(got.strehl[1]) and np.isnan(got.throughput[1])
    assert np.all(np.isfinite(got.stokes[0])) and got.strehl[0] > 0 and got.strehl_apodized[0] > 0


def test_a_constant_real_field_gives_the_scalar_psf():
    """Field e1 on every ray: S0 within the summed bounds of the scalar psf() of the same frame, S1 == S0 and
    S2 == S3 == axial == 0 exactly (the other components' amplitudes are exact zeros), strehl within bound of the
    scalar's."""
    case = R.psf_slice_case(2049, R.PSF_FILLER)
    got, ref, slices, inp = run("constant e1", case, V.constant_field(case.n_rows, E1), polarised=True)
    device = device_frame(case.frame)
    scalar = device.psf(R.SURFACE, weights="intensity", **case.options)
    scalar_ref = R.psf_reference(inp, slices=R.psf_slices(case.n_rows, 1, 63, compute_units()))
    hold("constant e1", "S0 against the scalar image", got.stokes[:, 0], scalar.image.astype(LD), ref.bound[:, 0] + scalar_ref.bound)
    hold("constant e1", "strehl against the scalar's", got.strehl, scalar.strehl.astype(LD), ref.strehl_bound + scalar_ref.strehl_bound)
    assert np.array_equal(got.stokes[:, 1], got.stokes[:, 0])
    assert not got.stokes[:, 2:].any() and not got.axial.any()
    assert np.array_equal(got.n_rays, scalar.n_rays) and got.throughput[0] == 1.0
    hold("constant e1", "strehl_apodized is strehl", got.strehl_apodized, got.strehl.astype(LD), ref.strehl_apodized_bound)


def test_a_phase_per_ray_in_the_field_adds_to_the_opd():
    """Field exp(i phi_r) e1 against the scalar reference with phi_r / 2 pi turns added to the phases."""
    case = R.psf_slice_case(2049, R.PSF_FILLER)
    rows = V.selected_rows(case.frame, R.SURFACE, case.options["rays_per_source"], 1)
    phi = np.random.default_rng(31).uniform(-np.pi, np.pi, len(rows))
    field = np.zeros((6, case.n_rows), dtype=complex)
    field[0:3, rows] = E1[:, None] * np.exp(1j * phi)[None, :]
    got, ref, slices, inp = run("phase in the field", case, field, polarised=True)
    scalar = R.psf_reference(inp, offset=lambda b, n: phi.astype(LD) / R.TWO_PI, slices=slices)
    hold("phase in the field", "S0 against psf_reference(offset=phi / 2 pi)", got.stokes[:, 0], scalar.image, scalar.bound)
    hold("phase in the field", "strehl", got.strehl, scalar.strehl, scalar.strehl_bound)
    assert got.strehl[0] < 0.01 < got.throughput[0]  # (2049 random phases: the image is gone, the energy is not)


def test_radial_polarisation_has_a_dark_centre():
    """A 4096-ray Vogel disk whose field points along the pupil radius: S0 at P stays within its bound of the
    reference's 1e-8, where adding the components as scalars gives 1."""
    case, field = V.radial_case()
    got, ref, slices, inp = run("radial polarisation", case, field, polarised=True)
    assert got.u[2] == 0.0 and got.v[2] == 0.0
    assert float(ref.stokes[0, 0, 2, 2]) < 1e-7 and ref.bound[0, 0, 2, 2] < 1e-9
    assert got.stokes[0, 0, 2, 2] <= float(ref.stokes[0, 0, 2, 2]) + ref.bound[0, 0, 2, 2] and got.strehl[0] < 1e-7
    device = device_frame(case.frame)
    assert device.psf(R.SURFACE, weights="intensity", **case.options).image[0, 2, 2] > 0.999


def test_rays_without_a_finite_field_are_left_out_and_counted():
    """5 rays of 300 with a NaN or an infinity in one state's field (real or imaginary part) are left out of both states
    and counted; the only test with rays left out."""
    case = R.psf_case([[300]], pixels=(9, 7), pixel_size=0.4 * R.LAMBDA_F, opd_waves=0.1, filler=500, seed=8)
    rows = V.selected_rows(case.frame, R.SURFACE, case.options["rays_per_source"], 1)
    field = V.random_field(case.n_rows, True, 41)
    for plane, row, value in ((0, 3, np.nan), (2, 77, np.nan * 1j), (4, 150, np.inf), (5, 151, -np.inf * 1j), (1, 299, np.nan)):
        field[plane, rows[row]] = value
    got, ref, slices, _ = run("non-finite fields", case, field, polarised=False, missed=5)
    assert got.n_missed.tolist() == [5] and got.n_rays.tolist() == [295]


def test_two_runs_agree_bit_for_bit_and_the_scalar_psf_is_untouched():
    case = R.psf_bucket_case()
    device = device_frame(case.frame)
    fresnel = fresnel_of(device, V.random_field(case.n_rows, True, 17), polarised=False)
    first = device.psf(R.SURFACE, weights="intensity", fresnel=fresnel, **case.options)
    scalar = device.psf(R.SURFACE, weights="intensity", **case.options)
    second = device.psf(R.SURFACE, weights="intensity", fresnel=fresnel, **case.options)
    for name in ("stokes_by_wavelength", "axial_by_wavelength", "image", "strehl", "strehl_apodized", "throughput",
                 "denominator", "record", "u", "v", "peak"):
        assert np.array_equal(getattr(first, name), getattr(second, name), equal_nan=True), name
    again = device.psf(R.SURFACE, weights="intensity", **case.options)
    for name in ("image_by_wavelength", "strehl", "record", "u", "v", "peak", "f_number"):
        assert np.array_equal(getattr(scalar, name), getattr(again, name), equal_nan=True), name
    assert type(scalar).__name__ == "PSF" and type(first).__name__ == "VectorPSF"
    # the two sums share their denominator: the scalar record's sum of amplitudes is the vector record's
    assert np.array_equal(first.record[:, :, 0, 2], scalar.record[:, :, 2])


def test_trace_psf_with_a_coated_singlet_end_to_end():
    """The singlet tests/test_gpu_psf.py traces (a 6 degree cone through the config-2 lens onto a detector), 2000 rays,
    16 x 16 pixels, circular input, a quarter-wave layer on both faces: the result against the reference fed with the device's own
    Fresnel.field, Wavefront.opd / pupil and the frame's columns, and the throughput against Fresnel.transmission."""
    import pyrayt_amd as pyrayt
    import scenes
    from pyrayt_amd.materials import Coating

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=2000)
    got = tracer.trace_psf(det, world_unit_um=1000, pixels=16,
                           fresnel=dict(polarization=(0, 1, 1j), coatings={lens: Coating.quarter_wave(1.38, 0.55)}))
    F = got.fresnel
    assert type(got).__name__ == "VectorPSF" and F.field.is_complex() and F.n_coated == 4000 and F.n_invalid == 0
    frame = F.frame.rows.cpu().numpy().T
    inp = R.psf_inputs_from(frame, got, float(det.get_id()))
    rows = V.selected_rows(frame, float(det.get_id()), None, 1)
    field = F.field.cpu().numpy()
    slices = V.vpsf_slices(len(frame), 1, 1, 256, compute_units())
    axes = got.wavefront._made_of["axes"]
    ref = V.vector_psf_reference(inp, V.field_of_rows(field, rows), 1, axes=axes, slices=slices)
    assert got.n_rays.tolist() == [2000] and got.n_missed.tolist() == [0] and not ref.n_missed.any()
    family = "coated singlet"
    hold(family, "stokes", np.concatenate([got.stokes, got.axial[:, None]], axis=1), ref.stokes, ref.bound)
    hold(family, "image", got.image, ref.image, ref.image_bound)
    hold(family, "strehl", got.strehl, ref.strehl, ref.strehl_bound)
    hold(family, "strehl_apodized", got.strehl_apodized, ref.strehl_apodized, ref.strehl_apodized_bound)
    hold(family, "throughput", got.throughput, ref.throughput, ref.throughput_bound)
    through = F.transmission(det)
    print(f"[vector psf] {family}: throughput {got.throughput[0]:.15f}, transmission {through[0]:.15f}, "
          f"strehl {got.strehl[0]:.6f}, strehl_apodized {got.strehl_apodized[0]:.6f}")
    assert abs(got.throughput[0] - through[0]) <= 1e-12 and 0.95 < through[0] < 1.0
    assert got.strehl[0] <= got.strehl_apodized[0] * (1 + 1e-12)  # (|E| <= 1: the aligned wave is no brighter than D_g)
    assert np.abs(got.stokes[0, 3]).max() > 0.9 * got.stokes[0, 0].max()  # (circular input stays circular)


def test_unpolarised_input_of_a_trace_is_summed_in_states_uniform_across_the_beam():
    """fresnel(polarization=None) launches each ray in a basis made from its own direction, which jumps across a cone:
    summed as they are, the two states of an uncoated singlet lose half the image.  psf() turns them into the states
    'y across the ray' and 'u0 x that' first: the first is the field fresnel(polarization=(0, 1, 0)) carries, the strict
    Strehl ratio is back at 1 and the image is unpolarised."""
    import pyrayt_amd as pyrayt
    import scenes
    from pyrayt_amd.frame import Fresnel

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    frame = pyrayt.RayTracer(src, [lens, det], rays_per_source=2000).trace_device()
    made = frame.fresnel(fields=True)
    assert made.launch_states == "per_ray" and frame.fresnel(polarization=(0, 1, 0)).launch_states == "polarised"
    along_y = frame.fresnel(polarization=(0, 1, 0), fields=True)
    uniform = made.uniform_states((0, 1, 0))
    assert float((uniform.field[:3] - along_y.field[:3]).abs().max()) < 1e-12
    assert float(((uniform.field.abs() ** 2).sum(dim=0) - (made.field.abs() ** 2).sum(dim=0)).abs().max()) < 1e-12
    got = frame.psf(det, world_unit_um=1000, pixels=16, fresnel=made)
    assert got.fresnel.launch_states == "uniform" and got.n_states == 2 and got.n_missed.tolist() == [0]
    as_they_are = Fresnel(frame, made.transmittance, made.field, np.zeros(6, dtype=np.int64))
    raw = frame.psf(det, world_unit_um=1000, pixels=16, fresnel=as_they_are)
    print(f"[vector psf] unpolarised singlet: strehl_apodized {got.strehl_apodized[0]:.6f} in uniform states, "
          f"{raw.strehl_apodized[0]:.6f} in the per-ray states; throughput {got.throughput[0]:.6f}")
    assert got.strehl_apodized[0] > 0.999 and raw.strehl_apodized[0] < 0.6
    assert abs(got.throughput[0] - made.transmission(det)[0]) <= 1e-12 and got.throughput[0] == pytest.approx(raw.throughput[0], abs=1e-12)
    i, j = np.unravel_index(int(np.argmax(got.image[0])), got.image[0].shape)
    assert got.degree_of_polarization()[0, i, j] < 0.02
