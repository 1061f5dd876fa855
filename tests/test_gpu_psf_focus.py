"""The diffraction PSF and the Strehl ratio through focus (DeviceFrame.psf(focus=), k_psff_huygens, k_psff_strehl) against
the longdouble reference of tests/psf_focus_reference.py, every pixel of every plane and every Strehl ratio held to the
budget derived there; the three contracts on bits (the plane 0.0 is psf(); a plane alone, among 41, reversed and listed
twice; run to run); planes past the slab cap; the chief line; closed forms; p3; and a traced lens end to end.  Each
test prints its largest deviation / bound."""
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import psf_focus_reference as F
from helpers import assert_same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
K = R.K
RATIOS = []  # deviation / bound of every hold() of this module: the largest is what profiles/psf_focus/README.md records


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


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
    with np.errstate(invalid="ignore"):
        ratio = np.where(nan, 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[focus bounds] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, "
          f"{got.size} values)")
    RATIOS.append(float(ratio.ravel()[k]))
    print(f"[focus bounds] largest deviation / bound so far, over {len(RATIOS)} holds: {max(RATIOS):.3f}")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


def held(family, frame, got, options, n_rows, weights="intensity"):
    """A PSFScan against the reference on the device's own wavefront, p3, line and centres."""
    G = options.get("n_groups", 1)
    inp = R.psf_inputs_from(frame, got, options["surface"], options.get("rays_per_source"), G, weights)
    axial = got.axial.cpu().numpy()
    assert len(axial) == len(inp.opd)
    slices = R.psf_slices(n_rows, G * len(got.wavelengths), len(got.u) * len(got.v), compute_units())
    ref = F.psf_focus_reference(inp, axial, got.focus, got.centres, got.line, slices=slices)
    assert np.array_equal(got.record[:, :, 0], ref.n_rays) and np.array_equal(got.record[:, :, 1], ref.n_missed)
    hold(family, "image_by_wavelength", got.image_by_wavelength, ref.image_by_wavelength, ref.bound_by_wavelength)
    hold(family, "image", got.image, ref.image, ref.bound)
    hold(family, "strehl", got.strehl, ref.strehl, ref.strehl_bound)
    # the centres are fma(delta, t, centre) of the device's own line, to the bit
    assert_same_bits(got.centres, F.centres_of(got.line, got.focus, got.centre), f"{family}: centres")
    return ref, inp, axial, slices


def run_scan(family, case, focus=F.SHIFTS, track="chief"):
    device = device_frame(case.frame)
    got = device.psf(R.SURFACE, weights="intensity", focus=focus, track=track, **case.options)
    ref, inp, axial, slices = held(family, case.frame, got, dict(case.options, surface=R.SURFACE), case.n_rows)
    assert np.array_equal(ref.n_rays, case.counts) and not ref.n_missed.any()
    design = case.inputs(got.u, got.v)
    np.testing.assert_allclose(axial, F.sphere_axial(design), rtol=1e-9)
    return SimpleNamespace(got=got, ref=ref, inp=inp, axial=axial, slices=slices, device=device)


# ---- the bound --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filler", (0, R.PSF_FILLER), ids=("alone", "among_other_rows"))
@pytest.mark.parametrize("n", R.SIZES)
def test_focus_ray_slices_and_the_lds_tile(n, filler):
    """R's ray-slice family at three planes (-1, 0 and +0.64 depths of focus): rays of a bucket about the LDS tile and the
    slice, alone and among rows of another surface that raise the slices over the same rays."""
    run = run_scan("focus ray slices", R.psf_slice_case(n, filler))
    assert run.slices == max(1, (n + filler) // K.kPsfMinSlice) and run.got.image.shape == (1, 3, 9, 7)
    assert run.got.strehl.shape == (1, 3) and np.all(run.got.axial.cpu().numpy() < 0)


@pytest.mark.parametrize("grid", ((32, 32), (31, 33), (64, 65), (2, 513)), ids=lambda g: f"{g[0]}x{g[1]}")
def test_focus_pixel_tiles(grid):
    """A whole tile, one pixel short of it, five tiles of which the last is partial, and 1026 pixels in two rows, on
    three planes: blockIdx.z carries (bucket, plane), and every plane's tile edges are the grid's."""
    run = run_scan("focus pixel tiles", R.psf_tile_case(grid))
    assert run.slices == 1 and run.got.image.shape == (1, 3) + grid


def test_focus_buckets_of_1_300_4000_and_0_rays():
    run = run_scan("focus uneven buckets", R.psf_bucket_case())
    got = run.got
    assert run.slices == 2 and got.image_by_wavelength.shape == (2, 3, 3, 9, 7)
    assert np.all(np.isnan(got.image[1])) and np.all(np.isnan(got.strehl[1])) and np.all(np.isfinite(got.image[0]))
    assert np.all(np.isnan(got.line[1])) and np.all(np.isnan(got.centres[1])) and np.all(np.isnan(got.best_focus()[1:]))
    table = got.to_pandas()
    assert len(table) == 6 and list(table.columns) == ["source_id", "focus", "strehl", "peak"]


@pytest.mark.parametrize("micrometres", (False, True), ids=("R2000mm", "R2e6um"))
def test_focus_large_phases(micrometres):
    """R / lambda_w = 5e6 cycles, pixels out to 0.3 R and shifts of both signs of 0.05 R and 0.03 R: inside the budget's
    domain (cross < 0.5 k0, asserted by the reference), where ulp(5e6) cycles is a visible part of it."""
    case = R.psf_large_phase_case(micrometres)
    radius = case.options["radius"]
    run_scan("focus large phases", case, focus=(-0.05 * radius, 0.0, 0.03 * radius))


# ---- the bits ---------------------------------------------------------------------------------------------------------------
def same_scan(a, b, what):
    for name in ("image_by_wavelength", "strehl", "record", "line", "centres"):
        assert_same_bits(getattr(a, name), getattr(b, name), f"{what}: {name}")
    assert_same_bits(a.axial.cpu().numpy(), b.axial.cpu().numpy(), f"{what}: axial")


@pytest.mark.parametrize("name", ("ray slices", "buckets", "64x65"))
def test_the_plane_zero_has_the_bits_of_psf(name):
    """Contract 1: image, Strehl ratio and record of the plane delta = 0.0, among others, are psf()'s."""
    case = {"ray slices": lambda: R.psf_slice_case(2049, R.PSF_FILLER), "buckets": R.psf_bucket_case,
            "64x65": lambda: R.psf_tile_case((64, 65))}[name]()
    device = device_frame(case.frame)
    plain = device.psf(R.SURFACE, weights="intensity", **case.options)
    for track in ("chief", None):
        scan = device.psf(R.SURFACE, weights="intensity", focus=F.SHIFTS, track=track, **case.options)
        assert scan.focus[1] == 0.0
        assert_same_bits(scan.image_by_wavelength[:, 1], plain.image_by_wavelength, f"{name}: image")
        assert_same_bits(scan.strehl[:, 1], plain.strehl, f"{name}: strehl")
        assert_same_bits(scan.record, plain.record, f"{name}: record")
        assert_same_bits(scan.u + scan.centres[0, 1, 0], plain.u, f"{name}: u")
        one = scan.plane(0.0)
        assert_same_bits(one.image, plain.image, f"{name}: plane(0.0).image")
        assert np.array_equal(one.peak, plain.peak, equal_nan=True)
    assert np.any(scan.image[:, 0] != scan.image[:, 1])


def test_a_plane_has_the_same_bits_alone_among_41_reversed_and_twice():
    """Contracts 2 and 3 on np.linspace(-0.2, 0.2, 41), whose entry 20 is 0.0."""
    case = R.psf_slice_case(2049, R.PSF_FILLER)
    device = device_frame(case.frame)
    focus = np.linspace(-0.2, 0.2, 41)
    assert focus[20] == 0.0
    scan = lambda shifts: device.psf(R.SURFACE, weights="intensity", focus=shifts, **case.options)  # noqa: E731
    among = scan(focus)
    same_scan(among, scan(focus), "run to run")
    backwards = scan(focus[::-1])
    assert_same_bits(backwards.image_by_wavelength[:, ::-1], among.image_by_wavelength, "reversed: image")
    assert_same_bits(backwards.strehl[:, ::-1], among.strehl, "reversed: strehl")
    assert_same_bits(backwards.centres[:, ::-1], among.centres, "reversed: centres")
    for k in (0, 20, 40):
        alone = scan([focus[k]])
        twice = scan([focus[k], focus[5], focus[k]])
        for other, at in ((alone, 0), (twice, 0), (twice, 2)):
            assert_same_bits(other.image_by_wavelength[:, at], among.image_by_wavelength[:, k], f"plane {k}: image")
            assert_same_bits(other.strehl[:, at], among.strehl[:, k], f"plane {k}: strehl")
            assert_same_bits(other.centres[:, at], among.centres[:, k], f"plane {k}: centres")
        assert_same_bits(alone.record, among.record, f"plane {k}: record")
    plain = device.psf(R.SURFACE, weights="intensity", **case.options)
    assert_same_bits(among.image_by_wavelength[:, 20], plain.image_by_wavelength, "plane 20 is psf()")


def test_planes_past_the_slab_cap_run_in_chunks():
    """1024 x 1024 pixels of 16 bytes are 16 MiB a plane and slice: 16 planes fill the 256 MiB slab, so 17 planes need
    two launches.  The last plane of the first, the first of the second and the plane 0.0 are what they are alone."""
    npix = 1024 * 1024
    per_chunk = K.kPsfSlabBytes // (npix * 16)
    assert per_chunk == 16 and R.psf_slices(5, 1, npix, compute_units()) == 1
    case = R.psf_case([[5]], pixels=(1024, 1024), pixel_size=0.02 * R.LAMBDA_F, opd_waves=0.1, seed=3)
    device = device_frame(case.frame)
    focus = (np.arange(per_chunk + 1) - 3) * 0.01
    assert focus[3] == 0.0
    among = device.psf(R.SURFACE, weights="intensity", focus=focus, **case.options)
    assert among.image.shape == (1, 17, 1024, 1024) and np.all(np.isfinite(among.image))
    for k in (per_chunk - 1, per_chunk, 3):
        alone = device.psf(R.SURFACE, weights="intensity", focus=[focus[k]], **case.options)
        assert_same_bits(alone.image_by_wavelength[:, 0], among.image_by_wavelength[:, k], f"plane {k}")
        assert_same_bits(alone.strehl[:, 0], among.strehl[:, k], f"plane {k}: strehl")
    assert np.any(among.image[0, per_chunk] != among.image[0, per_chunk - 1])


# ---- the chief line ---------------------------------------------------------------------------------------------------------
def test_the_chief_line_of_displaced_pupils():
    case = F.offaxis_case()
    run = run_scan("focus chief line", case)
    got = run.got
    buckets = len(got.wavelengths)
    want, bound = F.chief_line(run.inp, run.axial, depth=F.line_depth(600, run.slices, buckets))
    hold("focus chief line", "line", got.line, want, bound)
    assert np.all(bound < 1e-13) and np.all(np.abs(got.line) > 0.004) and np.sign(got.line[0, 0]) != np.sign(got.line[1, 0])
    assert np.any(got.centres[0] != got.centres[1])
    with pytest.raises(ValueError, match="group="):
        got.plane(F.SHIFTS[0])
    assert got.plane(F.SHIFTS[0], group=1).centre == tuple(got.centres[1, 0])
    axis = run_scan("focus chief line (track=None)", case, track=None).got
    assert not axis.line.any() and np.all(axis.centres == np.asarray(case.options["centre"]))


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def test_a_converging_wave_on_the_device():
    """A perfect wave that converges at P + 0.2 a: Strehl 1 there within the bound, below 1 at P (0.495, issue's figure),
    and in that plane the Airy pattern's dark rings where the in-focus pattern has them, scaled by (R + delta0) / R."""
    n, step = 4096, 3.6 * R.LAMBDA_F / 256
    case = F.converging_case(n, pixels=(513, 1), pixel_size=step)
    run = run_scan("focus converging wave", case, focus=(F.DELTA0, 0.0), track=None)
    got, ref = run.got, run.ref
    assert abs(got.strehl[0, 0] - 1.0) <= ref.strehl_bound[0, 0] + 8 * n * float(np.finfo(LD).eps)
    assert abs(got.strehl[0, 1] - 0.495) < 0.002 and got.best_focus()[0] == F.DELTA0
    profile = got.image[0, 0, 256:, 0]
    assert profile[0] == pytest.approx(got.strehl[0, 0], abs=1e-6)
    minima = [k for k in range(1, 256) if profile[k] < profile[k - 1] and profile[k] < profile[k + 1]]
    assert len(minima) >= 3 and max(profile[minima[:3]]) < 1e-4
    for k, zero in zip(minima[:3], (1.22, 2.23, 3.24)):
        assert abs(k * step / (zero * R.LAMBDA_F * (10.0 + F.DELTA0) / 10.0) - 1) < 0.02, (k, zero)


# ---- p3 ---------------------------------------------------------------------------------------------------------------------
def test_axial_is_the_sphere_points_third_component():
    """axial^2 + |pupil rho|^2 = R^2 to 64 u R^2: the row's reach s to the sphere is within about ten roundings, E = Q - s u
    two more on each component, twelve u R on |E - P| and so 24 u R^2 on its square, the three dot products and the
    pupil's scaling a few each.  Its sign is -sign(u.a); it is NaN exactly where the pupil point is, and the rows
    left out are psf()'s."""
    case = R.psf_slice_case(300, 100)
    frame = case.frame.copy()
    at = np.flatnonzero(frame[:, 5] == R.SURFACE)
    frame[at[3], 9:12], frame[at[3], 12:15] = (0.0, 50.0, 0.0), (1.0, 0.0, 0.0)  # (a line that misses the sphere)
    frame[at[7], 10] = np.nan                                                      # (an end point that is no number)
    frame[at[11], 1] = -1.0                                                        # (a weight psf() leaves out)
    device = device_frame(frame)
    for axis, sign in ((None, -1.0), ((-1.0, 0.0, 0.0), 1.0)):
        options = dict(case.options, **({} if axis is None else {"axis": axis}))
        scan = device.psf(R.SURFACE, weights="intensity", focus=(0.0, 0.05), **options)
        plain = device.psf(R.SURFACE, weights="intensity", **options)
        axial, pupil = scan.axial.cpu().numpy(), scan.wavefront.pupil.cpu().numpy()
        assert len(axial) == 300 and np.array_equal(np.isnan(axial), np.isnan(pupil[:, 0])) and np.isnan(axial).sum() == 2
        ok = ~np.isnan(axial)
        assert np.all(np.sign(axial[ok]) == sign)
        p = pupil[ok] * scan.wavefront.pupil_radius[0]
        residual = (axial[ok].astype(LD) ** 2 + p[:, 0].astype(LD) ** 2 + p[:, 1].astype(LD) ** 2) - LD(10.0) ** 2
        print(f"[focus bounds] axial: largest |axial^2 + p^2 - R^2| {float(np.abs(residual).max()) / (R.U64 * 100.0):.2f} u R^2")
        assert float(np.abs(residual).max()) <= 64 * R.U64 * 100.0
        assert_same_bits(scan.record, plain.record, "record")
        assert scan.n_missed[0] == 3 and scan.n_rays[0] == 297
        assert_same_bits(scan.image_by_wavelength[:, 0], plain.image_by_wavelength, "image of the plane 0.0")


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_trace_psf_through_focus_of_a_lens():
    """A collimated beam of 10 240 rays on 16 rings of equal area through a biconvex singlet with spherical aberration:
    trace_psf(focus=) against the reference on the device's own wavefront, and a diffraction focus away from the
    detector."""
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    rings = [pyrayt.components.CircleOfRays(diameter=0.7 * np.sqrt((k + 0.5) / 16)).move_x(-1) for k in range(16)]
    det = pyrayt.components.baffle((1, 1)).move_x(2.0)
    tracer = pyrayt.RayTracer(rings, [lens, det], rays_per_source=640)
    plain = tracer.trace_psf(det, world_unit_um=1000.0, pixels=9)
    depth = 2 * plain.wavelengths[0] * 1e-3 * plain.f_number[0] ** 2
    focus = depth * np.arange(5.0)
    got = tracer.trace_psf(det, world_unit_um=1000.0, pixels=9, focus=focus)
    assert got.image.shape == (1, 5, 9, 9) and got.n_rays[0] > 10_000
    assert_same_bits(got.image_by_wavelength[:, 0], plain.image_by_wavelength, "the plane 0.0 is trace_psf()'s")
    assert_same_bits(got.strehl[:, 0], plain.strehl, "the plane 0.0 has trace_psf()'s Strehl ratio")
    frame = tracer.trace_device().to_numpy()
    held("focus traced lens", frame, got, dict(surface=float(det.get_id())), len(frame))
    best = got.best_focus()[0]
    nearest = int(np.argmin(np.abs(got.focus - best)))
    assert got.strehl[0, nearest] >= got.strehl[0, 0] and focus[0] < best < focus[-1]
    assert got.strehl[0, nearest] > 0.5 > got.strehl[0, 0]  # (the detector is not where the wave converges best)
    with pytest.raises(ValueError, match="fresnel"):
        tracer.trace_psf(det, world_unit_um=1000.0, focus=focus, fresnel={})
