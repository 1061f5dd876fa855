"""Diffraction PSF and Strehl ratio of the result frame on the device (DeviceFrame.psf, RayTracer.trace_psf): against
a numpy restatement of the definitions (include/prt.h) on a synthetic frame and on one of the reference's frames,
against the closed forms of an Airy disk, a ring pupil's J0^2 pattern and a defocused Strehl ratio, and run twice
for bit-identical outputs."""
import math

import numpy as np
import pytest

import diffraction_reference
import helpers
import scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}
LAMBDA = 0.633  # micrometres


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


# ---- the numpy restatement ----------------------------------------------------------------------------------------------
def psf_reference(frame, surface, psf, unit, rays_per_source=None, n_groups=1, weights="intensity"):
    """image (n_groups, n_wavelengths, nx, ny) and Strehl per group from the definitions, built from the Wavefront's
    opd / pupil and the frame's own columns (the wavefront's rows: at ``surface``, in a group, in row order)."""
    wave = psf.wavefront
    rows = frame[frame[:, IX["surface"]] == surface]
    groups = np.floor(rows[:, IX["id"]] / rays_per_source) if rays_per_source else np.zeros(len(rows))
    keep = (groups >= 0) & (groups < n_groups)
    rows, groups = rows[keep], groups[keep].astype(int)
    opd, pupil = wave.opd.cpu().numpy(), wave.pupil.cpu().numpy()
    assert len(opd) == len(rows)
    w = np.ones(len(rows)) if weights is None else rows[:, IX[weights]]
    u, v = psf.u, psf.v
    image = np.full((n_groups, len(psf.wavelengths), len(u), len(v)), np.nan)
    strehl = np.full(n_groups, np.nan)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    uu, vv = uu.ravel(), vv.ravel()
    for g in range(n_groups):
        ok = (groups == g) & np.isfinite(opd)
        if not ok.any():
            continue
        radius, rho = wave.radius[g], wave.pupil_radius[g]
        amplitudes, numerator, denominator = [], 0.0, 0.0
        for k, lam in enumerate(psf.wavelengths):
            m = ok & (rows[:, IX["wavelength"]] == lam)
            lw = lam / unit
            a, o = np.sqrt(w[m]), opd[m]
            p1, p2 = pupil[m, 0] * rho, pupil[m, 1] * rho
            total = np.zeros(len(uu), dtype=complex)
            for at in range(0, len(uu), 128):
                su, sv = uu[at:at + 128, None], vv[at:at + 128, None]
                d = np.sqrt(radius ** 2 + su ** 2 + sv ** 2 - 2 * (su * p1 + sv * p2))
                total[at:at + 128] = (a * np.exp(2j * np.pi * (o + d - radius) / lw)).sum(axis=1)
            amplitudes.append(np.abs(total / lw) ** 2)
            numerator += abs((a * np.exp(2j * np.pi * o / lw)).sum()) ** 2 / lw ** 2
            denominator += (a.sum() / lw) ** 2
        image[g] = np.array(amplitudes).reshape(len(psf.wavelengths), len(u), len(v)) / denominator
        strehl[g] = numerator / denominator
    return image, strehl


def check_psf(frame, device, surface, unit, **options):
    got = device.psf(surface, world_unit_um=unit, **options)
    image, strehl = psf_reference(frame, surface, got, unit, options.get("rays_per_source"), options.get("n_groups", 1),
                                  options.get("weights", "intensity"))
    assert got.image_by_wavelength.shape == image.shape
    np.testing.assert_allclose(got.image_by_wavelength, image, rtol=0, atol=1e-5, equal_nan=True)
    np.testing.assert_allclose(got.image, image.sum(axis=1), rtol=0, atol=2e-5, equal_nan=True)
    np.testing.assert_allclose(got.strehl, strehl, rtol=0, atol=1e-9, equal_nan=True)
    # ... and every pixel against the longdouble reference, within the derived budget (tests/diffraction_reference.py),
    # which on these frames is tighter than the flat figures above (tests/test_host_diffraction_reference.py)
    n_groups = options.get("n_groups", 1)
    inputs = diffraction_reference.psf_inputs_from(frame, got, surface, options.get("rays_per_source"), n_groups,
                                                   options.get("weights", "intensity"))
    ref = diffraction_reference.psf_reference(inputs)
    for value, want, bound in ((got.image_by_wavelength, ref.image_by_wavelength, ref.bound_by_wavelength),
                               (got.image, ref.image, ref.bound), (got.strehl, ref.strehl, ref.strehl_bound)):
        nan = np.isnan(want.astype(float))
        assert np.array_equal(np.isnan(value), nan)
        assert np.all(np.abs(value.astype(np.longdouble) - want)[~nan] <= bound[~nan])
    assert np.nanmax(ref.bound_by_wavelength) < 1e-5 and np.nanmax(ref.bound) < 2e-5 and np.nanmax(ref.strehl_bound) < 1e-9
    assert np.array_equal(got.record[:, :, 0], ref.n_rays) and np.array_equal(got.record[:, :, 1], ref.n_missed)
    return got


synthetic_frame = helpers.psf_synthetic_frame


def test_psf_against_numpy_on_a_synthetic_frame():
    frame = synthetic_frame()
    device = device_frame(frame)
    lam_f = 0.55e-3 * 5.0
    got = check_psf(frame, device, 5.0, 1000.0, pixels=(33, 31), pixel_size=(0.4 * lam_f, 0.35 * lam_f),
                    centre=(1.3 * lam_f, -0.7 * lam_f), rays_per_source=6000, n_groups=2)
    assert list(got.wavelengths) == [0.55, 0.65] and got.image.shape == (2, 33, 31)
    assert np.all(got.n_rays > 1000) and np.all(got.n_missed == 0)
    assert 0.0 < got.strehl.min() and got.strehl.max() < 1.0
    check_psf(frame, device, 5.0, 1000.0, pixels=(33, 31), pixel_size=0.5 * lam_f, weights=None)
    # the default pixel size: lambda_min F / 4
    auto = device.psf(5.0, world_unit_um=1000.0, pixels=8)
    assert auto.pixel_size[0] == pytest.approx(0.55e-3 * np.nanmin(auto.f_number) / 4, rel=1e-12)


def test_psf_against_numpy_on_a_reference_frame():
    frame = helpers.load("scene_config2.npz")["frame"]
    device = device_frame(frame)
    last = frame[:, 0].max()
    imager = float(frame[frame[:, 0] == last][-1, IX["surface"]])
    n_groups = int(frame[:, IX["id"]].max() // 512) + 1
    got = check_psf(frame, device, imager, 1000.0, pixels=(33, 31), centre=(2e-3, -1e-3), rays_per_source=512,
                    n_groups=n_groups)
    assert got.n_rays.sum() > 500


def test_a_row_of_a_wavelength_not_in_the_list_is_refused():
    from pyrayt_amd import engine

    frame = synthetic_frame()
    device = device_frame(frame)
    wave, rows, surface, n_groups, record = device._wavefront(5.0, "centroid", None, None, None, None, 15, None, None,
                                                              None, None)
    lam, centre = np.array([0.55]), np.zeros(2)
    image = torch.empty(64, dtype=torch.float64, device="cuda:0")
    strehl = torch.empty(1, dtype=torch.float64, device="cuda:0")
    out = torch.empty(4, dtype=torch.float64, device="cuda:0")
    lib = engine.library()
    work = torch.empty(lib.prt_frame_psf_workspace_bytes(rows.shape[1], 1, 1), dtype=torch.uint8, device="cuda:0")
    rc = lib.prt_frame_psf(0, rows.data_ptr(), rows.stride(0), rows.shape[1], surface, float("nan"), 0.0, 1,
                           wave.opd.data_ptr(), wave.pupil.data_ptr(), record.data_ptr(), -1, lam.ctypes.data, 1, 1000.0,
                           8, 8, 1e-3, 1e-3, centre.ctypes.data, image.data_ptr(), strehl.data_ptr(), out.data_ptr(),
                           work.data_ptr(), None)
    assert rc == -1 and "not in the list" in lib.prt_last_error().decode()


# ---- physics ------------------------------------------------------------------------------------------------------------
def disk_rays(n, radius, x, seed=13):
    """Rays along -x filling a disk, mirror-symmetric under y -> -y (pairs), the rim sampled evenly."""
    rng = np.random.default_rng(seed)
    half = n // 2
    r, t = np.sqrt(rng.random(half)) * radius, (rng.random(half) - 0.5) * np.pi  # (the half y >= 0, then mirrored)
    r[:128], t[:128] = radius, ((np.arange(128) + 0.5) / 128 - 0.5) * np.pi
    y, z = np.concatenate([r * np.cos(t), -r * np.cos(t)]), np.concatenate([r * np.sin(t), r * np.sin(t)])
    return along_minus_x(y, z, x)


def ring_rays(n, radius, x):
    t = (np.arange(n) + 0.5) / n * 2 * np.pi
    return along_minus_x(radius * np.cos(t), radius * np.sin(t), x)


def along_minus_x(y, z, x):
    rays = scenes.blank_rays(len(y), LAMBDA)
    rays[0], rays[1], rays[2] = x, y, z
    rays[4:7] = np.array([-1.0, 0.0, 0.0])[:, None]
    return rays


def parabola_frame(rays):
    """An on-axis parabolic mirror of focal length 9 mm and diameter 1 mm, focus at the origin; a detector 2 mm past
    the focus."""
    import pyrayt_amd as pyrayt
    from pyrayt_amd import engine
    from pyrayt_amd.frame import DeviceFrame
    from pyrayt_amd.scene import SceneSnapshot

    mirror = pyrayt.components.parabolic_mirror(9.0, 1, aperture=1)
    det = pyrayt.components.baffle((20, 20)).move_x(2)
    rows, counts = engine.DeviceScene(SceneSnapshot([mirror, det])).trace(torch.from_numpy(rays).to("cuda:0"), 10)
    return DeviceFrame(rows, counts), det


def radial_profile(psf):
    r = np.hypot(psf.u[:, None], psf.v[None, :]).ravel()
    step = psf.pixel_size[0]
    bins = np.rint(r / step).astype(int)
    total = np.bincount(bins, psf.image[0].ravel())
    count = np.bincount(bins)
    return np.arange(len(total)) * step, total / np.maximum(count, 1)


def first_minimum(x, y):
    k = next(i for i in range(1, len(y) - 1) if y[i] <= y[i - 1] and y[i] < y[i + 1])
    a, b, c = y[k - 1], y[k], y[k + 1]
    return x[k] + 0.5 * (a - c) / (a - 2 * b + c) * (x[1] - x[0])


def test_airy_disk_of_a_parabola_at_f10():
    frame, det = parabola_frame(disk_rays(200_000, 0.45, 1.0))  # (F = 9 / 0.9)
    focus = (0.0, 0.0, 0.0)
    wave = frame.wavefront(det, reference=focus)
    f_number = wave.radius[0] / (2 * wave.pupil_radius[0])  # (R / (2 rho_max))
    assert 9.5 < f_number < 10.5
    lam_f = LAMBDA * 1e-3 * f_number
    psf = frame.psf(det, world_unit_um=1000.0, pixels=257, pixel_size=lam_f / 8, reference=focus)  # (odd: P a centre)
    assert psf.n_rays[0] == 200_000 and psf.n_missed[0] == 0
    assert psf.f_number[0] == f_number
    assert psf.strehl[0] >= 0.999
    assert psf.peak[0] == pytest.approx(psf.strehl[0], rel=1e-3)
    airy = 1.22 * LAMBDA * 1e-3 * psf.f_number[0]
    assert abs(psf.encircled_energy(airy)[0] - 0.838) <= 0.02
    assert np.abs(psf.image[0] - psf.image[0][::-1, :]).max() <= 1e-6
    fine = frame.psf(det, world_unit_um=1000.0, pixels=128, pixel_size=lam_f / 32, reference=focus)
    radius, profile = radial_profile(fine)
    assert abs(first_minimum(radius, profile) / airy - 1) <= 0.03


def test_ring_pupil_gives_j0_squared():
    frame, det = parabola_frame(ring_rays(4096, 0.4, 1.0))
    wave = frame.wavefront(det, reference=(0.0, 0.0, 0.0))
    na = wave.pupil_radius[0] / wave.radius[0]
    step = LAMBDA * 1e-3 / na / 200
    psf = frame.psf(det, world_unit_um=1000.0, pixels=(401, 1), pixel_size=step, reference=(0.0, 0.0, 0.0))
    assert psf.n_rays[0] == 4096
    centre = 200
    zero = first_minimum(psf.u[centre:], psf.image[0, centre:, 0])
    assert abs(zero / (2.405 / (2 * np.pi) * LAMBDA * 1e-3 / na) - 1) <= 0.03
    assert psf.image[0, centre + int(round(zero / step)), 0] < 1e-3


def test_defocus_strehl_in_closed_form():
    rays = disk_rays(100_000, 0.45, 1.0)
    frame, det = parabola_frame(rays)
    lw = LAMBDA * 1e-3
    for delta in (0.12, 0.25):
        psf = frame.psf(det, world_unit_um=1000.0, pixels=16, reference=(delta, 0.0, 0.0))
        w20 = 2 * math.sqrt(3) * psf.wavefront.zernike[0, 3] / lw
        want = np.sinc(w20) ** 2  # (numpy's sinc: sin(pi x) / (pi x))
        assert abs(w20) > 0.2
        assert abs(psf.strehl[0] / want - 1) <= 0.01, (delta, psf.strehl[0], want, w20)
        # the Strehl ratio restated from the wavefront's OPD
        opd = psf.wavefront.opd.cpu().numpy()
        a = np.sqrt(np.full(len(opd), 100.0))
        restated = abs((a * np.exp(2j * np.pi * opd / lw)).sum()) ** 2 / a.sum() ** 2
        assert abs(psf.strehl[0] - restated) <= 1e-6


# ---- reproducibility, trace_psf, errors ---------------------------------------------------------------------------------
def config2_tracer(n):
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    return pyrayt.RayTracer(src, [lens, det], rays_per_source=n), lens, det


def same(a, b):
    for name in ("image_by_wavelength", "strehl", "record", "u", "v", "peak", "f_number"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


def test_reproducible_at_a_million_rays_and_trace_psf():
    tracer, lens, det = config2_tracer(1_000_000)
    frame = tracer.trace_device()
    first = frame.psf(det, world_unit_um=1000.0)
    same(first, frame.psf(det, world_unit_um=1000.0))
    traced = tracer.trace_psf(det, world_unit_um=1000.0)
    same(traced, tracer.trace_psf(det, world_unit_um=1000.0))
    same(traced, first)
    assert first.image.shape == (1, 128, 128) and first.n_rays[0] > 900_000 and np.isfinite(first.strehl[0])
    table = first.to_pandas()
    assert table.shape[0] == 1 and "strehl" in table
    # an active record_only() setting survives the call
    tracer.record_only(det, columns=("y1", "z1"))
    spot = tracer.trace().to_numpy(dtype=float)
    tracer.trace_psf(det, world_unit_um=1000.0, pixels=16, rays_per_source=True)
    assert tracer._record_surfaces == (det.get_id(),) and tracer._record_columns == ("y1", "z1")
    assert np.array_equal(tracer.trace().to_numpy(dtype=float), spot)


# ---- the stable sort under the pass (prt_sort.hpp) ----------------------------------------------------------------------
SORT_R = 105 / 8                    # the reference sphere's radius
SORT_P = (1.0, 0.0, 0.0)            # ... and its centre
SORT_RPS = 4096                     # ids a group


def sort_points():
    """Integer (y, z, root) with y^2 + z^2 + root^2 = 105^2: in units of 1/8 a ray along x through (y, z) meets the
    sphere of radius 105 / 8 about a point of the axis at a distance that fp64 holds exactly."""
    found = []
    for y in range(-60, 61):
        for z in range(-60, 61):
            root = math.isqrt(105 * 105 - y * y - z * z)
            if root * root == 105 * 105 - y * y - z * z and (y, z) != (0, 0):  # (a lone ray on the axis: no pupil radius)
                found.append((y, z, root))
    return np.array(found, dtype=float)


def sort_frame(n, filler):
    """One generation: 2 groups x 2 wavelengths, n rays a bucket at surface 5, row i in bucket i % 4, so that all four
    buckets occur inside every 64-row step; ray n // 2 of bucket (1, 0.55) misses the sphere (its OPD is NaN).  With
    ``filler`` a row of surface 2 follows every row.  Everything the wavefront adds up over these rows is exact: the rays
    run along x through the points of ``sort_points`` and end on multiples of 1/8, so OPL, the sphere's root and the OPD
    are multiples of 1/8 below 2^6, the weights are 1, 2 or 4, and sum w and sum w OPD (the piston that comes off the
    OPD) are the same bits however k_frame_zernike cuts the rows -- it cuts them by n_rows, which the filler doubles.
    The reference point and the radius are given, the slices are one in both frames (4 n and 8 n rows are below
    4 buckets x kPsfMinSlice): what is left to differ is the order of a bucket's rays."""
    points = sort_points()
    assert len(points) >= 40
    i = np.arange(4 * n)
    bucket, ray = i % 4, i // 4
    group, colour = bucket // 2, bucket % 2
    at = points[(7 * ray + 3 * bucket) % len(points)]
    frame = np.zeros((4 * n, 15))
    frame[:, IX["intensity"]] = 2.0 ** ((ray + bucket) % 3)
    frame[:, IX["wavelength"]] = np.where(colour == 0, 0.55, 0.65)
    frame[:, IX["index"]] = 1.0
    frame[:, IX["id"]] = group * SORT_RPS + 2 * ray + colour
    frame[:, IX["surface"]] = 5.0
    frame[:, IX["x0"]], frame[:, IX["y0"]], frame[:, IX["z0"]] = -4.0, at[:, 0] / 8, at[:, 1] / 8
    frame[:, IX["x1"]], frame[:, IX["y1"]], frame[:, IX["z1"]] = SORT_P[0] + (ray % 7) / 8, at[:, 0] / 8, at[:, 1] / 8
    frame[:, IX["x_tilt"]] = 1.0
    miss = 4 * (n // 2) + 2
    frame[miss, IX["y0"]] = frame[miss, IX["y1"]] = 2 * SORT_R
    if not filler:
        return frame
    other = frame.copy()
    other[:, IX["surface"]] = 2.0
    other[:, IX["id"]] = 2 * SORT_RPS + i
    return np.stack([frame, other], 1).reshape(8 * n, 15)


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_rows_of_another_surface_between_the_rays_change_no_bit(n):
    """The sort's own promise, on (group, wavelength) buckets that all occur inside every 64-row step -- at 300 rays a
    bucket the 1200 rows are two waves of the row passes (kWfRowsPerWave = 1024), three with the filler, so every
    bucket crosses a wave's edge: image, Strehl ratio and record of ``sort_frame`` alone and with a row of another
    surface after every row are the same uint64 bits, and the counts of rays kept and left out are numpy's."""
    runs = []
    for filler in (False, True):
        frame = sort_frame(n, filler)
        assert len(frame) == (8 if filler else 4) * n
        selected = frame[frame[:, IX["surface"]] == 5.0]
        for step in range(0, len(selected) - 63, 64):
            assert len(set(selected[step:step + 64, IX["id"]] // SORT_RPS * 2 + (selected[step:step + 64, IX["wavelength"]] == 0.65))) == 4
        got = device_frame(frame).psf(5.0, world_unit_um=1000.0, pixels=(9, 7), pixel_size=2e-3, centre=(1e-3, -2e-3),
                                      reference=SORT_P, radius=SORT_R, rays_per_source=SORT_RPS, n_groups=2)
        assert list(got.wavelengths) == [0.55, 0.65] and got.image_by_wavelength.shape == (2, 2, 9, 7)
        # the wavefront's own sums are exact, as sort_frame says: OPDs on a grid of 1/8 about the piston that came off
        opd = got.wavefront.opd.cpu().numpy()
        assert np.isnan(opd).sum() == 1 and len(opd) == 4 * n
        kept = np.full((2, 2), n)
        kept[1, 0] -= 1
        assert np.array_equal(got.record[:, :, 0], kept) and np.array_equal(got.record[:, :, 1], n - kept)
        assert np.array_equal(got.record[:, :, 0], [[np.sum((selected[:, IX["id"]] // SORT_RPS == g) & (selected[:, IX["wavelength"]] == lam)
                                                            & (np.abs(selected[:, IX["y1"]]) < SORT_R)) for lam in (0.55, 0.65)] for g in (0, 1)])
        runs.append(got)
    alone, among = runs
    for name in ("image_by_wavelength", "strehl", "record"):
        a, b = (np.ascontiguousarray(getattr(run, name), dtype=np.float64).view(np.uint64) for run in runs)
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    assert np.array_equal(alone.wavefront.opd.cpu().numpy().view(np.uint64), among.wavefront.opd.cpu().numpy().view(np.uint64))
    if n > 1:
        assert np.all(np.isfinite(alone.strehl)) and np.all(np.isfinite(alone.image_by_wavelength))


def test_errors_on_the_device():
    tracer, lens, det = config2_tracer(4096)
    frame = tracer.trace_device()
    with pytest.raises(ValueError, match="where"):
        frame.where(surface=det.get_id()).psf(det, world_unit_um=1000.0)
    with pytest.raises(ValueError, match="pixels"):
        frame.psf(det, world_unit_um=1000.0, pixels=2048)
    with pytest.raises(NotImplementedError):
        frame.psf(det, world_unit_um=1000.0, group=object())
    tracer.record_only(det)
    with pytest.raises(ValueError, match="record_only"):
        tracer.trace_device().psf(det, world_unit_um=1000.0)
