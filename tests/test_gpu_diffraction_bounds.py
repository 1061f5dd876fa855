"""The diffraction PSF (k_psf_huygens, k_psf_strehl) and the geometric OTF (k_mtf_sum) against the longdouble reference of
tests/diffraction_reference.py, every pixel and every output held to the error budget derived there: at the edges of
the pixel tiles, the ray slices and the LDS tile, at dark pixels, at phases of millions of cycles, and over the lanes
and output tiles of the OTF.  Each test names the edge it sits on and prints its largest deviation and ratio to bound."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
K = R.K


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


# The slice, lane and tile counts asserted below come from Python copies of the host rules (R.psf_slices, R.mtf_slices,
# R.mtf_lanes): the device's own counts cannot be read back.  tests/test_host_diffraction_reference.py holds the copies
# to the headers' text, so a changed rule fails there rather than moving these cases off their edges unnoticed.
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
    ratio = np.where(nan, 0.0, deviation / bound)
    k = int(np.nanargmax(ratio))
    print(f"[bounds] {family} {what}: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
          f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {bound.ravel()[k]:.3e}, "
          f"{got.size} values)")
    assert np.all(ratio <= 1.0), (family, what, float(ratio.ravel()[k]), float(deviation.ravel()[k]), float(bound.ravel()[k]))
    return float(ratio.ravel()[k])


# ---- the PSF ----------------------------------------------------------------------------------------------------------------
def run_psf(family, case):
    device = device_frame(case.frame)
    got = device.psf(R.SURFACE, weights="intensity", **case.options)
    G = case.options["n_groups"]
    inp = R.psf_inputs_from(case.frame, got, R.SURFACE, case.options["rays_per_source"], G)
    # the wavefront the frame was designed for is the one the device found (the CPU test's mutations run on the design)
    design = case.inputs(got.u, got.v)
    scale = float(np.nanmax(design.radius))
    assert np.array_equal(inp.group, design.group) and np.array_equal(inp.wavelength, design.wavelength)
    np.testing.assert_allclose(inp.opd, design.opd, rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(inp.pupil, design.pupil, rtol=0, atol=1e-9)
    nx, ny = len(got.u), len(got.v)
    slices = R.psf_slices(case.n_rows, G * len(got.wavelengths), nx * ny, compute_units())
    ref = R.psf_reference(inp, slices=slices)
    assert np.array_equal(got.record[:, :, 0], ref.n_rays) and np.array_equal(got.record[:, :, 1], ref.n_missed)
    assert np.array_equal(ref.n_rays, case.counts) and not ref.n_missed.any()
    hold(family, "image_by_wavelength", got.image_by_wavelength, ref.image_by_wavelength, ref.bound_by_wavelength)
    hold(family, "image", got.image, ref.image, ref.bound)
    hold(family, "strehl", got.strehl, ref.strehl, ref.strehl_bound)
    return got, ref, slices


@pytest.mark.parametrize("grid", R.PSF_GRIDS + R.PSF_GRIDS_WITHIN_THE_CAP, ids=lambda g: f"{g[0]}x{g[1]}")
def test_psf_pixel_tiles(grid):
    """The pixels of a workgroup, kPsfBlock * kPsfPix = 1024: one pixel, one short of a tile (1023), a whole tile, one
    pixel into the second (1025 as 25 x 41), and five tiles of which the last is partial (4160).  A side of 1025 is past
    the library's cap of 1024 a side and must be refused, so a single row or column cannot cross a tile; instead: a
    whole tile as one row and as one column (pix / ny is 0 throughout, or pix itself), and 1026 pixels as 2 x 513 and
    513 x 2, where i or j steps in the middle of the first tile and two pixels lie on the far side of its edge.
    Off-centre, with du != dv: a swapped axis shows."""
    assert K.kPsfTile == K.kPsfBlock * K.kPsfPix == 1024
    tiles = -(-grid[0] * grid[1] // K.kPsfTile)
    assert tiles == {1: 1, 1023: 1, 1024: 1, 1025: 2, 1026: 2, 4160: 5}[grid[0] * grid[1]]
    case = R.psf_tile_case(grid)
    if max(grid) > 1024:
        with pytest.raises(ValueError, match="1..1024"):
            device_frame(case.frame).psf(R.SURFACE, weights="intensity", **case.options)
        return
    got, ref, slices = run_psf("psf pixel tiles", case)
    assert slices == 1 and got.image.shape == (1,) + grid


@pytest.mark.parametrize("filler", (0, R.PSF_FILLER), ids=("alone", "among_other_rows"))
@pytest.mark.parametrize("n", R.SIZES)
def test_psf_ray_slices_and_the_lds_tile(n, filler):
    """Rays of a bucket about the LDS tile (kPsfBlock = 256 rays) and the slice (kPsfMinSlice = 2048): alone in the
    frame (one slice until 3 * 2048 + 1 rows give three), and among 4196 rows of another surface, which raise n_rows
    and with it the slices (2 to 5) over the same rays: slices of 1, 128, 683 and 1229 rays, and at one ray a slice
    that starts where the bucket ends."""
    assert (K.kPsfBlock, K.kPsfMinSlice) == (256, 2048)
    got, ref, slices = run_psf("psf ray slices", R.psf_slice_case(n, filler))
    assert slices == max(1, (n + filler) // K.kPsfMinSlice)
    if filler:
        assert slices >= 2
    if n == 1 and filler:
        assert R.slice_range(1, slices, 1) == (1, 1)


@pytest.mark.parametrize("counts", ([[5]], [[3, 2]]), ids=("one_bucket", "two_buckets"))
def test_psf_more_slices_than_rays(counts):
    """20 000 rows of which 5 reach the surface.  One bucket: 9 slices over 5 rays, slices 5 to 8 start at and past the
    bucket's end.  Two wavelengths: 4 slices over 3 and 2 rays, and bucket 0's slice 3 starts on bucket 1's first ray
    with lo == hi, bucket 1's slice 3 has lo past hi."""
    case = R.psf_sparse_case(counts)
    got, ref, slices = run_psf("psf more slices than rays", case)
    assert case.n_rows == 20_000 and slices == 20_000 // (len(counts[0]) * K.kPsfMinSlice) > max(counts[0])
    lo, hi = R.slice_range(counts[0][-1], slices, slices - 1)
    assert lo > hi


def test_psf_buckets_of_1_300_4000_and_0_rays():
    """Two groups x three wavelengths: buckets of 1, 300 and 4000 rays share the slices (2, from n_rows), the second
    group has none: it is NaN, its three empty buckets start where the rays end, and the first group's image is the one
    the reference gives."""
    got, ref, slices = run_psf("psf uneven buckets", R.psf_bucket_case())
    assert slices == 2
    assert np.all(np.isnan(got.image[1])) and np.isnan(got.strehl[1]) and np.all(np.isfinite(got.image[0]))


def test_psf_dark_pixels_two_rays_in_antiphase():
    """I = 0 at the centre pixel: the bound there is eps^2, about 2e-13, where a flat 1e-5 could never fail."""
    got, ref, slices = run_psf("psf dark pixels (antiphase)", R.psf_antiphase_case())
    assert float(ref.image[0, 1, 1]) < 1e-20 and ref.bound[0, 1, 1] < 1e-12
    assert got.image[0, 1, 1] <= ref.bound[0, 1, 1] + float(ref.image[0, 1, 1])


def test_psf_dark_rings_of_an_airy_pattern():
    """A 4096-ray Vogel disk along a line through the first three minima of its Airy pattern: the reference's minima are
    1e-6 and below, and the bound follows them down as 2 eps sqrt(I)."""
    got, ref, slices = run_psf("psf dark pixels (Airy rings)", R.psf_airy_case())
    profile = ref.image[0, 256:, 0].astype(float)
    minima = [k for k in range(1, 256) if profile[k] < profile[k - 1] and profile[k] < profile[k + 1]]
    assert len(minima) >= 3 and max(profile[minima[:3]]) < 1e-4
    assert ref.bound[0, 256 + minima[0], 0] < 2e-8


@pytest.mark.parametrize("micrometres", (False, True), ids=("R2000mm", "R2e6um"))
def test_psf_large_phases(micrometres):
    """R / lambda_w = 5e6 cycles (R = 2000 with world_unit_um = 1000 at 0.4 um, and the same in micrometres), pixels out
    to 0.3 R, OPD of both signs, weights from 1e-12 to 1e6 with exact zeros: fp64's rounding of the phase, ulp(5e6) =
    9.3e-10 cycles, is a visible part of the budget."""
    case = R.psf_large_phase_case(micrometres)
    got, ref, slices = run_psf("psf large phases", case)
    radius, s = case.options["radius"], R.inverse_wavelength(0.4, case.options["world_unit_um"])
    assert math.isclose(radius * s, 5e6, rel_tol=1e-12) and np.hypot(got.u[-1] - got.centre[0], got.v[-1] - got.centre[1]) > 0.29 * radius
    inp = case.inputs(got.u, got.v)
    assert inp.opd.min() < 0 < inp.opd.max() and (inp.weight == 0).sum() > 50


# ---- the OTF ----------------------------------------------------------------------------------------------------------------
def run_mtf(family, frame, frequencies, rays_per_source=None, n_groups=1, **options):
    from pyrayt_amd.frame import pupil_axes

    device = device_frame(frame)
    grouping = dict(rays_per_source=rays_per_source, n_groups=n_groups) if rays_per_source else {}
    got = device.mtf(R.SURFACE, frequencies, **grouping, **options)
    rows, groups = R.select_rows(frame, R.SURFACE, rays_per_source, n_groups)
    ref = R.mtf_reference(rows[:, 9:12], rows[:, 12:15], rows[:, 1], groups, n_groups, frequencies,
                          options.get("azimuths", (0.0, 90.0)), options.get("focus", (0.0,)),
                          pupil_axes(options.get("axis")), centre=got.centre)
    assert np.array_equal(got.n_rays, ref.n_rays) and np.array_equal(got.n_missed, ref.n_missed)
    assert got.otf.shape == ref.re.shape
    nan = np.isnan(ref.re.astype(np.float64))
    assert np.array_equal(np.isnan(got.otf), nan)
    deviation = R.otf_deviation(got.otf, ref)
    ratio = np.where(nan, 0.0, deviation / ref.bound)
    if not nan.all():
        k = int(np.nanargmax(ratio))
        print(f"[bounds] {family} otf: largest deviation {np.nanmax(deviation):.3e}, largest deviation / bound "
              f"{ratio.ravel()[k]:.3f} (deviation {deviation.ravel()[k]:.3e}, bound {ref.bound.ravel()[k]:.3e}, "
              f"{deviation.size} values)")
        assert np.all(ratio <= 1.0), (family, float(ratio.ravel()[k]))
    if "reference" not in options:  # the device's own centroid, apart from the sums
        for g in range(n_groups):
            if ref.n_rays[g]:
                assert np.all(np.abs(got.centre[g].astype(LD) - ref.centroid[g]) <= ref.centre_bound[g]), g
    return got, ref, deviation


@pytest.mark.parametrize("p, slope, focus", ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.25, 0.5), (-1.0, -0.125, 0.3)),
                         ids=("focus0", "focus0_negative_phases", "shifted_plane", "shifted_plane_negative"))
def test_otf_one_ray_phasor_sweep(p, slope, focus):
    """One ray about a fixed reference=: OTF(nu) = exp(-2 pi i nu (p1 + delta s1)), 65 536 turns in 16 calls of 4096
    frequencies.  At focus 0 the turns reach v_cos_f32 / v_sin_f32 as they are (negative phases through v_fract_f64):
    the deviation is eps_hw itself.  At a shifted plane the turns are fp64 values the conversion rounds.  Every output
    is held to the budget, and the largest deviation to EPS_TRIG / 2: EPS_TRIG is twice the largest eps_hw on record
    (tools/trig_sweep.py, profiles/mtf/README.md), so a larger one here is a finding, not a constant to raise."""
    turns = R.sweep_turns()
    assert len(turns) == R.SWEEP_TURNS >= 65536 and len(np.unique(turns)) > 65000
    assert 0.0 in turns and 1 - 2.0 ** -24 in turns and 1 - 2.0 ** -30 in turns and R.EPS_HW_TURN in turns
    frame = R.mtf_single_ray(p, slope)
    device = device_frame(frame)
    got = np.concatenate([device.mtf(R.SURFACE, turns[at:at + R.SWEEP_CHUNK], azimuths=(0.0,), focus=(focus,),
                                     reference=(0.0, 0.0, 0.0)).otf[0, 0, 0] for at in range(0, len(turns), R.SWEEP_CHUNK)])
    ref = R.mtf_reference(frame[:, 9:12], frame[:, 12:15], frame[:, 1], np.zeros(1, dtype=np.int64), 1, turns,
                          azimuths=(0.0,), focus=(focus,), centre=np.zeros((1, 3)))
    deviation = R.otf_deviation(got, SimpleNamespace(re=ref.re[0, 0, 0], im=ref.im[0, 0, 0]))
    ratio = deviation / ref.bound[0, 0, 0]
    k = int(np.argmax(ratio))
    print(f"[bounds] otf one-ray sweep otf: largest deviation {deviation.max():.3e}, largest deviation / bound "
          f"{ratio[k]:.3f} (deviation {deviation[k]:.3e}, bound {ref.bound[0, 0, 0, k]:.3e}, {deviation.size} values)")
    k = int(np.argmax(deviation))
    print(f"[bounds] eps_hw on this sweep: {deviation[k]:.4e} at nu = {turns[k].hex()} "
          f"(recorded {R.EPS_HW_MEASURED:.4e} at turn {R.EPS_HW_TURN.hex()}, EPS_TRIG {R.EPS_TRIG:.0e})")
    assert np.all(ratio <= 1.0)
    assert deviation.max() <= R.EPS_TRIG / 2


def test_otf_first_order_correction_pairs():
    """What k_mtf_sum puts back for the conversion to float: an fp64 turn t and the float tf it rounds to reach the same
    v_cos_f32 / v_sin_f32, so OTF(t) = OTF(tf) (1 - i theta), theta = 2 pi (t - tf), to the two fmas' roundings (4 u),
    whatever eps_hw is.  The budget's own bound cannot see this term: theta <= 2 pi 2^-25 = 1.9e-7 lies under
    EPS_TRIG."""
    rng = np.random.default_rng(3)
    tf = (0.5 + 0.5 * rng.random(256, dtype=np.float32)).astype(np.float32)
    tf = tf[tf < np.float32(0.999)].astype(np.float64)
    delta = np.where(rng.random(len(tf)) < 0.5, -1.0, 1.0) * rng.uniform(0.3, 0.98, len(tf)) * 2.0 ** -25
    t = tf + delta
    assert np.array_equal(t.astype(np.float32).astype(np.float64), tf) and np.all(t != tf)
    device = device_frame(R.mtf_single_ray(1.0))
    got = device.mtf(R.SURFACE, np.concatenate([t, tf]), azimuths=(0.0,), reference=(0.0, 0.0, 0.0)).otf[0, 0, 0]
    theta = R.TWO_PI * (t.astype(LD) - tf.astype(LD))
    base_re, base_im = got[len(t):].real.astype(LD), got[len(t):].imag.astype(LD)
    want_re, want_im = base_re + theta * base_im, base_im - theta * base_re
    gap = np.hypot(got[:len(t)].real.astype(LD) - want_re, got[:len(t)].imag.astype(LD) - want_im).astype(float)
    uncorrected = np.abs(got[:len(t)] - got[len(t):])
    print(f"[bounds] otf first-order correction: largest gap {gap.max():.3e} (bound {4 * R.U64:.3e}); the correction "
          f"itself is up to {uncorrected.max():.3e}")
    assert gap.max() <= 4 * R.U64 and uncorrected.max() > 1e-7


@pytest.mark.parametrize("outputs", tuple(R.MTF_OUTPUTS))
@pytest.mark.parametrize("n", R.SIZES)
def test_otf_rays_per_group(n, outputs):
    """Rays of a group about the LDS tile (kMtfBlock = 256) and the slice (kMtfMinSlice = 2048: 2049 rays are two slices
    of 1025, 3 * 2048 + 1 four of 1537), with 24 outputs (lanes = 4: four waves split the tile's rays and their sums are
    folded), 300 (lanes = 2) and 520 (lanes = 1)."""
    options = R.MTF_OUTPUTS[outputs]
    n_out = len(options["frequencies"]) * len(options["azimuths"]) * len(options.get("focus", (0.0,)))
    assert R.mtf_lanes(n_out) == int(outputs[-1])
    assert R.mtf_slices(n, 1, n_out) == -(-n // K.kMtfMinSlice)
    case = R.mtf_case([n], left_out=1 if n > 1 else 0, seed=40 + n)
    options = dict(options)
    run_mtf(f"otf rays per group ({outputs})", case.frame, options.pop("frequencies"), **options)


@pytest.mark.parametrize("shape", R.MTF_OUTPUT_COUNTS, ids=lambda s: str(s[0] * s[1] * s[2]))
def test_otf_output_tiles(shape):
    """planes x azimuths x frequencies one below, on and one above a workgroup's tile of threads * kMtfOut outputs:
    255 / 256 (lanes = 4, tile 256), 257 (the first count with lanes = 2), 511 / 512 (tile 512), 513 (the first with
    lanes = 1), 1023 / 1024 / 1025 (tile 1024: the last needs a second, almost empty tile)."""
    n_out = shape[0] * shape[1] * shape[2]
    lanes, tile = R.mtf_lanes(n_out), R.mtf_tile(n_out)
    assert (lanes, tile) == {255: (4, 256), 256: (4, 256), 257: (2, 512), 511: (2, 512), 512: (2, 512), 513: (1, 1024),
                             1023: (1, 1024), 1024: (1, 1024), 1025: (1, 1024)}[n_out]
    options = R.mtf_output_options(shape)
    got, ref, deviation = run_mtf(f"otf output tiles (lanes {lanes})", R.mtf_case([300], seed=50).frame,
                                  options.pop("frequencies"), **options)
    assert got.otf.shape == (1,) + shape


def test_otf_groups_of_very_uneven_size():
    """Groups of 1, 5000, 0, 300 and 2049 rays along a tilted axis, shuffled among 3000 rows of another surface, two
    rows a group left out: 1 + 2 + 1 + 1 + 1 chunks of 4096 and 1 + 3 + 1 + 1 + 2 slices, each bordering another
    group's."""
    counts = [1, 5000, 0, 300, 2049]
    case = R.mtf_case(counts, filler=3000, left_out=2, axis=(1.0, 0.2, 0.0), seed=60)
    assert [R.mtf_slices(c, 5, 48) for c in counts] == [1, 3, 1, 1, 2]
    got, ref, deviation = run_mtf("otf uneven groups", case.frame, np.linspace(0.0, 330.0, 12), azimuths=(0.0, 90.0),
                                  focus=(0.0, 0.03), **case.options)
    assert list(got.n_rays) == counts and list(got.n_missed) == [2] * 5 and np.all(np.isnan(got.otf[2]))


def test_otf_twenty_thousand_cycles():
    """nu p up to 2e4 cycles: 4000 cycles per unit about a reference= five units away, at azimuths 0, 90, 33 degrees and
    along p itself; the fp64 phase's rounding, 13 u times 2e4 cycles (1.8e-10), is what the last term of the budget
    is for."""
    case = R.mtf_case([500], seed=70)
    nu = np.concatenate([[0.0, 1.0], np.linspace(3.0, 4000.0, 14)])
    got, ref, deviation = run_mtf("otf 2e4 cycles", case.frame, nu, azimuths=R.FAR_AZIMUTHS, focus=(0.0, 0.01),
                                  reference=R.FAR_REFERENCE)
    # T, the magnitudes of the phase's terms the reference itself summed: 2e4 cycles along the azimuth of p
    assert 1.95e4 < ref.phase_terms[0, :, 3].max() < 2.1e4 and 1.5e4 < ref.phase_terms[0, :, 1].max() < 1.7e4
    assert ref.bound.max() > R.EPS_TRIG + 2 * math.pi * R.K_OTF * R.U64 * 1.95e4


def test_otf_azimuths_half_a_turn_apart():
    """theta and theta + 180 degrees: k changes sign, the OTF is conjugated; both are held to the reference, and to each
    other by twice the bound."""
    case = R.mtf_case([700], seed=80)
    got, ref, deviation = run_mtf("otf azimuths half a turn apart", case.frame, np.linspace(0.0, 300.0, 16),
                                  azimuths=(0.0, 180.0, 37.0, 217.0), focus=(0.0, 0.04))
    for a in (0, 2):
        assert np.all(np.abs(got.otf[:, :, a] - np.conj(got.otf[:, :, a + 1])) <= 2 * ref.bound[:, :, a])


def test_otf_scan_of_41_planes():
    """A through-focus scan of 41 planes x 2 azimuths x 5 frequencies = 410 outputs (lanes = 2): kc delta and ks delta
    are rounded once per output."""
    case = R.mtf_case([600], seed=90)
    got, ref, deviation = run_mtf("otf 41-plane scan", case.frame, np.linspace(0.0, 200.0, 5),
                                  focus=np.linspace(-0.2, 0.2, 41))
    assert got.otf.shape == (1, 41, 2, 5) and R.mtf_lanes(410) == 2 and math.isclose(got.focus[20], 0.0, abs_tol=1e-17)
