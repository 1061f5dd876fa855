"""The longdouble reference of the diffraction sums (tests/diffraction_reference.py) on the CPU: against exact cases and
against mpmath at 50 digits, to a few longdouble ulps (the figure reached is printed); the error budget's constants;
and the budget's teeth: mutations of the reference -- a ray dropped, a pixel's indices swapped, a slice shifted by one
ray, 1e-6 turn added to the phases, the conversion to float left uncorrected -- must break the bound on the inputs the
GPU tests run (tests/test_gpu_diffraction_bounds.py builds its frames from the same functions)."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import diffraction_reference as R

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
ULPS = 8  # "a few longdouble ulps" of the sum of the magnitudes

try:
    import mpmath
except ImportError:  # pragma: no cover
    mpmath = None


def exact_phasor(cycles):
    """(cos, sin)(2 pi cycles) of an exact rational number of cycles: mpmath at 50 digits, or with the phase reduced
    exactly by fractions and the remainder's sine and cosine from longdouble."""
    frac = cycles - math.floor(cycles)
    if mpmath is not None:
        mpmath.mp.dps = 50
        angle = 2 * mpmath.pi * (mpmath.mpf(frac.numerator) / frac.denominator)
        return mpmath.cos(angle), mpmath.sin(angle)
    angle = R.TWO_PI * (LD(frac.numerator) / LD(frac.denominator))
    return np.cos(angle), np.sin(angle)


def to_ld(x):
    return LD(mpmath.nstr(x, 30)) if mpmath is not None and isinstance(x, mpmath.mpf) else LD(x)


def one_pixel(opd, weight, pupil, unit=1.0, wavelength=0.5, radius=1e4, rho=500.0, u=(0.0,), v=(0.0,)):
    n = len(opd)
    return R.psf_inputs(np.zeros(n), np.full(n, wavelength), opd, pupil, weight, [radius], [rho], [wavelength], unit, u, v, 1)


# ---- exact cases --------------------------------------------------------------------------------------------------------------
def test_the_format_and_the_constants_of_the_budget():
    assert np.finfo(LD).eps == LD(2) ** -63 and EPS < 1.1e-19
    assert abs(float(R.PI) - math.pi) < 1e-15 and np.sin(R.PI) < 2 * EPS
    # EPS_TRIG: twice the measured eps_hw, rounded up to one digit; never above what DESIGN.md claimed before
    digit = 10.0 ** math.floor(math.log10(2 * R.EPS_HW_MEASURED))
    assert R.EPS_TRIG == pytest.approx(math.ceil(2 * R.EPS_HW_MEASURED / digit) * digit, rel=1e-12)
    assert R.EPS_HW_MEASURED <= 5e-7 and R.EPS_TRIG <= 1e-6
    assert 0 <= R.EPS_HW_TURN < 1 and float(np.float32(R.EPS_HW_TURN)) == R.EPS_HW_TURN
    # the partition rules are the code's
    assert (R.K.kPsfBlock, R.K.kPsfPix, R.K.kPsfTile, R.K.kPsfMinSlice) == (256, 4, 1024, 2048)
    assert (R.K.kMtfBlock, R.K.kMtfOut, R.K.kMtfChunk, R.K.kMtfMinSlice, R.K.kMtfMaxSlices) == (256, 4, 4096, 2048, 256)
    assert [R.mtf_lanes(n) for n in (1, 256, 257, 512, 513)] == [4, 4, 2, 2, 1]
    assert [R.mtf_tile(n) for n in (256, 257, 513)] == [256, 512, 1024]
    assert R.slice_range(5, 4, 3) == (6, 5) and R.slice_range(2049, 3, 2) == (1366, 2049)
    assert R.psf_slices(20_000, 2, 63, 256) == 4 and R.psf_slices(2049, 1, 63, 256) == 1
    assert R.wf_waves(20_000) == 20


def test_the_host_rules_are_the_headers_own_lines():
    """psf_slices, slice_range, mtf_slices, mtf_lanes and mtf_tile restate lines of prt_frame_psf / prt_frame_mtf; the
    GPU tests place their cases by them.  The lines they restate must still stand in the headers, word for word."""
    import os

    for name, lines in R.HOST_RULES.items():
        text = " ".join(open(os.path.join(R.ROOT, "pyrayt_amd", "csrc", name)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, (name, line)


def test_two_rays_give_cos_squared():
    """I = cos^2(pi Delta) at the pixel where the two distances agree: 1 / lambda_w = 2 exactly, OPD = +-Delta / 4."""
    worst = 0.0
    for delta in (Fraction(1, 2), Fraction(1, 4), Fraction(1, 3), Fraction(123, 1000), Fraction(7, 8), Fraction(5, 2)):
        opd = np.array([float(delta) / 4, -float(delta) / 4])
        inp = one_pixel(opd, [9.0, 9.0], [[0.6, 0.0], [-0.6, 0.0]])
        ref = R.psf_reference(inp)
        cycles = (Fraction(opd[0]) - Fraction(opd[1])) * 2  # (of the fp64 OPD the reference was given)
        c, _ = exact_phasor(cycles / 2)
        gap = abs(float(ref.image[0, 0, 0] - to_ld(c * c)))
        worst = max(worst, gap)
        assert gap <= ULPS * EPS, (delta, gap)
        assert abs(float(ref.strehl[0] - to_ld(c * c))) <= ULPS * EPS
    assert float(R.psf_reference(one_pixel([0.125, -0.125], [9.0, 9.0], [[0.6, 0.0], [-0.6, 0.0]])).image[0, 0, 0]) <= EPS ** 2
    print(f"[reference] two rays, I = cos^2(pi Delta): within {worst / EPS:.2f} longdouble ulps of 1")


def test_equally_spaced_phasors_sum_to_zero():
    """N rays at p1 = k / N: OTF(nu) = 0 at nu = 1 .. N - 1, 1 at nu = 0 and N."""
    worst = 0.0
    for n in (2, 64, 1000, 4096 + 64):
        q = np.zeros((n, 3))
        q[:, 1] = np.arange(n) / n
        u = np.tile([1.0, 0.0, 0.0], (n, 1))
        nu = np.array([0.0, 1.0, 2.0, n - 1.0, float(n)] if n > 2 else [0.0, 1.0, 2.0])
        ref = R.mtf_reference(q, u, np.ones(n), np.zeros(n, dtype=int), 1, nu, azimuths=(0.0,), centre=np.zeros((1, 3)))
        size = np.hypot(ref.re[0, 0, 0], ref.im[0, 0, 0]).astype(float)
        # p1 = fl(k / n) is not k / n unless n is a power of two: the exact sum of the phasors of the fp64 points
        for k, value in enumerate(nu):
            want_re = sum(exact_phasor(Fraction(float(value)) * Fraction(x))[0] for x in q[:, 1]) / n
            worst = max(worst, abs(float(ref.re[0, 0, 0, k] - to_ld(want_re))))
        if n & (n - 1) == 0:
            assert np.all(size[1:-1] <= ULPS * EPS) and abs(size[0] - 1) <= EPS and abs(size[-1] - 1) <= ULPS * EPS
    assert worst <= ULPS * EPS
    print(f"[reference] equally spaced phasors: within {worst / EPS:.2f} longdouble ulps of the exact sums")


def test_the_dirichlet_kernel():
    """Rays at p1 = k h, k = 0 .. N - 1: OTF(nu) = exp(-i pi nu h (N - 1)) sin(pi nu h N) / (N sin(pi nu h))."""
    if mpmath is None:
        pytest.skip("the closed form is evaluated with mpmath")
    mpmath.mp.dps = 50
    n, h = 37, 2.0 ** -10
    q = np.zeros((n, 3))
    q[:, 2] = np.arange(n) * h
    u = np.tile([2.0, 0.0, 0.0], (n, 1))
    nu = np.array([0.3, 17.25, 1000.0 / 3.0, 4000.0, 27.675675675675677])
    ref = R.mtf_reference(q, u, np.full(n, 0.25), np.zeros(n, dtype=int), 1, nu, azimuths=(90.0,), centre=np.zeros((1, 3)))
    ks = nu * math.sin(90.0 * (math.pi / 180.0))
    worst = 0.0
    for k, value in enumerate(ks):
        x = mpmath.pi * mpmath.mpf(float(value)) * mpmath.mpf(h)
        want = mpmath.expj(-x * (n - 1)) * mpmath.sin(x * n) / (n * mpmath.sin(x))
        # kc = nu cos(90 degrees) is 6e-17 nu, not 0, and multiplies d.e1 = 0
        gap = math.hypot(float(ref.re[0, 0, 0, k] - to_ld(want.real)), float(ref.im[0, 0, 0, k] - to_ld(want.imag)))
        worst = max(worst, gap)
    assert worst <= ULPS * EPS
    print(f"[reference] the Dirichlet kernel: within {worst / EPS:.2f} longdouble ulps")


# ---- against mpmath at 50 digits --------------------------------------------------------------------------------------------
@pytest.mark.skipif(mpmath is None, reason="mpmath is not installed")
def test_the_psf_against_mpmath():
    mpmath.mp.dps = 50
    rng = np.random.default_rng(1)
    n, unit, lams = 7, 1000.0, np.array([0.4, 0.65])
    inp = R.psf_inputs(np.zeros(n), lams[rng.integers(0, 2, n)], rng.normal(0, 3e-4, n), rng.uniform(-0.7, 0.7, (n, 2)),
                       10.0 ** rng.uniform(-3, 3, n), [2000.0], [100.0], lams, unit, [-600.0, 0.0, 3.7], [-2e-3, 450.0], 1)
    ref = R.psf_reference(inp)
    f = mpmath.mpf
    den, largest = 0, 0.0
    amplitude = {}
    for k, lam in enumerate(lams):
        s = f(float(R.inverse_wavelength(lam, unit)))
        m = inp.wavelength == lam
        a = [f(float(np.sqrt(w))) for w in inp.weight[m]]
        den += (s * sum(a)) ** 2
        for i, uu in enumerate(inp.u):
            for j, vv in enumerate(inp.v):
                total = 0
                for ray, amp in zip(np.flatnonzero(m), a):
                    p1, p2 = f(float(inp.pupil[ray, 0] * 100.0)), f(float(inp.pupil[ray, 1] * 100.0))
                    d = mpmath.sqrt(f(2000.0) ** 2 + f(uu) ** 2 + f(vv) ** 2 - 2 * (f(uu) * p1 + f(vv) * p2))
                    cycles = (f(float(inp.opd[ray])) + d - 2000) * s
                    largest = max(largest, abs(float(cycles)))
                    total += amp * mpmath.expj(2 * mpmath.pi * cycles)
                amplitude[k, i, j] = abs(s * total) ** 2
    worst = max(abs(float(ref.image_by_wavelength[0, k, i, j] - to_ld(value / den))) for (k, i, j), value in amplitude.items())
    # the phase itself is a longdouble: a few ulps of 2 pi times its size in cycles (2e5 here, at 0.3 R) are what the
    # reference can hold at such a pixel, seven orders under the budget's eps; on the axis that is a few ulps of 1
    assert largest > 1e5 and worst <= ULPS * EPS * 2 * math.pi * largest
    print(f"[reference] PSF against mpmath at |u| up to 0.3 R, R / lambda_w = 5e6: {worst:.2e}, "
          f"{worst / (EPS * 2 * math.pi * largest):.2f} longdouble ulps of the phase (up to {largest:.3g} cycles)")
    near = R.psf_inputs(inp.group, inp.wavelength, inp.opd, inp.pupil, inp.weight, [2000.0], [100.0], lams, unit, [0.0], [0.0], 1)
    assert abs(float(R.psf_reference(near).image[0, 0, 0] - R.psf_reference(near).strehl[0])) <= ULPS * EPS


@pytest.mark.skipif(mpmath is None, reason="mpmath is not installed")
def test_the_otf_against_mpmath():
    from pyrayt_amd.frame import pupil_axes

    mpmath.mp.dps = 50
    f = mpmath.mpf
    rng = np.random.default_rng(2)
    n = 6
    axes = pupil_axes((1.0, 0.2, -0.1))
    q, u, w = rng.normal(0, 1.0, (n, 3)), rng.normal(0, 0.2, (n, 3)) + axes[:3], rng.uniform(0.1, 2.0, n)
    nu, az, focus = np.array([0.0, 3.3, 400.0]), (0.0, 30.0, 217.0), (0.0, -0.7)
    ref = R.mtf_reference(q, u, w, np.zeros(n, dtype=int), 1, nu, az, focus, axes)
    vec = lambda x: mpmath.matrix([f(float(v)) for v in x])  # noqa: E731
    dot = lambda x, y: sum(x[k] * y[k] for k in range(3))  # noqa: E731
    a, e1, e2 = vec(axes[:3]), vec(axes[3:6]), vec(axes[6:])
    total = sum(f(float(x)) for x in w)
    c = [sum(f(float(w[r])) * f(float(q[r, k])) for r in range(n)) / total for k in range(3)]
    kc, ks = R.frequency_table(nu, az)
    worst, largest = 0.0, 0.0
    for fi, delta in enumerate(focus):
        for ai in range(len(az)):
            for ni in range(len(nu)):
                value = 0
                for r in range(n):
                    d, uu = vec(q[r]) - mpmath.matrix(c), vec(u[r])
                    t = (dot(mpmath.matrix(c), a) + f(delta) - dot(vec(q[r]), a)) / dot(uu, a)  # X = Q + u t
                    x = d + uu * t
                    phase = f(float(kc[ai, ni])) * dot(x, e1) + f(float(ks[ai, ni])) * dot(x, e2)
                    largest = max(largest, abs(float(phase)))
                    value += f(float(w[r])) * mpmath.expj(-2 * mpmath.pi * phase)
                value /= total
                gap = math.hypot(float(ref.re[0, fi, ai, ni] - to_ld(value.real)), float(ref.im[0, fi, ai, ni] - to_ld(value.imag)))
                worst = max(worst, gap)
    assert worst <= ULPS * EPS * (1 + 2 * math.pi * largest)
    print(f"[reference] OTF against mpmath from the plane's own definition X = Q + u t: {worst:.2e}, "
          f"{worst / (EPS * (1 + 2 * math.pi * largest)):.2f} longdouble ulps of the phase (up to {largest:.3g} cycles)")


# ---- the budget's teeth: mutations on the inputs of the GPU tests -------------------------------------------------------------
def design(case):
    options = case.options
    size = options.get("pixel_size")
    u, v = R.pixel_centres(options["pixels"], size, options["centre"])
    return case.inputs(u, v)


@functools.lru_cache(maxsize=None)
def psf_family(name, key):
    case = {"tiles": R.psf_tile_case, "slices": lambda n: R.psf_slice_case(n, R.PSF_FILLER),
            "sparse": lambda c: R.psf_sparse_case([list(c)]), "buckets": lambda _: R.psf_bucket_case(),
            "antiphase": lambda _: R.psf_antiphase_case(), "airy": lambda _: R.psf_airy_case(),
            "large": R.psf_large_phase_case}[name](key)
    inp = design(case)
    return case, inp, R.psf_reference(inp)


def psf_breaks(ref, mutated):
    with np.errstate(invalid="ignore"):
        deviation = np.abs(mutated.image_by_wavelength - ref.image_by_wavelength).astype(float)
        return bool(np.nanmax(deviation / ref.bound_by_wavelength) > 1.0), float(np.nanmax(deviation / ref.bound_by_wavelength))


def slices_of(case, inp):
    return R.psf_slices(case.n_rows, inp.n_groups * len(inp.wavelengths), len(inp.u) * len(inp.v), 256)


def shifted(bucket, slices, which):
    """select(b, n): slice ``which`` of ``bucket`` reads its rays one place on."""
    def select(b, n):
        index = np.arange(n)
        if b == bucket:
            lo, hi = R.slice_range(n, slices, which)
            index[lo:hi] = np.minimum(index[lo:hi] + 1, n - 1)
        return index
    return select


def test_every_psf_family_runs_on_the_design_and_stays_within_its_size():
    """Every case at or under 2e7 reference terms; the reference of the design is finite where the group has rays."""
    keys = ([("tiles", g) for g in R.PSF_GRIDS + R.PSF_GRIDS_WITHIN_THE_CAP] + [("slices", n) for n in R.SIZES] + [("sparse", (5,)), ("sparse", (3, 2)),
            ("buckets", 0), ("antiphase", 0), ("airy", 0), ("large", False), ("large", True)])
    for name, key in keys:
        case, inp, ref = psf_family(name, key)
        assert int(case.counts.sum()) * len(inp.u) * len(inp.v) <= 2e7
        with_rays = case.counts.sum(axis=1) > 0
        assert np.all(np.isfinite(ref.image[with_rays].astype(float))) and np.all(np.isnan(ref.image[~with_rays].astype(float)))
        # the Strehl ratio's bound: two orders under the flat 1e-9 at R / lambda_w of 2e4 cycles; at 5e6 cycles fp64's
        # own rounding of the phase, ulp(5e6) = 9.3e-10 cycles, puts it at 2.5e-9
        assert np.all(ref.bound[with_rays] > 0) and np.all(ref.strehl_bound[with_rays] < (3e-9 if name == "large" else 1e-10))
        assert np.array_equal(ref.n_rays, case.counts)


def test_dropping_the_last_ray_of_a_2049_ray_bucket_breaks_the_psf_bound():
    case, inp, ref = psf_family("slices", 2049)
    broke, ratio = psf_breaks(ref, R.psf_reference(inp, select=lambda b, n: np.arange(n - 1)))
    print(f"[teeth] psf, last of 2049 rays dropped: {ratio:.1f} times the bound")
    assert broke


@pytest.mark.parametrize("grid", [g for g in R.PSF_GRIDS + R.PSF_GRIDS_WITHIN_THE_CAP if g[0] != g[1]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_swapping_i_and_j_of_one_pixel_breaks_the_psf_bound(grid):
    case, inp, ref = psf_family("tiles", grid)
    nx, ny = grid
    uu, vv = (x.ravel().copy() for x in np.meshgrid(inp.u, inp.v, indexing="ij"))
    du, dv = inp.u[1] - inp.u[0] if nx > 1 else case.options["pixel_size"][0], case.options["pixel_size"][1]
    # the brightest pixel whose swapped indices name another point
    order = np.argsort(-ref.image[0].astype(float).ravel())
    pick = next(k for k in order if (k // ny - 0.5 * (nx - 1)) * du != (k % ny - 0.5 * (ny - 1)) * du)
    i, j = pick // ny, pick % ny
    uu[pick] = case.options["centre"][0] + (j - 0.5 * (nx - 1)) * du
    vv[pick] = case.options["centre"][1] + (i - 0.5 * (ny - 1)) * dv
    broke, ratio = psf_breaks(ref, R.psf_reference(inp, uu=uu, vv=vv))
    print(f"[teeth] psf {nx}x{ny}, pixel ({i}, {j}) read as ({j}, {i}): {ratio:.1f} times the bound")
    assert broke


@pytest.mark.parametrize("name, key, bucket", (("slices", 3 * 2048 + 1, 0), ("slices", 2049, 0), ("slices", 255, 0),
                                               ("sparse", (5,), 0), ("sparse", (3, 2), 1), ("buckets", 0, 2)))
def test_shifting_one_slice_by_one_ray_breaks_the_psf_bound(name, key, bucket):
    case, inp, ref = psf_family(name, key)
    slices = slices_of(case, inp)
    assert slices >= 2
    broke, ratio = psf_breaks(ref, R.psf_reference(inp, select=shifted(bucket, slices, 0)))
    print(f"[teeth] psf {name} {key}: slice 0 of {slices} shifted by one ray: {ratio:.1f} times the bound")
    assert broke


def test_a_common_phase_offset_cannot_show_in_the_psf_but_one_on_every_other_ray_does():
    """|U|^2 does not change when 1e-6 turn is added to every phase: that mutation belongs to the OTF.  Added to every
    second ray it is a wavefront error of 1e-6 turn and breaks the bound where the image is bright."""
    case, inp, ref = psf_family("slices", 2049)
    same = R.psf_reference(inp, offset=lambda b, n: np.full(n, 1e-6))
    assert np.abs(same.image - ref.image).max() <= 64 * EPS
    broke, ratio = psf_breaks(ref, R.psf_reference(inp, offset=lambda b, n: 1e-6 * (np.arange(n) % 2)))
    print(f"[teeth] psf, 1e-6 turn on every second ray: {ratio:.2f} times the bound")
    # a sixth of eps: a phase error this small in the rays is what eps allows every ray, and stays inside the budget
    assert not broke
    broke, ratio = psf_breaks(ref, R.psf_reference(inp, offset=lambda b, n: 1e-5 * (np.arange(n) % 2)))
    print(f"[teeth] psf, 1e-5 turn on every second ray: {ratio:.2f} times the bound")
    assert broke


@functools.lru_cache(maxsize=None)
def mtf_family(name):
    """(rows, groups, n_groups, reference arguments) of a GPU family's inputs."""
    from pyrayt_amd.frame import pupil_axes

    if name.startswith("rays"):
        n = int(name.split("_")[1])
        case, options = R.mtf_case([n], left_out=1 if n > 1 else 0, seed=40 + n), dict(R.MTF_OUTPUTS["lanes4"])
    elif name == "tiles":
        case, options = R.mtf_case([300], seed=50), R.mtf_output_options((3, 5, 17))
    elif name == "uneven":
        case = R.mtf_case([1, 5000, 0, 300, 2049], filler=3000, left_out=2, axis=(1.0, 0.2, 0.0), seed=60)
        options = dict(frequencies=np.linspace(0.0, 330.0, 12), azimuths=(0.0, 90.0), focus=(0.0, 0.03))
    elif name == "far":
        case = R.mtf_case([500], seed=70)
        options = dict(frequencies=np.concatenate([[0.0, 1.0], np.linspace(3.0, 4000.0, 14)]), azimuths=R.FAR_AZIMUTHS,
                       focus=(0.0, 0.01), centre=np.array([[0.3, -3.0, 4.0]]))
    elif name == "half_turn":
        case = R.mtf_case([700], seed=80)
        options = dict(frequencies=np.linspace(0.0, 300.0, 16), azimuths=(0.0, 180.0, 37.0, 217.0), focus=(0.0, 0.04))
    elif name == "scan":
        case, options = R.mtf_case([600], seed=90), dict(frequencies=np.linspace(0.0, 200.0, 5), focus=np.linspace(-0.2, 0.2, 41))
    else:
        sign, plane = {"sweep": (1.0, None), "sweep_shifted": (1.0, (0.25, 0.5)), "sweep_negative": (-1.0, (-0.125, 0.3))}[name]
        frame = R.mtf_single_ray(sign, plane[0] if plane else 0.0)
        options = dict(frequencies=R.sweep_turns(), azimuths=(0.0,), focus=(plane[1] if plane else 0.0,), centre=np.zeros((1, 3)))
        case = None
    if case is not None:
        grouped = len(case.frame) and case.n_groups > 1
        rows, groups = R.select_rows(case.frame, R.SURFACE, case.rays_per_source if grouped else None, case.n_groups)
        n_groups, axes = case.n_groups, pupil_axes(case.axis)
    else:
        rows, groups, n_groups, axes = frame, np.zeros(1, dtype=np.int64), 1, None
    args = (rows[:, 9:12], rows[:, 12:15], rows[:, 1], groups, n_groups, options.pop("frequencies"))
    options["axes"] = axes
    return args, options, R.mtf_reference(*args, **options)


MTF_FAMILIES = ("sweep", "sweep_shifted", "sweep_negative", "rays_1", "rays_257", "rays_2049", f"rays_{3 * 2048 + 1}", "tiles",
                "uneven", "far", "half_turn", "scan")


def otf_breaks(ref, mutated):
    with np.errstate(invalid="ignore"):
        ratio = np.hypot((mutated.re - ref.re).astype(float), (mutated.im - ref.im).astype(float)) / ref.bound
    return bool(np.nanmax(ratio) > 1.0), float(np.nanmax(ratio))


@pytest.mark.parametrize("name", MTF_FAMILIES)
def test_a_millionth_of_a_turn_on_every_phase_breaks_the_otf_bound(name):
    args, options, ref = mtf_family(name)
    assert args[0].shape[0] * ref.re.size <= 2e7
    broke, ratio = otf_breaks(ref, R.mtf_reference(*args, offset=1e-6, **options))
    print(f"[teeth] otf {name}: 1e-6 turn on every phase: {ratio:.1f} times the bound")
    assert broke


def test_dropping_the_last_ray_of_a_2049_ray_group_breaks_the_otf_bound():
    args, options, ref = mtf_family("rays_2049")
    broke, ratio = otf_breaks(ref, R.mtf_reference(*args, select=lambda g, n: np.arange(n - 1), **options))
    print(f"[teeth] otf, last of 2049 rays dropped: {ratio:.1f} times the bound")
    assert broke


@pytest.mark.parametrize("name, group", ((f"rays_{3 * 2048 + 1}", 0), ("rays_2049", 0), ("uneven", 1), ("uneven", 4)))
def test_shifting_one_slice_by_one_ray_breaks_the_otf_bound(name, group):
    args, options, ref = mtf_family(name)
    slices = R.mtf_slices(int(ref.n_rays[group]), ref.re.shape[0], ref.re[0].size)
    assert slices >= 2
    broke, ratio = otf_breaks(ref, R.mtf_reference(*args, select=shifted(group, slices, 1), **options))
    print(f"[teeth] otf {name}: slice 1 of {slices} of group {group} shifted by one ray: {ratio:.1f} times the bound")
    assert broke


@pytest.mark.parametrize("name", MTF_FAMILIES)
def test_what_the_uncorrected_conversion_to_float_costs(name):
    """Skipping k_mtf_sum's first-order correction moves a phasor by at most 2 pi 2^-25 = 1.87e-7, and EPS_TRIG, twice
    the measured eps_hw, is 3e-7: the OTF bound cannot tell this mutation from the instruction's own error on any
    input, and over many rays it averages down further.  It is held by a sharper check of its own instead
    (test_otf_first_order_correction_pairs on the GPU): the mutated reference misses that check's 4 u by eight orders."""
    args, options, ref = mtf_family(name)
    mutated = R.mtf_reference(*args, float_turn=True, **options)
    gap = np.nanmax(np.hypot((mutated.re - ref.re).astype(float), (mutated.im - ref.im).astype(float)))
    print(f"[teeth] otf {name}: conversion left uncorrected: {gap:.3e} (the bound is {np.nanmin(ref.bound):.3e} or more)")
    assert gap <= 2 * math.pi * R.F32_TURN * (1 + 1e-9) < R.EPS_TRIG
    if name.startswith("sweep"):  # one ray: the pair check's quantity, |OTF(t) - OTF(float(t)) (1 - i theta)|
        turns = args[5]
        inexact = turns.astype(np.float32).astype(np.float64) != turns
        if name == "sweep":
            assert inexact.sum() >= 6 and gap > 1e-8 > 1e6 * 4 * R.U64
        else:
            assert gap > 1e-7


# ---- never looser than the tolerances the older tests used ------------------------------------------------------------------
def test_the_budget_is_tighter_than_the_flat_tolerances_on_the_older_tests_frames():
    """tests/test_gpu_psf.py used 1e-5 (per wavelength), 2e-5 (image) and 1e-9 (Strehl); tests/test_gpu_mtf.py 1e-6."""
    import helpers

    # PSF: I_l <= f_l, so the bound is at most (2 eps + eps^2) f_l per wavelength and 2 eps + eps^2 for the image,
    # whatever the image: eps on the frames' geometry, every pixel of their grids
    frame = helpers.psf_synthetic_frame()
    last = frame[frame[:, 5] == 5.0]
    centre = last[:, 9:12].mean(axis=0)
    radius = np.linalg.norm(centre - last[:, 6:9].mean(axis=0))
    lam_f = 0.55e-3 * 5.0
    grid = np.meshgrid(1.3 * lam_f + (np.arange(33) - 16) * 0.5 * lam_f, -0.7 * lam_f + (np.arange(31) - 15) * 0.5 * lam_f)
    eps = R.psf_epsilon(radius, R.inverse_wavelength(0.55, 1000.0), 1.5, 0.1, grid[0].ravel(), grid[1].ravel()).max()
    assert 2 * eps + eps * eps < 1e-5 / 5
    eta, depth = R.strehl_eta(radius, R.inverse_wavelength(0.55, 1000.0), 0.1, 3000, 1)
    assert 2 * (2 * eta + eta * eta) + (2 * depth + 10) * R.U64 < 1e-9 / 5
    config2 = helpers.load("scene_config2.npz")["frame"]
    imager = config2[config2[:, 0] == config2[:, 0].max()][-1, 5]
    last = config2[config2[:, 5] == imager]
    radius = np.linalg.norm(last[:, 9:12].mean(axis=0) - last[:, 6:9].mean(axis=0))
    s = R.inverse_wavelength(last[:, 2].min(), 1000.0)
    extent = 20 * last[:, 2].min() * 1e-3 * 10  # (33 pixels of lambda F / 4 at F < 10)
    eps = R.psf_epsilon(radius, s, 0.5 * radius / 2, 0.1, np.array([extent]), np.array([extent])).max()
    eta, depth = R.strehl_eta(radius, s, 0.1, len(last), 1)
    assert 2 * eps + eps * eps < 1e-5 / 5 and 2 * (2 * eta + eta * eta) + (2 * depth + 10) * R.U64 < 1e-9 / 5
    # MTF: the bound itself on the frames and arguments of check_mtf
    frame, axis = helpers.mtf_synthetic_frame()
    from pyrayt_amd.frame import pupil_axes

    rows, groups = R.select_rows(frame, 5.0, 6000, 2)
    nu = np.concatenate([[0.0], np.linspace(1.0, 400.0, 37)])
    ref = R.mtf_reference(rows[:, 9:12], rows[:, 12:15], rows[:, 1], groups, 2, nu, (0.0, 30.0, 90.0, 200.0),
                          (-0.05, 0.0, 0.02, 0.1), pupil_axes(axis))
    assert ref.n_missed.sum() == 5 and np.nanmax(ref.bound) < 1e-6 / 3
    rows, groups = R.select_rows(config2, imager, 512, int(config2[:, 4].max() // 512) + 1)
    ref = R.mtf_reference(rows[:, 9:12], rows[:, 12:15], rows[:, 1], groups, int(groups.max()) + 1, np.linspace(0.0, 60.0, 25),
                          (0.0, 45.0, 90.0), (-0.2, 0.0, 0.3))
    assert np.nanmax(ref.bound) < 1e-6 / 3
    print(f"[budget] PSF eps {eps:.2e}: image bound at most {2 * eps:.1e} against 1e-5; OTF bound {np.nanmax(ref.bound):.2e} "
          "against 1e-6")
