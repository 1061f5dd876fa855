"""An extended-precision reference of the two diffraction sums (the Huygens PSF with its Strehl ratio, and the
geometric OTF: the definitions of include/prt.h), the error budget the HIP kernels are held to, and the inputs the
tests run on.  Everything after the kernels' own inputs is np.longdouble (80-bit, eps 2^-63).

What counts as an input.  PSF: the wavefront's opd, pupil, radius and pupil_radius, the frame's weight and wavelength
columns, 1 / lambda_w as the library forms it and the pixel centres PSF.u / PSF.v; p = pupil * rho is formed in fp64 as
k_psf_stage forms it.  MTF: the frame's rows, the (kc, ks) table as the library's host code forms it (libm's cos and
sin of azimuth * (pi / 180), times nu, in fp64) and the centre C_g the device used (its own centroid is held to
``centroid_bound`` apart from the sums).

The budget.  u = 2^-53 is fp64's unit roundoff; ulp(x) is the spacing of fp64 at x, so u x < ulp(x) <= 2 u x.
EPS_TRIG bounds eps_hw, the distance between (v_cos_f32(t), v_sin_f32(t)) and the unit phasor of the float turn t: it
is measured, not derived (see EPS_HW_MEASURED).  |exp(ia) - exp(ib)| <= |a - b| turns every phase error e (cycles) into
2 pi e of phasor error.

OTF, per output (``otf_bound``): eps_hw + (2 pi 2^-25)^2 / 2 + 2 pi K_OTF u T.
  * The conversion of a turn in [0, 1) to float moves it by at most half a float ulp below 1, 2^-25; k_mtf_sum puts
    theta = 2 pi (turn - float) back as (c + i s)(1 + i theta), which leaves theta^2 / 2 of exp(i theta).
  * T is the weighted mean over the rays of the magnitudes that enter the phase:
    T_r = |kc| P1 + |ks| P2 + |delta| (|kc| S1 + |ks| S2), with A(x, e) = sum_k |x_k e_k|,
    S1 = (A(u, e1) + |s1| A(u, a)) / |u.a| >= |s1| and P1 = A(d, e1) + S1 A(d, a) >= |p1| (on the default axes
    P1 = |d.e1| + 2 |s1 d.a| and S1 = 2 |s1|).
  * K_OTF = 13 counts roundings to first order, each relative to the magnitude it acts on, fused or not:
    d = Q - C 1; a dot product of three terms 3 (so d.e1 and d.a 4 each); s1 = (u.e1) / (u.a) 3 + 3 + 1, at most 4 S1;
    s1 (d.a) 4 + 4 + 1 = 9 and the subtraction 1: p1 is within 10 u P1.  The chain fma(kc, p1, fma(ks, p2,
    fma(kc delta, s1, (ks delta) s2))) adds one rounding for each of kc delta and ks delta, one for the innermost
    product and one per fma: the p terms carry 10 + 2 = 12, the s terms 4 + 1 + 1 + 3 = 9.  12, and one more for
    the terms of second order.  v_fract_f64 is exact.
PSF, per pixel and (group, wavelength) bucket (``psf_epsilon``, ``psf_bound``): |U~ - U| <= eps sum a gives
  |I~ - I| <= 2 eps sqrt(I f) + eps^2 f on the normalised intensity, f = (sum a / lambda_w)^2 over the group's
  denominator (f = 1 for one wavelength: 2 eps sqrt(I) + eps^2); the bounds of a group's buckets add up
  for ``image``.  eps = eps_hw + 2 pi 2^-25 + 2 pi k' ulp(M): the PSF does not correct the conversion.  M is the largest
  fp64 value on the way to the phase, max(R + |OPD|, d) / lambda_w, and k' counts, in ulp(M):
    c = ((OPD - R) / lambda_w): two roundings, 2;  k0 = R^2 + u^2 + v^2 three roundings and the two fmas of |x - E|^2
    two, each relative to k0 + 2 rho r or less: 5 u kappa on d^2 with kappa = (k0 + 2 rho r) / (k0 - 2 rho r), half of
    it on d: 2.5 kappa;  psf_sqrt's last Goldschmidt step is not rounded to nearest but is faithful, one ulp of d: 2;
    fma(d, 1 / lambda_w, c): 1;  the pixel centres, which the kernel may form with one fma where numpy rounds twice, one
    ulp of u and of v: 3 r (r + rho) / k0.  About 7.5 on the axis.
Strehl (``strehl_bound``): fp64 sincospi of fma(R, 1 / lambda_w, c).  eta = 2 pi 2 ulp((R + |OPD|) / lambda_w)
  + (4 + 1 + depth) u: c's two roundings are half an ulp of R + |OPD| scaled and half an ulp of c, 1.5 ulp, the fma
  rounds OPD / lambda_w, together under 2; sincospi within 2 ulp of fp64, 4 u; a * cos 1; depth = the additions a term
  passes through (ceil(rays of a slice / kPsfBlock), the tree's log2 kPsfBlock, the slices).  The ratio then moves by
  sum over the buckets of 2 eta sqrt(S_l f_l) + eta^2 f_l, plus (2 depth + 10) u S for sum a, the squares and the
  division.

What the budget leaves to EPS_TRIG's margin: the fp64 accumulation of the kernels' own sums (at most rays-per-slice
times u of sum a, under 1e-12 at the sizes tested) and their normalisation (a few u).  EPS_TRIG is twice the largest
measured value, so its margin is eps_hw itself, five orders above those.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps == LD(2) ** -63, "np.longdouble is not the 80-bit extended format here"
PI = LD("3.14159265358979323846264338327950288")
TWO_PI = 2 * PI
U64 = 2.0 ** -53
F32_TURN = 2.0 ** -25  # (half a float ulp below 1)

# Measured on an MI355X by tools/trig_sweep.py (it writes profiles/mtf/trig_sweep.json and the table of
# profiles/mtf/README.md) through DeviceFrame.mtf: one ray with p1 = +1 / -1 exactly and reference= fixed gives
# OTF(nu) = exp(-2 pi i nu p1), so a frequency sweep reads v_cos_f32 / v_sin_f32 out directly.  Sampled: every float turn
# of the ten binades from 2^-10 to 1 (8.4e7 turns), every multiple of 2^-24 with both signs of the phase (negative ones
# go through v_fract_f64), 0, the quarter turns and eight neighbours each side, 2^-k down to 2^-59, 1 - 2^-24, and fp64
# turns that round in the conversion (1 - 2^-30 rounds up to 1.0f).  Below 2^-10 turn only the powers of two and random
# turns were sampled; the largest value per binade falls from 1.4e-7 to 7e-8 on the way there (profiles/mtf/README.md).
EPS_HW_MEASURED = 1.4398e-07  # the largest distance found, and the float turn where it was found
EPS_HW_TURN = float.fromhex("0x1.3fe062p-5")  # 0.039047423750162125
EPS_TRIG = 3e-7               # twice EPS_HW_MEASURED, rounded up to one digit: the sample is not every float turn
K_OTF = 13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernels' partition rules, read from the code ---------------------------------------------------------------------
def kernel_constants():
    """The static const ints of prt_psf.hpp, prt_mtf.hpp and prt_wavefront.hpp (kPsfBlock, kMtfOut, ...)."""
    found = {}
    for name in ("prt_wavefront.hpp", "prt_psf.hpp", "prt_mtf.hpp"):
        text = open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read()
        for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
            value = re.sub(r"(\d+)u\b", r"\1", value)
            try:
                found[key] = int(eval(value, {"__builtins__": {}}, dict(found)))  # (sums, products of earlier names)
            except (NameError, SyntaxError, TypeError):
                pass  # (not a plain constant)
    return SimpleNamespace(**found)


K = kernel_constants()
# The host rules below (psf_slices, mtf_slices, mtf_lanes) are Python copies of lines of psf_plan (with the arguments
# prt_frame_psf gives it) / mtf_slices and mtf_plan (with the arguments prt_frame_mtf gives it):
# the device's own slice count is not observable, so tests/test_host_diffraction_reference.py holds the copies to the
# header text (HOST_RULES), and a change of a rule there fails that test instead of moving the GPU tests off their edges.
HOST_RULES = {
    "prt_psf.hpp": (
        "const int64_t tiles = (npix + tile_pixels - 1) / tile_pixels;",
        "int64_t slices = (4 * (int64_t)cus + tiles * buckets - 1) / (tiles * buckets);",
        "slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_items / (sort_buckets * kPsfMinSlice)));",
        "slices = std::min<int64_t>(slices, (int64_t)(kPsfSlabBytes / ((size_t)buckets * npix * pixel_bytes)));",
        "slices = std::max<int64_t>(1, std::min<int64_t>(slices, kPsfMaxSlices));",
        "const PsfPlan plan = psf_plan(cus, n_rows, buckets, buckets, npix, kPsfTile, 16, 16, 3);",
        "const int64_t n = bucket_total[b], per = (n + slices - 1) / slices;"),
    "prt_mtf.hpp": (
        "const int64_t s = (count + kMtfMinSlice - 1) / kMtfMinSlice;",
        "return s < 1 ? 1 : (s > max_slices ? max_slices : s);",
        "const size_t cells = (size_t)n_groups * n_out * cell_bytes;",
        "p.max_slices = std::max<int64_t>(1, std::min<int64_t>(kMtfMaxSlices, (int64_t)(kMtfSlabBytes / cells)));",
        "const int lanes = n_out <= out * block / 4 ? 4 : (n_out <= out * block / 2 ? 2 : 1);",
        "const int64_t tile = (int64_t)out * (block / lanes), tiles = (n_out + tile - 1) / tile;",
        'int rc = mtf_plan("mtf", frequencies, n_frequencies, azimuths_deg, n_azimuths, focus, n_focus, axes, n_groups, 16,',
        "kMtfOut, kMtfBlock, plan);"),
}


def wf_waves(n_rows):
    """wf_waves(n_rows, 1) of prt_wavefront.hpp: the waves of the PSF's row passes (before the count cap)."""
    return min(max(-(-n_rows // K.kWfRowsPerWave), 1), K.kWfMaxWaves)


def psf_slices(n_rows, buckets, npix, cus):
    """The ray slices prt_frame_psf picks: they follow n_rows of the whole frame, not the rays selected."""
    tiles = -(-npix // K.kPsfTile)
    slices = (4 * cus + tiles * buckets - 1) // (tiles * buckets)
    slices = min(slices, max(1, n_rows // (buckets * K.kPsfMinSlice)))
    slices = min(slices, K.kPsfSlabBytes // (buckets * npix * 16))
    return max(1, min(slices, K.kPsfMaxSlices))


def slice_range(n, slices, k):
    """psf_slice / k_mtf_sum: the rays [lo, hi) of slice k of a bucket of n rays; lo may lie past hi."""
    per = -(-n // slices)
    lo = k * per
    return lo, min(lo + per, n)


def mtf_slices(count, n_groups, n_out):
    cap = max(1, min(K.kMtfMaxSlices, K.kMtfSlabBytes // (n_groups * n_out * 16)))
    return min(max(-(-count // K.kMtfMinSlice), 1), cap)


def mtf_lanes(n_out):
    return 4 if n_out <= K.kMtfOut * K.kMtfBlock // 4 else (2 if n_out <= K.kMtfOut * K.kMtfBlock // 2 else 1)


def mtf_tile(n_out):
    """Outputs of a k_mtf_sum workgroup: threads * kMtfOut."""
    return K.kMtfOut * (K.kMtfBlock // mtf_lanes(n_out))


# ---- shared pieces --------------------------------------------------------------------------------------------------------
def ulp(x):
    return float(np.spacing(np.float64(abs(x))))


def phasor(cycles):
    """(cos, sin)(2 pi cycles) of longdouble cycles, the phase reduced to a fraction of a turn first."""
    frac = cycles - np.rint(cycles)
    angle = TWO_PI * frac
    return np.cos(angle), np.sin(angle)


def _chunks(n_items, n_rays, budget=150_000):
    step = max(1, budget // max(1, n_rays))
    return [(at, min(at + step, n_items)) for at in range(0, n_items, step)]


# ---- the Huygens PSF and the Strehl ratio -----------------------------------------------------------------------------------
def inverse_wavelength(wavelength_um, unit):
    """1 / lambda_w as prt_frame_psf forms it in fp64: 1.0 / (w / world_unit_um)."""
    return 1.0 / (np.float64(wavelength_um) / np.float64(unit))


def huygens_amplitude(p1, p2, opd, a, radius, s, uu, vv, offset=None):
    """sum_r a_r exp(2 pi i (OPD_r + d_r - R) s) at the points (uu, vv): (re, im), longdouble, not yet over lambda_w.
    d - R is formed without cancellation as (u^2 + v^2 - 2 (u p1 + v p2)) / (d + R)."""
    n = len(p1)
    re, im = np.zeros(len(uu), dtype=LD), np.zeros(len(uu), dtype=LD)
    if n == 0:
        return re, im
    P1, P2, O, A = (np.asarray(x, dtype=np.float64).astype(LD)[None, :] for x in (p1, p2, opd, a))
    R, S = LD(radius), LD(s)
    extra = LD(0) if offset is None else np.asarray(offset, dtype=LD)[None, :]
    for lo, hi in _chunks(len(uu), n):
        u, v = (np.asarray(x[lo:hi], dtype=np.float64).astype(LD)[:, None] for x in (uu, vv))
        q = u * u + v * v - 2 * (u * P1 + v * P2)
        d = np.sqrt(R * R + q)
        c, sn = phasor((O + q / (d + R)) * S + extra)
        re[lo:hi], im[lo:hi] = (A * c).sum(axis=1), (A * sn).sum(axis=1)
    return re, im


def psf_epsilon(radius, s, rho, opd_max, uu, vv):
    """eps of |U~ - U| <= eps sum a, per point: the module docstring's count, term by term."""
    uu, vv = np.asarray(uu, dtype=float), np.asarray(vv, dtype=float)
    r = np.hypot(uu, vv)
    k0, cross = radius * radius + r * r, 2.0 * rho * r
    assert np.all(cross < 0.5 * k0), "a pixel as far out as the reference sphere's radius: not what the budget counts"
    kappa = (k0 + cross) / (k0 - cross)
    largest = np.maximum(np.sqrt(k0 + cross), radius + opd_max) * s
    roundings = 2.0 + 2.5 * kappa + 2.0 + 1.0 + 3.0 * r * (r + rho) / k0
    return EPS_TRIG + 2 * math.pi * F32_TURN + 2 * math.pi * roundings * np.spacing(largest)


def psf_bound(intensity, share, eps):
    """|I~ - I| <= 2 eps sqrt(I f) + eps^2 f; intensity the reference's, share f of the group's denominator."""
    return 2.0 * eps * np.sqrt(np.asarray(intensity, dtype=float) * share) + eps * eps * share


def strehl_eta(radius, s, opd_max, rays, slices):
    depth = -(-(-(-max(rays, 1) // slices)) // K.kPsfBlock) + int(math.log2(K.kPsfBlock)) + slices
    return 2 * math.pi * 2.0 * ulp((radius + opd_max) * s) + (4 + 1 + depth) * U64, depth


def psf_reference(inp, uu=None, vv=None, select=None, offset=None, slices=1):
    """The definitions of include/prt.h on ``inp`` (see psf_inputs): a namespace of image_by_wavelength (G, L, nx, ny)
    and image (G, nx, ny) in longdouble, strehl (G), n_rays / n_missed (G, L), and the budget evaluated on them:
    bound_by_wavelength, bound (of image) and strehl_bound.  A group without rays is NaN.  For the mutations:
    uu / vv replace the flattened pixel centres, select(b, n) returns the indices of bucket b's rays that are summed,
    offset(b, n) turns added to the phases."""
    nx, ny = len(inp.u), len(inp.v)
    if uu is None:
        uu, vv = (x.ravel() for x in np.meshgrid(inp.u, inp.v, indexing="ij"))
    G, L = inp.n_groups, len(inp.wavelengths)
    image = np.full((G, L, nx * ny), np.nan, dtype=LD)
    bound = np.full((G, L, nx * ny), np.nan)
    strehl, strehl_bound = np.full(G, np.nan, dtype=LD), np.full(G, np.nan)
    n_rays, n_missed = np.zeros((G, L), dtype=np.int64), np.zeros((G, L), dtype=np.int64)
    usable = np.isfinite(inp.opd) & np.all(np.isfinite(inp.pupil), axis=1) & (inp.weight >= 0) & np.isfinite(inp.weight)
    for g in range(G):
        parts = []
        for k, lam in enumerate(inp.wavelengths):
            m = (inp.group == g) & (inp.wavelength == lam)
            n_missed[g, k] = int((m & ~usable).sum())
            m &= usable
            n_rays[g, k] = int(m.sum())
            s = inverse_wavelength(lam, inp.unit)
            rho = inp.rho[g]
            ray = dict(p1=inp.pupil[m, 0] * rho, p2=inp.pupil[m, 1] * rho, opd=inp.opd[m], a=np.sqrt(inp.weight[m]))
            extra = None if offset is None else np.asarray(offset(g * L + k, int(m.sum())), dtype=LD)
            if select is not None:
                pick = np.asarray(select(g * L + k, int(m.sum())), dtype=np.int64)
                ray = {key: value[pick] for key, value in ray.items()}
                extra = None if extra is None else extra[pick]
            re, im = huygens_amplitude(ray["p1"], ray["p2"], ray["opd"], ray["a"], inp.radius[g], s, uu, vv, extra)
            c, sn = phasor(ray["opd"].astype(LD) * LD(s) + (0 if extra is None else extra))
            a = ray["a"].astype(LD)
            parts.append(SimpleNamespace(s=s, re=re, im=im, sum_a=a.sum(), wave=((a * c).sum(), (a * sn).sum()),
                                         opd_max=float(np.abs(ray["opd"]).max()) if len(a) else 0.0, rays=len(a)))
        den = sum((LD(p.s) * p.sum_a) ** 2 for p in parts)
        if not n_rays[g].sum() or not den > 0:
            continue
        strehl[g], strehl_bound[g] = 0, 0
        for k, p in enumerate(parts):
            share = float((LD(p.s) * p.sum_a) ** 2 / den)
            image[g, k] = LD(p.s) ** 2 * (p.re * p.re + p.im * p.im) / den
            eps = psf_epsilon(inp.radius[g], p.s, inp.rho[g], p.opd_max, uu, vv)
            bound[g, k] = psf_bound(image[g, k], share, eps)
            part = LD(p.s) ** 2 * (p.wave[0] ** 2 + p.wave[1] ** 2) / den
            eta, depth = strehl_eta(inp.radius[g], p.s, p.opd_max, p.rays, slices)
            strehl[g] += part
            strehl_bound[g] += 2 * eta * math.sqrt(float(part) * share) + eta * eta * share + (2 * depth + 10) * U64 * float(part)
    shape = (G, L, nx, ny)
    return SimpleNamespace(image_by_wavelength=image.reshape(shape), image=image.reshape(shape).sum(axis=1),
                           bound_by_wavelength=bound.reshape(shape), bound=bound.reshape(shape).sum(axis=1),
                           strehl=strehl, strehl_bound=strehl_bound, n_rays=n_rays, n_missed=n_missed)


def psf_inputs(group, wavelength, opd, pupil, weight, radius, rho, wavelengths, unit, u, v, n_groups):
    """The PSF's inputs, one entry per row the wavefront selected, in its order (fp64): group, wavelength (um), opd,
    pupil (n, 2), weight; per group radius and rho (the pupil radius); the distinct wavelengths, world_unit_um, and
    the pixel centres u (nx) and v (ny)."""
    f = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731
    return SimpleNamespace(group=np.asarray(group, dtype=np.int64), wavelength=f(wavelength), opd=f(opd),
                           pupil=f(pupil).reshape(-1, 2), weight=f(weight), radius=f(radius), rho=f(rho),
                           wavelengths=f(wavelengths), unit=float(unit), u=f(u), v=f(v), n_groups=int(n_groups))


def psf_inputs_from(frame, got, surface, rays_per_source=None, n_groups=1, weights="intensity"):
    """psf_inputs of a host frame (n, 15) and the PSF the device returned for it: the wavefront's own opd, pupil, radius
    and pupil_radius, the frame's columns, PSF.u / PSF.v."""
    rows, groups = select_rows(frame, surface, rays_per_source, n_groups)
    wave = got.wavefront
    opd, pupil = wave.opd.cpu().numpy(), wave.pupil.cpu().numpy()
    assert len(opd) == len(rows)
    weight = np.ones(len(rows)) if weights is None else rows[:, COLUMNS.index(weights)]
    return psf_inputs(groups, rows[:, 2], opd, pupil, weight, wave.radius, wave.pupil_radius, got.wavelengths,
                      got.world_unit_um, got.u, got.v, n_groups)


# ---- the geometric OTF ----------------------------------------------------------------------------------------------------
def default_axes():
    return np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def frequency_table(frequencies, azimuths):
    """(kc, ks) (A, N) as prt_frame_mtf's host code forms them in fp64 (the same libm)."""
    nu = np.asarray(frequencies, dtype=np.float64)
    kc = np.array([nu * math.cos(az * (math.pi / 180.0)) for az in azimuths])
    ks = np.array([nu * math.sin(az * (math.pi / 180.0)) for az in azimuths])
    return kc, ks


def mtf_kept(q, u, w, axes):
    """The rows include/prt.h keeps: finite values, u.a != 0, finite slopes, a weight finite and >= 0."""
    a, e1, e2 = axes[:3], axes[3:6], axes[6:]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ua = u @ a
        s = np.stack([u @ e1, u @ e2], 1) / ua[:, None]
        return (np.all(np.isfinite(q), 1) & np.all(np.isfinite(u), 1) & np.isfinite(w) & (w >= 0) & (ua != 0)
                & np.all(np.isfinite(s), 1))


def centroid(q, w):
    """The weighted centroid in longdouble, and the bound its fp64 sum in chunks and trees is held to, per axis."""
    W, Q = w.astype(LD), q.astype(LD)
    c = (W[:, None] * Q).sum(axis=0) / W.sum()
    depth = K.kMtfChunk // K.kMtfBlock + int(math.log2(K.kMtfBlock)) + -(-len(w) // K.kMtfChunk)
    scale = (W[:, None] * np.abs(Q)).sum(axis=0) / W.sum()
    return c, (2 * (depth + 2) * U64 * scale).astype(float)


def otf_bound(mean_terms):
    """eps_hw + (2 pi 2^-25)^2 / 2 + 2 pi K_OTF u T, T the weighted mean of the phase terms' magnitudes."""
    return EPS_TRIG + (2 * math.pi * F32_TURN) ** 2 / 2 + 2 * math.pi * K_OTF * U64 * mean_terms


def mtf_reference(q, u, w, group, n_groups, frequencies, azimuths=(0.0, 90.0), focus=(0.0,), axes=None, centre=None,
                  select=None, offset=0.0, float_turn=False):
    """OTF_g(delta, theta, nu) of include/prt.h from the selected rows (q, u (n, 3), w, group, in row order): a namespace
    of otf (G, F, A, N) complex of longdouble parts (re, im), n_rays, n_missed, centre (the one used: ``centre`` (G, 3)
    fp64, or the longdouble centroid), centroid and centre_bound, sum_weights, bound and phase_terms (T) (G, F, A, N).  For the mutations: select(g, n)
    returns the indices of group g's rays that are summed, offset is added to every phase in turns, float_turn rounds
    the reduced turn to float as the kernel's conversion does and puts nothing back."""
    axes = default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    q, u, w = (np.asarray(x, dtype=np.float64) for x in (q, u, w))
    kept = mtf_kept(q, u, w, axes)
    a, e1, e2 = (axes[k:k + 3].astype(LD) for k in (0, 3, 6))
    kc, ks = frequency_table(frequencies, azimuths)
    planes = np.asarray(focus, dtype=np.float64)
    F, (A, N) = len(planes), kc.shape
    re, im = np.full((n_groups, F, A, N), np.nan, dtype=LD), np.full((n_groups, F, A, N), np.nan, dtype=LD)
    bound, phase_terms = np.full((n_groups, F, A, N), np.nan), np.full((n_groups, F, A, N), np.nan)
    used, missed = np.zeros(n_groups, dtype=np.int64), np.zeros(n_groups, dtype=np.int64)
    centres, centre_bound = np.full((n_groups, 3), np.nan, dtype=LD), np.full((n_groups, 3), np.nan)
    centroids = np.full((n_groups, 3), np.nan, dtype=LD)
    sums = np.full(n_groups, np.nan, dtype=LD)
    for g in range(n_groups):
        m = kept & (group == g)
        used[g], missed[g] = int(m.sum()), int(((group == g) & ~kept).sum())
        if not used[g]:
            continue
        Q, Uv, W = q[m].astype(LD), u[m].astype(LD), w[m].astype(LD)
        own, centre_bound[g] = centroid(q[m], w[m])
        centroids[g] = own
        c = own if centre is None else np.asarray(centre[g], dtype=np.float64).astype(LD)
        centres[g] = c
        d = Q - c
        ua = Uv @ a
        s1, s2 = (Uv @ e1) / ua, (Uv @ e2) / ua
        da = d @ a
        p1, p2 = d @ e1 - s1 * da, d @ e2 - s2 * da
        # the magnitudes the budget is stated in
        mag = lambda x, e: (np.abs(x) * np.abs(e)).sum(axis=1)  # noqa: E731
        S1, S2 = ((mag(Uv, e) + np.abs(s) * mag(Uv, a)) / np.abs(ua) for e, s in ((e1, s1), (e2, s2)))
        P1, P2 = mag(d, e1) + S1 * mag(d, a), mag(d, e2) + S2 * mag(d, a)
        if select is not None:
            pick = np.asarray(select(g, int(used[g])), dtype=np.int64)
            p1, p2, s1, s2, W, P1, P2, S1, S2 = (x[pick] for x in (p1, p2, s1, s2, W, P1, P2, S1, S2))
        total = W.sum()
        sums[g] = total
        if not total > 0:
            continue
        mean = lambda x: float((W * x).sum() / total)  # noqa: E731
        KC, KS = kc.astype(LD).reshape(-1, 1), ks.astype(LD).reshape(-1, 1)
        for f, delta in enumerate(planes):
            x1, x2 = p1 + LD(delta) * s1, p2 + LD(delta) * s2
            for lo, hi in _chunks(A * N, len(W)):
                cycles = KC[lo:hi] * x1[None, :] + KS[lo:hi] * x2[None, :] + LD(offset)
                if float_turn:
                    cycles = (cycles - np.floor(cycles)).astype(np.float64).astype(np.float32).astype(LD)
                cs, sn = phasor(cycles)
                re[g, f].reshape(-1)[lo:hi] = (W * cs).sum(axis=1) / total
                im[g, f].reshape(-1)[lo:hi] = -(W * sn).sum(axis=1) / total
            terms = (np.abs(kc) * mean(P1) + np.abs(ks) * mean(P2)
                     + abs(delta) * (np.abs(kc) * mean(S1) + np.abs(ks) * mean(S2)))
            phase_terms[g, f], bound[g, f] = terms, otf_bound(terms)
    return SimpleNamespace(re=re, im=im, otf=re.astype(np.float64) + 1j * im.astype(np.float64), bound=bound,
                           n_rays=used, n_missed=missed, centre=centres, centroid=centroids, centre_bound=centre_bound,
                           sum_weights=sums, phase_terms=phase_terms)


def otf_deviation(got, ref):
    """|got - reference| per output, the difference taken in longdouble."""
    return np.hypot(np.real(got).astype(LD) - ref.re, np.imag(got).astype(LD) - ref.im).astype(np.float64)


def select_rows(frame, surface, rays_per_source, n_groups):
    """The rows the passes select (at ``surface``, in a group), in row order, and their groups."""
    rows = frame if surface is None else frame[frame[:, 5] == surface]
    groups = np.floor(rows[:, 4] / rays_per_source) if rays_per_source else np.zeros(len(rows))
    keep = (groups >= 0) & (groups < n_groups)
    return rows[keep], groups[keep].astype(np.int64)


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
SURFACE, ELSEWHERE = 5.0, 2.0
COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")


def vogel(n, radius=1.0):
    k = np.arange(n) + 0.5
    r, t = radius * np.sqrt(k / n), k * (math.pi * (3.0 - math.sqrt(5.0)))
    return r * np.cos(t), r * np.sin(t)


def psf_case(counts, *, radius=10.0, rho=0.5, unit=1000.0, wavelengths=(0.55,), pixels=(9, 7), pixel_size=None,
             centre=(0.0, 0.0), opd_waves=0.3, weights=None, filler=0, pupil=None, opd=None, seed=1):
    """A one-generation frame whose wavefront is known in advance, and that wavefront.  counts (G, L): the rays of each
    (group, wavelength) bucket; filler: rows at another surface, shuffled among them (n_rows, and with it the slices,
    grow; the rays selected do not).  A ray leaves E on the sphere (P = 0, R) towards P and ends a little past it; its
    segment starts L0 + o before E, so its OPD about the sphere is o less the group's weighted mean.  Returns a namespace
    of frame (n, 15), options for DeviceFrame.psf, and ``inputs(u, v)`` -> psf_inputs of the designed wavefront, which
    the device's own agrees with to rounding (the GPU tests take the device's)."""
    rng = np.random.default_rng(seed)
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    G, L = counts.shape
    assert L == len(wavelengths)
    per_source = int(counts.sum(axis=1).max()) + 7
    bucket = np.concatenate([np.full(c, b) for b, c in enumerate(counts.ravel())]).astype(np.int64)
    n = len(bucket)
    ray_row = rng.permutation(n + filler)[:n]  # ray r (listed bucket by bucket) lies in row ray_row[r]
    g, k = bucket // L, bucket % L
    if pupil is None:
        r, t = rho * np.sqrt(rng.random(n)), rng.random(n) * 2 * math.pi
        y, z = r * np.cos(t), r * np.sin(t)
    else:
        y, z = (np.asarray(x, dtype=float) for x in pupil)
    lam = np.asarray(wavelengths, dtype=float)[k]
    if opd is None:  # (defocus, coma and noise, both signs, in waves of the shortest wavelength)
        x, yy = y / rho, z / rho
        scale = opd_waves * min(wavelengths) / unit
        opd = scale * (2 * (x * x + yy * yy) - 1 + 0.8 * x * (x * x + yy * yy) + 0.3 * rng.normal(size=n))
    w = 50 + 50 * rng.random(n) if weights is None else np.asarray(weights(rng, n), dtype=float)
    e = np.stack([-np.sqrt(radius * radius - y * y - z * z), y, z], 1)
    towards = -e / radius
    past = 0.02 * radius
    start, end = e - towards * (0.1 * radius + 1.0 + np.asarray(opd))[:, None], towards * past
    rows = np.zeros((n + filler, 15))
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 5] = 1.0, wavelengths[0], 1.0, ELSEWHERE
    rows[:, 4] = G * per_source + np.arange(n + filler)
    rows[:, 9], rows[:, 12] = 1.0, 1.0
    rows[ray_row, 1], rows[ray_row, 2], rows[ray_row, 5] = w, lam, SURFACE
    rows[ray_row, 6:9], rows[ray_row, 9:12], rows[ray_row, 12:15] = start, end, towards
    for group in range(G):
        mine = ray_row[g == group]
        rows[mine, 4] = group * per_source + np.argsort(np.argsort(mine))
    in_order = np.argsort(ray_row)  # (the rays in the wavefront's order: row order)
    options = dict(world_unit_um=unit, pixels=pixels, centre=centre, reference=(0.0, 0.0, 0.0), radius=radius,
                   rays_per_source=per_source, n_groups=G)
    if pixel_size is not None:
        options["pixel_size"] = pixel_size

    def inputs(u, v):
        go, gy, gz, gw, gg, gl = (x[in_order] for x in (np.asarray(opd, dtype=float), y, z, w, g, lam))
        extent = np.array([np.hypot(gy[gg == i], gz[gg == i]).max() if (gg == i).any() else np.nan for i in range(G)])
        mean = np.array([(gw[gg == i] * go[gg == i]).sum() / gw[gg == i].sum() if (gg == i).any() else 0.0
                         for i in range(G)])
        pupil_points = np.stack([gy, gz], 1) / extent[gg][:, None]
        return psf_inputs(gg, gl, go - mean[gg], pupil_points, gw, np.full(G, radius), extent, np.unique(lam), unit, u, v, G)

    return SimpleNamespace(frame=rows, options=options, inputs=inputs, counts=counts, n_rows=n + filler)


def pixel_centres(pixels, pixel_size, centre):
    """PSF.u / PSF.v."""
    (nx, ny), (du, dv) = pixels, np.broadcast_to(np.asarray(pixel_size, dtype=float), (2,))
    return centre[0] + (np.arange(nx) - 0.5 * (nx - 1)) * du, centre[1] + (np.arange(ny) - 0.5 * (ny - 1)) * dv


def mtf_case(counts, *, spread=2e-3, slope=0.05, offset=(0.0, 0.0, 0.0), filler=0, left_out=0, axis=None, seed=2):
    """A frame whose rows at SURFACE end near ``offset`` with directions about the axis: counts[g] rays per group in row
    order, shuffled with ``filler`` rows of another surface; ``left_out`` rows per group that the pass must count and
    leave out (a NaN end point, a direction perpendicular to the axis, a negative weight)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    G = len(counts)
    per_source = int(counts.max()) + left_out + 5
    group = np.concatenate([np.full(c + left_out, k) for k, c in enumerate(counts)]).astype(np.int64)
    n = len(group)
    a = np.array([1.0, 0.0, 0.0]) if axis is None else np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    rows = np.zeros((n + filler, 15))
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 5] = 1.0, 0.55, 1.0, ELSEWHERE
    rows[:, 4] = G * per_source + np.arange(n + filler)
    rows[:, 12] = 1.0
    at = np.sort(rng.permutation(n + filler)[:n])
    group = group[rng.permutation(n)]
    rows[at, 5] = SURFACE
    rows[at, 1] = 50 + 50 * rng.random(n)
    rows[at, 9:12] = np.asarray(offset) + rng.normal(0, spread, (n, 3)) * (1 + 3 * group[:, None] / max(G, 1))
    rows[at, 12:15] = (a + rng.normal(0, slope, (n, 3))) * (0.5 + rng.random(n))[:, None]
    for k in range(G):
        mine = at[group == k]
        rows[mine, 4] = k * per_source + np.arange(len(mine))
        bad = mine[rng.permutation(len(mine))[:left_out]] if left_out else mine[:0]
        for j, row in enumerate(bad):
            if j % 3 == 0:
                rows[row, 10] = np.nan
            elif j % 3 == 1:
                assert a[2] == 0.0  # (z is then perpendicular to the axis exactly: u.a == 0 in fp64 too)
                rows[row, 12:15] = [0.0, 0.0, 1.0 + j]
            else:
                rows[row, 1] = -1.0
    return SimpleNamespace(frame=rows, rays_per_source=per_source, n_groups=G, axis=axis,
                           options=dict(rays_per_source=per_source, n_groups=G, **({} if axis is None else {"axis": axis})))


# ---- the families the GPU tests run, by name: the CPU test applies its mutations to the same inputs -----------------------
LAMBDA_F = 0.55e-3 * 10.0  # lambda_w F of the default psf_case: R = 10, rho = 0.5, 0.55 um in millimetres
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1)
PSF_GRIDS = ((1, 1), (31, 33), (32, 32), (25, 41), (1, 1025), (1025, 1), (64, 65))
# prt_frame_psf takes nx, ny in 1..1024, so a single row or column never leaves its first tile and (1, 1025) / (1025, 1)
# can only be refused; the nearest grids the contract allows: a whole tile as one row / one column, and 1026 pixels in
# two rows / two columns, where i (or j) changes in the middle of a tile and the second tile holds two pixels
PSF_GRIDS_WITHIN_THE_CAP = ((1, 1024), (1024, 1), (2, 513), (513, 2))
PSF_FILLER = 2 * 2048 + 100  # rows of another surface: n_rows, and so the slices, grow past the rays selected


def psf_tile_case(grid):
    return psf_case([[300]], pixels=grid, pixel_size=(0.31 * LAMBDA_F, 0.23 * LAMBDA_F),
                    centre=(0.9 * LAMBDA_F, -0.4 * LAMBDA_F), opd_waves=0.1, seed=11 + grid[0] + 3 * grid[1])


def psf_slice_case(n, filler):
    return psf_case([[n]], pixels=(9, 7), pixel_size=(0.4 * LAMBDA_F, 0.45 * LAMBDA_F), centre=(0.3 * LAMBDA_F, 0.0),
                    opd_waves=0.1, filler=filler, seed=100 + n)


def psf_sparse_case(counts):
    """About 20 000 rows of which 5 reach the surface: more slices than rays."""
    return psf_case(counts, wavelengths=(0.5, 0.6)[:np.shape(counts)[1]], pixels=(9, 7), pixel_size=0.4 * LAMBDA_F,
                    opd_waves=0.1, filler=20_000 - int(np.sum(counts)), seed=5)


def psf_bucket_case():
    """Two groups x three wavelengths holding 1 / 300 / 4000 rays and none at all."""
    return psf_case([[1, 300, 4000], [0, 0, 0]], wavelengths=(0.45, 0.55, 0.65), pixels=(9, 7), pixel_size=0.4 * LAMBDA_F,
                    centre=(0.0, 0.2 * LAMBDA_F), opd_waves=0.1, filler=30_000, seed=6)


def psf_antiphase_case():
    """Two rays in exact antiphase at the centre pixel (micrometres, 0.5 um: 1 / lambda_w = 2 exactly)."""
    return psf_case([[2]], radius=1e4, rho=500.0, unit=1.0, wavelengths=(0.5,), pixels=(3, 3), pixel_size=2.0,
                    pupil=([300.0, -300.0], [0.0, 0.0]), opd=[0.125, -0.125], weights=lambda rng, n: np.full(n, 64.0))


def psf_airy_case():
    """A 4096-ray Vogel disk without aberration, along a line through its first three minima (1.22, 2.23, 3.24
    lambda F)."""
    return psf_case([[4096]], pixels=(513, 1), pixel_size=3.6 * LAMBDA_F / 256, pupil=vogel(4096, 0.5), opd=np.zeros(4096),
                    weights=lambda rng, n: np.ones(n))


def _wide_weights(rng, n):
    w = 10.0 ** rng.uniform(-12, 6, n)
    w[::7] = 0.0
    w[1], w[2] = 1e-12, 1e6
    return w


def psf_large_phase_case(micrometres):
    """R / lambda_w = 5e6 cycles, pixels out to 0.3 R, OPD of both signs, weights from 1e-12 to 1e6 and exact zeros."""
    scale = 1000.0 if micrometres else 1.0
    return psf_case([[500]], radius=2000.0 * scale, rho=100.0 * scale, unit=1.0 if micrometres else 1000.0,
                    wavelengths=(0.4,), pixels=(9, 7), pixel_size=(106.0 * scale, 141.0 * scale),
                    centre=(3.0 * scale, -2.0 * scale), opd_waves=2.0, weights=_wide_weights, seed=9)


SWEEP_TURNS, SWEEP_CHUNK = 65536, 4096  # prt_frame_mtf takes 4096 frequencies a call: the sweep is 16 calls


def sweep_turns():
    """65 536 turns for the one-ray sweep: float turns (0, the quarter turns and four neighbours each side, 1 - 2^-24,
    powers of two, the multiples of 2^-13, the turn of EPS_HW_MEASURED, random ones) and fp64 turns that round in the
    conversion (1 - 2^-30 rounds up to 1.0f)."""
    rng = np.random.default_rng(20)
    near = []
    for quarter in (0.0, 0.25, 0.5, 0.75, 1.0):
        lo = hi = np.float32(quarter)
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            near += [float(lo), float(hi)]
    special = [0.0, 0.25, 0.5, 0.75, 1 - 2.0 ** -24, EPS_HW_TURN] + [x for x in near if 0 <= x < 1]
    special += [2.0 ** -k for k in range(1, 40)]
    rounded = [1 - 2.0 ** -30, 1 - 2.0 ** -25, 1 - 2.0 ** -26, 0.25 + 2.0 ** -27, 0.5 - 2.0 ** -27, 0.75 + 2.0 ** -40]
    fixed = np.unique(np.concatenate([special, rounded, np.arange(8192) / 8192.0]))
    random = rng.random(SWEEP_TURNS - len(fixed), dtype=np.float32).astype(np.float64)
    return np.concatenate([fixed, random])


def mtf_single_ray(p, slope=0.0):
    """One ray that ends at (0, p, 0) with direction (1, slope, 0): about reference=(0, 0, 0) p1 = p and s1 = slope."""
    rows = np.zeros((1, 15))
    rows[0, 1], rows[0, 5], rows[0, 10], rows[0, 12], rows[0, 13] = 1.0, SURFACE, p, 1.0, slope
    return rows


# about reference=(0.3, -3, 4) the rays lie near p = (3, -4): five units away, along the last of these azimuths
FAR_REFERENCE, FAR_AZIMUTHS = (0.3, -3.0, 4.0), (0.0, 90.0, 33.0, math.degrees(math.atan2(-4.0, 3.0)) + 360.0)
MTF_OUTPUTS = {"lanes4": dict(frequencies=np.linspace(0.0, 300.0, 6), azimuths=(0.0, 90.0), focus=(0.0, 0.05)),
               "lanes2": dict(frequencies=np.linspace(0.0, 300.0, 25), azimuths=tuple(15.0 * k for k in range(12))),
               "lanes1": dict(frequencies=np.linspace(0.0, 300.0, 40), azimuths=tuple(14.0 * k for k in range(13)))}
# planes x azimuths x frequencies: one below, on and one above a workgroup's tile for lanes = 4 (256; 257 selects
# lanes = 2), lanes = 2 (512; 513 selects lanes = 1) and lanes = 1 (1024)
MTF_OUTPUT_COUNTS = ((3, 5, 17), (4, 4, 16), (1, 1, 257), (7, 1, 73), (8, 4, 16), (3, 9, 19), (3, 11, 31), (4, 16, 16),
                     (5, 5, 41))


def mtf_output_options(shape):
    planes, azimuths, frequencies = shape
    return dict(focus=np.linspace(-0.04, 0.06, planes) if planes > 1 else (0.0,),
                azimuths=tuple(np.linspace(0.0, 170.0, azimuths)), frequencies=np.linspace(0.0, 400.0, frequencies))
