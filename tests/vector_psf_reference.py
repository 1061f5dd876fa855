"""An extended-precision reference of the polarised Huygens PSF (prt_frame_vector_psf: the definitions of
include/prt.h) and the error budget k_vpsf_huygens, k_vpsf_strehl and k_vpsf_fold are held to.  It builds on
tests/diffraction_reference.py (imported, not edited): the same inputs, the same 80-bit np.longdouble, the same eps.

What counts as an input: what psf_inputs holds (the wavefront's opd, pupil, radius and pupil_radius, the frame's weight
and wavelength columns, 1 / lambda_w as the library forms it, the pixel centres), the fields of the selected rows as
the Fresnel holds them (fp64 or complex128, world components) and the nine axes.  The component amplitudes
c_k = sqrt(w) E . e_k are formed here in longdouble; the device forms them in fp64 (a square root, a product and a dot
product of three terms: under 6 u of |A|), which falls under EPS_TRIG's margin like the accumulation does.

The field.  huygens_amplitude is linear in ``a``: with c_k = x + i y, U_k = H(x) + i H(y), two calls per component, H the
complex sum (re, im) that huygens_amplitude returns.  A component that is 0 on every ray is not summed.

The budget (derived, not measured).  u, ulp, EPS_TRIG and psf_epsilon's count of roundings are diffraction_reference's.
  * k_vpsf_huygens computes the phase with the function k_psf_huygens calls (psf_phase: the fma chain, psf_sqrt,
    v_fract_f64, then v_cos_f32 / v_sin_f32 on the float turn), so a ray's phasor is within eps = psf_epsilon(...) of the definition's and
    |U~_k - U_k| <= eps sum_r |c_{r,k}| / lambda, |c| the complex modulus: (x + i y)(cs + i sn) moves by |c| times the
    phasor's error.  The complex multiply-add's four fmas are four roundings of magnitude |c|, a few u: under EPS_TRIG's
    margin (eps_hw itself, 1.4e-7), as diffraction_reference's docstring argues for the accumulation.
  * With D the group's denominator, a_k = sum_r |c_{r,k}| / lambda, I_k = |U_k|^2 / D and f_k = a_k^2 / D:
    |U~_k|^2 / D moves by at most 2 eps sqrt(I_k f_k) + eps^2 f_k = b_k.
  * S0 = I_1 + I_2 and S1 = I_1 - I_2 move by at most b_1 + b_2; axial by b_3; the image S0 + axial by b_1 + b_2 + b_3.
  * conj(U~_1) U~_2 - conj(U_1) U_2 = conj(d_1) U_2 + conj(U_1) d_2 + conj(d_1) d_2 with |d_k| <= eps a_k, so S2 and S3
    (twice its real and imaginary part, over D) move by at most 2 (eps (a_1 |U_2| + a_2 |U_1|) + eps^2 a_1 a_2) / D.
  * States are averaged: the bounds are averaged with them.  Wavelengths add: their bounds add.
  * Strehl: the six sums are k_psf_strehl's with c_k for a, so strehl_eta applies per component: with
    part_k = |sum_r c_k exp(2 pi i OPD / lambda)|^2 / lambda^2 / D the ratio moves by
    sum over buckets, states (mean) and components of 2 eta sqrt(part_k f_k) + eta^2 f_k + (2 depth + 10) u part_k.
    strehl_apodized = numerator / D' with D' = mean_s sum_l (sum_r |A_r| / lambda)^2: the numerator's bound scaled by
    D / D', and D' itself, whose terms sqrt(w) sqrt(|E|^2) carry six more roundings: (2 depth + 16) u of the ratio.
  * throughput = sum_r w |E|^2 / sum_r w, formed as sqrt(w)^2 |E|^2 and sqrt(w)^2: under 8 roundings a term and depth
    additions in either sum, (2 depth + 16) u of the ratio.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R

LD = R.LD
U64 = R.U64


def kernel_constants():
    """diffraction_reference's constants and the static const ints of prt_vector_psf.hpp (kVpsfPix, kVpsfTile, ...)."""
    found = dict(vars(R.K))
    text = open(os.path.join(R.ROOT, "pyrayt_amd", "csrc", "prt_vector_psf.hpp")).read()
    for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
        value = re.sub(r"(\d+)u\b", r"\1", value)
        try:
            found[key] = int(eval(value, {"__builtins__": {}}, dict(found)))  # (sums, products of earlier names)
        except (NameError, SyntaxError, TypeError):
            pass  # (not a plain constant)
    return SimpleNamespace(**found)


K = kernel_constants()
# vpsf_slices is a Python copy of lines of psf_plan (prt_psf.hpp) with the arguments prt_frame_vector_psf gives it, as
# diffraction_reference.psf_slices is with prt_frame_psf's: tests/test_host_vector_psf.py holds the copy to the headers'
# text
HOST_RULES = {
    "prt_psf.hpp": (
        "const int64_t tiles = (npix + tile_pixels - 1) / tile_pixels;",
        "int64_t slices = (4 * (int64_t)cus + tiles * buckets - 1) / (tiles * buckets);",
        "slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_items / (sort_buckets * kPsfMinSlice)));",
        "slices = std::min<int64_t>(slices, (int64_t)(kPsfSlabBytes / ((size_t)buckets * npix * pixel_bytes)));",
        "slices = std::max<int64_t>(1, std::min<int64_t>(slices, kPsfMaxSlices));"),
    "prt_vector_psf.hpp": (
        "const int64_t group_waves = (int64_t)n_groups * n_wavelengths, buckets = group_waves * n_states;",
        "psf_plan(cus, n_rows, group_waves, buckets, npix, kVpsfTile, kVpsfPixelBytes, kVpsfPixelBytes, VPSF_SUMS);"),
}


def vpsf_slices(n_rows, group_waves, n_states, npix, cus):
    """The ray slices prt_frame_vector_psf picks: they follow n_rows of the whole frame, not the rays selected."""
    buckets = group_waves * n_states
    tiles = -(-npix // K.kVpsfTile)
    slices = (4 * cus + tiles * buckets - 1) // (tiles * buckets)
    slices = min(slices, max(1, n_rows // (group_waves * K.kPsfMinSlice)))
    slices = min(slices, K.kPsfSlabBytes // (buckets * npix * K.kVpsfPixelBytes))
    return max(1, min(slices, K.kPsfMaxSlices))


def world_field(components, axes=None):
    """(n, 3) world components of a field given along (e1, e2, a)."""
    axes = R.default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    basis = np.stack([axes[3:6], axes[6:9], axes[0:3]])
    return np.asarray(components) @ basis


def _complex_amplitude(ray, c, radius, s, uu, vv, extra):
    """U = sum_r c_r exp(2 pi i phase_r) at the points, as (re, im) in longdouble: one call per part of c that is not 0."""
    re, im = np.zeros(len(uu), dtype=LD), np.zeros(len(uu), dtype=LD)
    if np.any(c.real != 0):
        x, y = R.huygens_amplitude(ray["p1"], ray["p2"], ray["opd"], c.real, radius, s, uu, vv, extra)
        re, im = re + x, im + y
    if np.any(c.imag != 0):
        x, y = R.huygens_amplitude(ray["p1"], ray["p2"], ray["opd"], c.imag, radius, s, uu, vv, extra)
        re, im = re - y, im + x
    return re, im


def vector_psf_reference(inp, field, n_states, axes=None, slices=1, offset=None):
    """The definitions of include/prt.h on ``inp`` (diffraction_reference.psf_inputs) and ``field``: (2, n, 3) or
    (1, n, 3), real or complex, the world components of Ea (and Eb) on the selected rows, in their order.  A namespace of
    stokes_by_wavelength (G, L, 5, nx, ny) -- S0, S1, S2, S3, axial -- and stokes (G, 5, nx, ny) in longdouble with
    bound_by_wavelength and bound; image_by_wavelength, image and their bounds; strehl, strehl_apodized, throughput (G)
    with strehl_bound, strehl_apodized_bound, throughput_bound; n_rays / n_missed (G, L).  A group without rays is NaN.
    offset(b, n): turns added to the phases of bucket b's rays (for the tests of the reference itself)."""
    axes = R.default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    basis = np.stack([axes[3:6], axes[6:9], axes[0:3]]).astype(LD)  # e1, e2, a
    field = np.asarray(field)[:n_states]
    assert field.shape == (n_states, len(inp.opd), 3)
    nx, ny = len(inp.u), len(inp.v)
    uu, vv = (x.ravel() for x in np.meshgrid(inp.u, inp.v, indexing="ij"))
    G, L, S = inp.n_groups, len(inp.wavelengths), n_states
    planes = np.full((G, L, 5, nx * ny), np.nan, dtype=LD)
    bound = np.full((G, L, 5, nx * ny), np.nan)
    image_bound = np.full((G, L, nx * ny), np.nan)
    out = {name: np.full(G, np.nan, dtype=LD) for name in ("strehl", "strehl_apodized", "throughput")}
    out_bound = {name: np.full(G, np.nan) for name in ("strehl", "strehl_apodized", "throughput")}
    n_rays, n_missed = np.zeros((G, L), dtype=np.int64), np.zeros((G, L), dtype=np.int64)
    usable = (np.isfinite(inp.opd) & np.all(np.isfinite(inp.pupil), axis=1) & (inp.weight >= 0) & np.isfinite(inp.weight)
              & np.all(np.isfinite(field.real) & np.isfinite(field.imag), axis=(0, 2)))
    for g in range(G):
        parts = []
        for k, lam in enumerate(inp.wavelengths):
            m = (inp.group == g) & (inp.wavelength == lam)
            n_missed[g, k] = int((m & ~usable).sum())
            m &= usable
            n_rays[g, k] = int(m.sum())
            s = R.inverse_wavelength(lam, inp.unit)
            rho = inp.rho[g]
            ray = dict(p1=inp.pupil[m, 0] * rho, p2=inp.pupil[m, 1] * rho, opd=inp.opd[m])
            extra = None if offset is None else np.asarray(offset(g * L + k, int(m.sum())), dtype=LD)
            root = np.sqrt(inp.weight[m].astype(LD))
            cs, sn = R.phasor(ray["opd"].astype(LD) * LD(s) + (0 if extra is None else extra))
            states = []
            for state in range(S):
                e = field[state][m]
                e_re, e_im = np.real(e).astype(LD), np.imag(e).astype(LD)
                c_re, c_im = root[:, None] * (e_re @ basis.T), root[:, None] * (e_im @ basis.T)
                modulus = np.sqrt(c_re * c_re + c_im * c_im)
                norm2 = (e_re * e_re + e_im * e_im).sum(axis=1)
                u, wave = [], []
                for comp in range(3):
                    c = c_re[:, comp].astype(np.float64) + 1j * c_im[:, comp].astype(np.float64)
                    # (huygens_amplitude takes fp64 amplitudes: the components rounded to fp64 are within u of c)
                    u.append(_complex_amplitude(ray, c, inp.radius[g], s, uu, vv, extra))
                    wave.append(((c_re[:, comp] * cs - c_im[:, comp] * sn).sum(),
                                 (c_re[:, comp] * sn + c_im[:, comp] * cs).sum()))
                states.append(SimpleNamespace(u=u, wave=wave, a=modulus.sum(axis=0), sum_norm=(root * np.sqrt(norm2)).sum(),
                                              passed=(root * root * norm2).sum()))
            parts.append(SimpleNamespace(s=s, states=states, sum_a=root.sum(), launched=(root * root).sum(),
                                         opd_max=float(np.abs(ray["opd"]).max()) if len(root) else 0.0, rays=len(root)))
        den = sum((LD(p.s) * p.sum_a) ** 2 for p in parts)
        if not n_rays[g].sum() or not den > 0:
            continue
        aligned = sum((LD(p.s) * st.sum_norm) ** 2 for p in parts for st in p.states) / S
        numerator, numerator_bound = LD(0), 0.0
        for k, p in enumerate(parts):
            s = LD(p.s)
            eps = R.psf_epsilon(inp.radius[g], p.s, inp.rho[g], p.opd_max, uu, vv)
            eta, depth = R.strehl_eta(inp.radius[g], p.s, p.opd_max, p.rays, slices)
            planes[g, k], bound[g, k], image_bound[g, k] = 0, 0, 0
            for st in p.states:
                a = [float(s * x) for x in st.a]                                    # a_k
                mod = [s * np.sqrt(re * re + im * im) for re, im in st.u]           # |U_k|
                inten = [x * x / den for x in mod]                                  # I_k
                b = [R.psf_bound(inten[c], a[c] * a[c] / float(den), eps) for c in range(3)]
                (r1, i1), (r2, i2) = st.u[0], st.u[1]
                cross = s * s * (r1 * r2 + i1 * i2) / den, s * s * (r1 * i2 - i1 * r2) / den
                for plane, value in enumerate((inten[0] + inten[1], inten[0] - inten[1], 2 * cross[0], 2 * cross[1],
                                               inten[2])):
                    planes[g, k, plane] += value / S
                mixed = 2 * (eps * (a[0] * mod[1].astype(float) + a[1] * mod[0].astype(float)) + eps * eps * a[0] * a[1]) / float(den)
                for plane, value in enumerate((b[0] + b[1], b[0] + b[1], mixed, mixed, b[2])):
                    bound[g, k, plane] += value / S
                image_bound[g, k] += (b[0] + b[1] + b[2]) / S
                for c in range(3):
                    part = s * s * (st.wave[c][0] ** 2 + st.wave[c][1] ** 2) / den
                    share = a[c] * a[c] / float(den)
                    numerator += part / S
                    numerator_bound += (2 * eta * math.sqrt(float(part) * share) + eta * eta * share
                                        + (2 * depth + 10) * U64 * float(part)) / S
        depth = max(R.strehl_eta(inp.radius[g], p.s, p.opd_max, p.rays, slices)[1] for p in parts)
        out["strehl"][g], out_bound["strehl"][g] = numerator, numerator_bound
        if aligned > 0:
            out["strehl_apodized"][g] = numerator * den / aligned
            out_bound["strehl_apodized"][g] = (numerator_bound * float(den / aligned)
                                               + (2 * depth + 16) * U64 * float(out["strehl_apodized"][g]))
        launched = sum(p.launched for p in parts)
        if launched > 0:
            out["throughput"][g] = sum(st.passed for p in parts for st in p.states) / S / launched
            out_bound["throughput"][g] = (2 * depth + 16) * U64 * float(out["throughput"][g])
    shape = (G, L, 5, nx, ny)
    planes, bound, image_bound = planes.reshape(shape), bound.reshape(shape), image_bound.reshape((G, L, nx, ny))
    return SimpleNamespace(
        stokes_by_wavelength=planes, bound_by_wavelength=bound, stokes=planes.sum(axis=1), bound=bound.sum(axis=1),
        image_by_wavelength=planes[:, :, 0] + planes[:, :, 4], image_bound_by_wavelength=image_bound,
        image=(planes[:, :, 0] + planes[:, :, 4]).sum(axis=1), image_bound=image_bound.sum(axis=1),
        strehl=out["strehl"], strehl_bound=out_bound["strehl"], strehl_apodized=out["strehl_apodized"],
        strehl_apodized_bound=out_bound["strehl_apodized"], throughput=out["throughput"],
        throughput_bound=out_bound["throughput"], n_rays=n_rays, n_missed=n_missed)


def selected_rows(frame, surface, rays_per_source, n_groups):
    """The indices of the rows the passes select (at ``surface``, in a group), in row order: what
    diffraction_reference.select_rows keeps, as positions in the frame (the field's columns)."""
    at = np.arange(len(frame)) if surface is None else np.nonzero(frame[:, 5] == surface)[0]
    groups = np.floor(frame[at, 4] / rays_per_source) if rays_per_source else np.zeros(len(at))
    return at[(groups >= 0) & (groups < n_groups)]


def field_of_rows(field, rows):
    """(2, n, 3) from the Fresnel's (6, n_rows) field (numpy) at the given rows: Ea and Eb."""
    return np.stack([field[0:3, rows].T, field[3:6, rows].T])


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
def random_field(n_rows, complex_field, seed):
    """(6, n_rows): random fields of magnitude about 1, Ea then Eb by component, as a Fresnel holds them."""
    rng = np.random.default_rng(seed)
    field = rng.normal(0, 0.6, (6, n_rows))
    if complex_field:
        field = field + 1j * rng.normal(0, 0.6, (6, n_rows))
    return field


def constant_field(n_rows, vector):
    """(6, n_rows): the same real world vector in Ea on every row, Eb zero."""
    field = np.zeros((6, n_rows))
    field[0:3] = np.asarray(vector, dtype=float)[:, None]
    return field


def radial_case(n=4096):
    """A Vogel disk without aberration whose field points along the pupil radius, (cos theta, sin theta, 0) in
    (e1, e2, a): the components cancel at P, a dark centre, where a scalar sum of the same amplitudes gives 1.  The golden
    angle leaves |sum exp(i theta)| <= 1 / sin(phi / 2) < 1.08, so S0 at P is below 1.2 / n^2.  Returns the psf_case
    (5 x 5 pixels about P) and the (6, n_rows) field."""
    case = R.psf_case([[n]], pixels=(5, 5), pixel_size=0.5 * R.LAMBDA_F, pupil=R.vogel(n, 0.5), opd=np.zeros(n),
                      weights=lambda rng, count: np.ones(count))
    rows = selected_rows(case.frame, R.SURFACE, case.options["rays_per_source"], 1)
    # a row's segment starts on the line from P through its pupil point, beyond it: (y0, z0) has the pupil point's angle
    theta = np.arctan2(case.frame[rows, 8], case.frame[rows, 7])
    field = np.zeros((6, case.n_rows))
    field[0:3, rows] = world_field(np.stack([np.cos(theta), np.sin(theta), np.zeros(n)], 1)).T
    return case, field
