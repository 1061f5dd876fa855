"""An extended-precision reference of the diffraction PSF and the Strehl ratio through focus (prt_frame_psf_focus: the
definitions of include/prt.h) and the error budget the HIP kernels are held to.  It extends tests/diffraction_reference.py
(``R`` below), whose conventions, inputs, EPS_TRIG and ulp / u notation it takes as they are; nothing there is changed.

What counts as an input.  What ``R.psf_inputs`` takes -- with ``u`` / ``v`` the pixel centres as offsets from a plane's
centre (PSFScan.u / PSFScan.v) --, and the device's ``axial`` (p3 per selected row, the wavefront's order), ``focus``,
``line`` (G, 2) and ``centres`` (G, F, 2).  A pixel's place is centre + offset, formed in fp64; the Strehl point of plane
f is (delta t1, delta t2), each product formed in fp64 as k_psff_strehl forms it.

The definitions.  A pixel of plane delta lies at P + u e1 + v e2 + delta a and a ray's sphere point at
P + p1 e1 + p2 e2 + p3 a, so d^2 = R^2 + q with q = u^2 + v^2 + delta^2 - 2 (u p1 + v p2 + delta p3); the phase is
(OPD + d - R) / lambda_w with d - R = q / (d + R), free of cancellation.  At delta = 0 every expression below is
``R.psf_reference``'s, operation for operation, so the two agree exactly.  The chief line: t_i = (sum w p_i) / (sum w p3)
over the group's kept rays of all wavelengths -- the line through P and the weighted mean sphere point, which is where
the image of a displaced pupil goes (``test_the_chief_line_follows_the_image`` shows it on a closed form).

The budget (``focus_epsilon``), per pixel, in the notation of R's docstring: eps = eps_hw + 2 pi 2^-25 + 2 pi (k' ulp(M)
+ axial), with k0 = R^2 + r^2 + delta^2, r the pixel's distance from the axis line, cross = 2 (rho r + |delta| |p3|max),
kappa = (k0 + cross) / (k0 - cross), M = max(R + |OPD|, sqrt(k0 + cross)) / lambda_w, and k' counting, in ulp(M):
    c = (OPD - R) / lambda_w: 2, as before;
    d^2: k0 = R^2 + u^2 + v^2 + delta^2 is R's three roundings and two more for delta^2 (its product and its addition),
    and the chain fma(mu, p1, fma(mv, p2, fma(mw, p3, k0))) has three fmas where R's has two: 3 + 2 + 3 = 8 roundings, each
    relative to k0 + cross or less: 8 u kappa on d^2, half of it on d: 4 kappa (R: 2.5 kappa);
    psf_sqrt, faithful: 2;  fma(d, 1 / lambda_w, c): 1;
    the pixel's place: R's 3 r (r + rho) / k0 for one ulp of u and of v, and as much again for the ulp of a tracked
    centre, fma(delta, t, u0), which the pixel's place inherits.  Both are taken on the magnitudes that enter,
    rm = hypot(|cu| + |offset u|, |cv| + |offset v|) >= r, and over k0 - cross <= d^2: 6 rm (rm + rho) / (k0 - cross).
  axial = |delta| ulp(|p3|max) / (lambda_w d_min), d_min = sqrt(k0 - cross): one ulp of p3 moves d by |delta| / d of it.
  (The reference reads the device's own p3 and centres, so these two are not needed to compare the two; they are counted
  because the budget is also what include/prt.h promises a caller who has p3 and the centres from elsewhere.)
The domain: cross < 0.5 k0, as R asserts it, asserted here per pixel and plane: pixels and shifts well inside the
reference sphere.  With delta = 0 and a centre on the axis line the count is R's plus 1.5 kappa + 3 rm (rm + rho) / k0.

Strehl (``focus_eta``): fp64 sincospi of fma(d, 1 / lambda_w, c), d a correctly rounded square root of d^2 at the plane's
point.  eta = 2 pi ((2 + 5 kappa + 0.5) ulp(M) + axial) + (4 + 1 + depth) u: R's 2 for c and the fma; d^2 there has four
products, three additions and three fmas, 10 roundings relative to k0 + cross, 5 kappa ulps of d; the root half an ulp;
the rest is R's ``strehl_eta``.  The ratio moves as R's does.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R

LD = R.LD


def fused(a, b, c):
    """fma(a, b, c) in fp64, correctly rounded: what k_psff_centres forms."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def centres_of(line, focus, centre):
    """centres (G, F, 2): fma(delta_f, t_g, (u0, v0))."""
    line, focus = np.asarray(line, dtype=np.float64), np.asarray(focus, dtype=np.float64)
    out = np.empty((len(line), len(focus), 2))
    for g, t in enumerate(line):
        for f, delta in enumerate(focus):
            out[g, f] = fused(delta, t[0], centre[0]), fused(delta, t[1], centre[1])
    return out


def usable(inp, axial):
    """The rays prt_frame_psf keeps, with a finite p3."""
    return (np.isfinite(inp.opd) & np.all(np.isfinite(inp.pupil), axis=1) & (inp.weight >= 0) & np.isfinite(inp.weight)
            & np.isfinite(axial))


def chief_line(inp, axial, depth=None):
    """t (G, 2) in longdouble from the definition, and the bound the device's fp64 sums are held to, per component:
    w = a^2 with a = sqrt(w) rounded is within 1.5 u of w and the product w p one more, a term then passes through
    ``depth`` additions (the rays of a slice over kPsfBlock, the tree, the slices, the buckets), and the division
    rounds once: |t~ - t| <= (depth + 3) u (A_i + |t_i| A_3) / |S_3| + u |t_i|, A the sums of magnitudes."""
    axial = np.asarray(axial, dtype=np.float64)
    keep = usable(inp, axial)
    G = inp.n_groups
    line, bound = np.full((G, 2), np.nan, dtype=LD), np.full((G, 2), np.nan)
    for g in range(G):
        m = keep & (inp.group == g)
        if not m.any():
            continue
        w = inp.weight[m].astype(LD)
        p = [(inp.pupil[m, i] * inp.rho[g]).astype(LD) for i in (0, 1)] + [axial[m].astype(LD)]
        s = [(w * x).sum() for x in p]
        mag = [float((w * np.abs(x)).sum()) for x in p]
        d = (int(m.sum()) if depth is None else depth) + 3
        for i in (0, 1):
            line[g, i] = s[i] / s[2]
            t = abs(float(line[g, i]))
            bound[g, i] = d * R.U64 * (mag[i] + t * mag[2]) / abs(float(s[2])) + R.U64 * t
    return line, bound


def line_depth(rays, slices, buckets):
    """The additions a term of the chief line's sums passes through on the device."""
    return -(-(-(-max(rays, 1) // slices)) // R.K.kPsfBlock) + int(math.log2(R.K.kPsfBlock)) + slices + buckets


def focus_amplitude(p1, p2, p3, opd, a, radius, s, uu, vv, delta):
    """sum_r a_r exp(2 pi i (OPD_r + d_r - R) s) at the points (uu, vv) of plane delta: (re, im), longdouble."""
    n = len(p1)
    re, im = np.zeros(len(uu), dtype=LD), np.zeros(len(uu), dtype=LD)
    if n == 0:
        return re, im
    P1, P2, P3, O, A = (np.asarray(x, dtype=np.float64).astype(LD)[None, :] for x in (p1, p2, p3, opd, a))
    Rr, S, D = LD(radius), LD(s), LD(np.float64(delta))
    for lo, hi in R._chunks(len(uu), n):
        u, v = (np.asarray(x[lo:hi], dtype=np.float64).astype(LD)[:, None] for x in (uu, vv))
        q = u * u + v * v + D * D - 2 * (u * P1 + v * P2 + D * P3)
        d = np.sqrt(Rr * Rr + q)
        c, sn = R.phasor((O + q / (d + Rr)) * S)
        re[lo:hi], im[lo:hi] = (A * c).sum(axis=1), (A * sn).sum(axis=1)
    return re, im


def _geometry(radius, rho, p3_max, delta, uu, vv):
    r = np.hypot(uu, vv)
    k0 = radius * radius + r * r + delta * delta
    cross = 2.0 * (rho * r + abs(delta) * p3_max)
    assert np.all(cross < 0.5 * k0), "a pixel or a shift as far out as the reference sphere's radius: not what the budget counts"
    return r, k0, cross, (k0 + cross) / (k0 - cross)


def focus_epsilon(radius, s, rho, opd_max, p3_max, delta, uu, vv, um=None, vm=None):
    """eps of |U~ - U| <= eps sum a, per point of plane delta: the module docstring's count.  um / vm: the magnitudes
    |centre| + |offset| behind uu / vv (default: |uu|, |vv|)."""
    uu, vv = np.asarray(uu, dtype=float), np.asarray(vv, dtype=float)
    r, k0, cross, kappa = _geometry(radius, rho, p3_max, delta, uu, vv)
    rm = r if um is None else np.hypot(um, vm)
    largest = np.maximum(np.sqrt(k0 + cross), radius + opd_max) * s
    roundings = 2.0 + 4.0 * kappa + 2.0 + 1.0 + 6.0 * rm * (rm + rho) / (k0 - cross)
    axial = abs(delta) * R.ulp(p3_max) * s / np.sqrt(k0 - cross)
    return R.EPS_TRIG + 2 * math.pi * R.F32_TURN + 2 * math.pi * (roundings * np.spacing(largest) + axial)


def focus_eta(radius, s, rho, opd_max, p3_max, delta, us, vs, rays, slices):
    """eta of the Strehl sums at the plane's point (us, vs), and the depth of their additions."""
    _, depth = R.strehl_eta(radius, s, opd_max, rays, slices)
    r, k0, cross, kappa = _geometry(radius, rho, p3_max, delta, np.float64(us), np.float64(vs))
    largest = max(math.sqrt(float(k0 + cross)), radius + opd_max) * s
    axial = abs(delta) * R.ulp(p3_max) * s / math.sqrt(float(k0 - cross))
    return 2 * math.pi * ((2.0 + 5.0 * float(kappa) + 0.5) * R.ulp(largest) + axial) + (4 + 1 + depth) * R.U64, depth


def psf_focus_reference(inp, axial, focus, centres, line, select=None, slices=1, strehl_only=False):
    """The definitions on ``inp`` (R.psf_inputs, u / v offsets from a plane's centre): a namespace of
    image_by_wavelength (G, F, L, nx, ny) and image (G, F, nx, ny) in longdouble, strehl (G, F), n_rays / n_missed
    (G, L), and the budget evaluated on them: bound_by_wavelength, bound and strehl_bound.  A group without rays is
    NaN.  select(b, n): the indices of bucket b's rays that are summed (for the mutations)."""
    axial, focus = np.asarray(axial, dtype=np.float64), np.asarray(focus, dtype=np.float64)
    centres, line = np.asarray(centres, dtype=np.float64), np.asarray(line, dtype=np.float64)
    nx, ny = len(inp.u), len(inp.v)
    G, L, F = inp.n_groups, len(inp.wavelengths), len(focus)
    off_u, off_v = (x.ravel() for x in np.meshgrid(inp.u, inp.v, indexing="ij"))
    if strehl_only:
        off_u, off_v = off_u[:0], off_v[:0]
    npix = len(off_u)
    image = np.full((G, F, L, npix), np.nan, dtype=LD)
    bound = np.full((G, F, L, npix), np.nan)
    strehl, strehl_bound = np.full((G, F), np.nan, dtype=LD), np.full((G, F), np.nan)
    n_rays, n_missed = np.zeros((G, L), dtype=np.int64), np.zeros((G, L), dtype=np.int64)
    keep = usable(inp, axial)
    for g in range(G):
        rays = []
        for k, lam in enumerate(inp.wavelengths):
            m = (inp.group == g) & (inp.wavelength == lam)
            n_missed[g, k] = int((m & ~keep).sum())
            m &= keep
            n_rays[g, k] = int(m.sum())
            rho = inp.rho[g]
            ray = dict(p1=inp.pupil[m, 0] * rho, p2=inp.pupil[m, 1] * rho, p3=axial[m], opd=inp.opd[m],
                       a=np.sqrt(inp.weight[m]))
            if select is not None:
                pick = np.asarray(select(g * L + k, int(m.sum())), dtype=np.int64)
                ray = {key: value[pick] for key, value in ray.items()}
            rays.append((R.inverse_wavelength(lam, inp.unit), ray))
        den = sum((LD(s) * ray["a"].astype(LD).sum()) ** 2 for s, ray in rays)
        if not n_rays[g].sum() or not den > 0:
            continue
        for f, delta in enumerate(focus):
            cu, cv = centres[g, f]
            uu, vv = cu + off_u, cv + off_v
            um, vm = abs(cu) + np.abs(off_u), abs(cv) + np.abs(off_v)
            us, vs = np.float64(delta) * line[g, 0], np.float64(delta) * line[g, 1]
            strehl[g, f], strehl_bound[g, f] = 0, 0
            for k, (s, ray) in enumerate(rays):
                a = ray["a"].astype(LD)
                share = float((LD(s) * a.sum()) ** 2 / den)
                n = len(a)
                opd_max = float(np.abs(ray["opd"]).max()) if n else 0.0
                p3_max = float(np.abs(ray["p3"]).max()) if n else 0.0
                re, im = focus_amplitude(ray["p1"], ray["p2"], ray["p3"], ray["opd"], ray["a"], inp.radius[g], s, uu, vv,
                                         delta)
                image[g, f, k] = LD(s) ** 2 * (re * re + im * im) / den
                eps = focus_epsilon(inp.radius[g], s, inp.rho[g], opd_max, p3_max, delta, uu, vv, um, vm)
                bound[g, f, k] = R.psf_bound(image[g, f, k], share, eps)
                wre, wim = focus_amplitude(ray["p1"], ray["p2"], ray["p3"], ray["opd"], ray["a"], inp.radius[g], s,
                                           np.array([us]), np.array([vs]), delta)
                part = LD(s) ** 2 * (wre[0] ** 2 + wim[0] ** 2) / den
                eta, depth = focus_eta(inp.radius[g], s, inp.rho[g], opd_max, p3_max, delta, us, vs, n, slices)
                strehl[g, f] += part
                strehl_bound[g, f] += (2 * eta * math.sqrt(float(part) * share) + eta * eta * share
                                       + (2 * depth + 10) * R.U64 * float(part))
    shape = (G, F, L, nx, ny) if not strehl_only else (G, F, L, 0, 0)
    return SimpleNamespace(image_by_wavelength=image.reshape(shape), image=image.reshape(shape).sum(axis=2),
                           bound_by_wavelength=bound.reshape(shape), bound=bound.reshape(shape).sum(axis=2),
                           strehl=strehl, strehl_bound=strehl_bound, n_rays=n_rays, n_missed=n_missed)


def sphere_axial(inp, sign=-1.0):
    """p3 of inputs whose rays leave the sphere (P, R) along +a (``R.psf_case``): -sqrt(R^2 - p1^2 - p2^2), fp64."""
    p = inp.pupil * inp.rho[inp.group][:, None]
    return sign * np.sqrt(inp.radius[inp.group] ** 2 - p[:, 0] ** 2 - p[:, 1] ** 2)


def converging_opd(y, z, radius, target):
    """OPD of a perfect wave that leaves the sphere points E = (-sqrt(R^2 - y^2 - z^2), y, z) and converges at
    ``target`` (x, y, z about P): |E - P| - |E - target| = R - |E - target|, up to a constant."""
    e = np.stack([-np.sqrt(radius * radius - y * y - z * z), y, z], 1)
    return radius - np.linalg.norm(e - np.asarray(target, dtype=float)[None, :], axis=1)


# ---- the named cases the GPU tests run and the CPU test mutates -----------------------------------------------------------
DEPTH_OF_FOCUS = 2 * R.LAMBDA_F * 10.0  # 2 lambda F^2 of the default psf_case (F = 10): 0.11
SHIFTS = (-DEPTH_OF_FOCUS, 0.0, 0.64 * DEPTH_OF_FOCUS)  # about -0.11, 0.0 and +0.07
DELTA0 = 0.2


def converging_case(n=4096, delta0=DELTA0, pixels=(9, 7), **kw):
    """A perfect wave on a Vogel disk of n rays that converges at P + delta0 a."""
    y, z = R.vogel(n, 0.5)
    kw.setdefault("pixel_size", 0.4 * R.LAMBDA_F)
    return R.psf_case([[n]], pixels=pixels, pupil=(y, z), opd=converging_opd(y, z, 10.0, (delta0, 0.0, 0.0)),
                      weights=lambda rng, k: np.ones(k), **kw)


def offaxis_case(offsets=((0.15, -0.1), (-0.2, 0.05)), n=600):
    """Groups whose pupils are displaced by known offsets: their chief lines have slopes of about offset / -R."""
    rng = np.random.default_rng(31)
    ys, zs = [], []
    for oy, oz in offsets:
        r, t = 0.3 * np.sqrt(rng.random(n)), rng.random(n) * 2 * math.pi
        ys.append(oy + r * np.cos(t))
        zs.append(oz + r * np.sin(t))
    y, z = np.concatenate(ys), np.concatenate(zs)
    return R.psf_case([[n]] * len(offsets), pixels=(9, 7), pixel_size=0.4 * R.LAMBDA_F, pupil=(y, z), opd_waves=0.1,
                      seed=32)
