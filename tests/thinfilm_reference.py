"""An extended-precision reference of a layer stack's r_s, r_p, t_s, t_p, independent of the kernel's formulation, and the
cases of the regimes the random stacks of tests/coating_reference.py leave out: strongly absorbing, evanescent and very
thick layers, angles next to the critical one and to grazing, a resonant cavity.

Conventions: include/prt.h ("Coefficients", "Which side the ray comes from", "The far medium"): the branch with
Im(n cos theta) >= 0, eta_s = n cos theta and eta_p = n / cos theta, transmitted coefficients power-normalised, r_p with the
sign of the basis s, pi, pt.

Formulation: no characteristic matrices.  The effective admittance Y is recursed from the far medium to the near one,
    rho = (eta_j - Y) / (eta_j + Y),   Y <- eta_j (1 - rho e^{2 i delta_j}) / (1 + rho e^{2 i delta_j}),
and t is carried as the product of the layers' factors e^{i delta_j} (1 + rho) / (1 + rho e^{2 i delta_j}); only e^{i delta}
and e^{2 i delta} appear, of modulus <= 1, so nothing overflows for any finite thickness and an opaque layer gives exactly
the bulk r and t = 0.  (In the code the quotients are multiplied through by eta_j + Y and the denominator is written on
1 - e^{2 i delta}: the same numbers, without the cancellation of 1 + rho e^{2 i delta} where rho -> -1.)

Precision: numpy.longdouble (64-bit mantissa, exponents to 1e4932).  The inputs are the doubles the kernel sees (ni,
cos theta_i, sin^2 theta_i = |ui x N|^2, the table's indices, thicknesses, the wavelength), converted exactly.  The two
places where 64 bits do not do are exact in rational arithmetic: n^2 - q (the cancellation next to a critical angle) and
the number of waves n cos theta d / lambda, whose real part is reduced modulo one before it meets 2 pi (a phase of 4e5
rad carries 64 bits' rounding at 2e-14).  tests/test_host_thinfilm_reference.py holds all this to a 40-digit evaluation.

The margin of an interface, from the reference alone: the largest change of any of the four coefficients when every
thickness and the Snell invariant q = (ni sin theta_i)^2 are scaled by 1 + 8 * 2^-53 and by 1 - 8 * 2^-53.  The 8 is twice
the four roundings the kernel's phase takes (the constant 2 pi, the product, the quotient, the scale by n cos theta); q
stands for the cancellation in n^2 - q.  It is what a correctly rounded double evaluation may differ by where the
coefficients are ill-conditioned, and nothing (some 1e-15) where they are not."""
import functools
from fractions import Fraction

import numpy as np

import coating_reference as cr
import fresnel_reference as ref

LD, CLD = np.longdouble, np.clongdouble
I = CLD(1j)
TWO_PI = 2 * LD("3.14159265358979323846264338327950288419716939937510")
EIGHT_ULPS = Fraction(8, 2 ** 53)
LAM = 0.55
POLARIZATIONS = (None, (0.3, 1.0, -0.2), (0.0, 1.0, 1.0j))
CAP, TIGHT_CAP = 1e-9, 1e-13  # (what the margin of a case may be; the tight one where the regime is well conditioned)


# ---- exact pieces -------------------------------------------------------------------------------------------------------
def to_ld(f):
    """A Fraction as a longdouble, to its last bit or two."""
    out = LD(0)
    for _ in range(3):
        part = float(f)
        out, f = out + LD(part), f - Fraction(part)
    return out


def to_fraction(x):
    """A longdouble as a Fraction, exactly."""
    high = float(x)
    return Fraction(high) + Fraction(float(x - LD(high)))


def ncos_exact(n, q):
    """n cos(theta) = sqrt(n^2 - q) on the branch Im >= 0 as a pair of Fractions good to some 35 digits: n^2 - q exactly,
    its square root in longdouble, then one Newton step in rational arithmetic."""
    nr, ni = Fraction(float(n.real)), Fraction(float(n.imag))
    wr, wi = nr * nr - ni * ni - q, 2 * nr * ni
    if wr == 0 and wi == 0:
        return Fraction(0), Fraction(0)
    re, im = to_ld(wr), to_ld(wi)
    t = np.sqrt((np.hypot(re, im) + abs(re)) / 2)
    o = abs(im) / (2 * t)
    sr, si = (t, o if im >= 0 else -o) if re >= 0 else (o, t if im >= 0 else -t)
    sr, si = to_fraction(sr), to_fraction(si)  # (64 bits of the root: the Newton step squares its error)
    m = sr * sr + si * si
    sr, si = (sr + (wr * sr + wi * si) / m) / 2, (si + (wi * sr - wr * si) / m) / 2
    if si < 0 or (si == 0 and sr < 0):
        sr, si = -sr, -si
    return sr, si


def angle_of(waves):
    """2 pi waves modulo 2 pi in [-pi, pi) for a real Fraction: reduced exactly, then one rounding."""
    turn = waves - (waves.numerator // waves.denominator)
    if turn >= Fraction(1, 2):
        turn -= 1
    return TWO_PI * to_ld(turn)


def phases(sr, si, waves):
    """(e^{i delta}, e^{2 i delta}, 1 - e^{2 i delta}) for delta = 2 pi (sr + i si) waves, si >= 0.  The last without
    cancellation: its real part is -expm1(-y) + e^{-y} 2 sin^2(x / 2) for 2 delta = x + i y, both terms >= 0."""
    x1, y1 = angle_of(sr * waves), TWO_PI * to_ld(si * waves)
    e1 = (CLD(np.cos(x1)) + I * CLD(np.sin(x1))) * CLD(np.exp(-y1))
    x, y = angle_of(2 * sr * waves), 2 * y1
    decay = np.exp(-y)
    e2 = (CLD(np.cos(x)) + I * CLD(np.sin(x))) * CLD(decay)
    return e1, e2, CLD(-np.expm1(-y) + decay * 2 * np.sin(x / 2) ** 2) - I * CLD(decay * np.sin(x))


def evaluate(ni, ci, q, far, layers, lam, scale=Fraction(1)):
    """(r_s, r_p, t_s, t_p) in the conventions of include/prt.h; layers [(n, d)] from the near medium to the far one; q a
    Fraction; thicknesses and q are scaled by `scale`."""
    q = q * scale
    near = (LD(ni) * LD(ci), LD(ni) / LD(ci))
    far = complex(far)
    fr, fi = ncos_exact(far, q)
    far_ncos = CLD(to_ld(fr)) + I * CLD(to_ld(fi))
    far_n = CLD(LD(far.real)) + I * CLD(LD(far.imag))
    y = [far_ncos, far_n * far_n / far_ncos]
    eta_far = list(y)
    through = [CLD(1), CLD(1)]
    for n, d in reversed(layers):
        n = complex(n)
        sr, si = ncos_exact(n, q)
        waves = Fraction(float(d)) * scale / Fraction(float(lam))
        e1, e2, less = phases(sr, si, waves)  # (e^{i delta}, e^{2 i delta}, 1 - e^{2 i delta}: moduli <= 1, 1, 2)
        ncos = CLD(to_ld(sr)) + I * CLD(to_ld(si))
        nn = CLD(LD(n.real)) + I * CLD(LD(n.imag))
        for pol, eta in enumerate((ncos, nn * nn / ncos)):
            # (1 -+ rho e^{2 i delta}, times eta + Y, written on 1 - e^{2 i delta}: nothing cancels where eta -> 0 or oo.
            # Y = eta (1 - back) with back = 2 (eta - Y) e^{2 i delta} / below, what returns from the far side: under
            # 2^-66 it is beyond the last bit, and the layer is the bulk material, exactly)
            swing = (eta - y[pol]) * less
            below = 2 * eta - swing
            through[pol] = through[pol] * e1 * 2 * eta / below
            back = 2 * (eta - y[pol]) * e2 / below
            y[pol] = eta if abs(back) < LD(2) ** -66 else eta * (2 * y[pol] + swing) / below
    out = []
    for pol in (0, 1):
        r = (near[pol] - y[pol]) / (near[pol] + y[pol])
        t = 2 * near[pol] / (near[pol] + y[pol]) * through[pol] * np.sqrt(max(eta_far[pol].real, LD(0)) / near[pol])
        out.append((r if pol == 0 else -r, t))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@functools.lru_cache(maxsize=None)
def stack_coefficients(ni, ci, xx, far, layers, lam):
    """((r_s, r_p, t_s, t_p) as clongdouble, margin) for the doubles the kernel sees: ni, cos theta_i, sin^2 theta_i, the
    far index, the layers ((n, d), ...) from the near medium to the far one, the wavelength."""
    q = Fraction(float(ni)) ** 2 * Fraction(float(xx))
    with np.errstate(all="ignore"):
        want = evaluate(ni, ci, q, far, layers, lam)
        moved = [evaluate(ni, ci, q, far, layers, lam, 1 + sign * EIGHT_ULPS) for sign in (1, -1)]
    margin = max(float(abs(other[k] - want[k])) for other in moved for k in range(4))
    return want, margin


class Longdouble:
    """The formulation= of coating_reference.fresnel that evaluates the stack here."""

    @staticmethod
    def projected(ni, cos_i, sin2, far, layers, lam, reflection):
        c, margin = stack_coefficients(float(ni), float(cos_i), float(sin2), complex(far),
                                       tuple((complex(n), float(d)) for n, d in layers), float(lam))
        cs, cp = (c[0], c[1]) if reflection else (c[2], c[3])
        return complex(cs), complex(cp), margin


def interfaces(frame, coatings):
    """The coated interfaces of a frame as the arguments of Longdouble.projected, in the order of the rows."""
    seen = []

    class Recorder:
        @staticmethod
        def projected(*arguments):
            seen.append(arguments)
            return Longdouble.projected(*arguments)

    cr.fresnel(frame, None, (), coatings, formulation=Recorder)
    return seen


def fresnel(frame, polarization=None, lossless=(), coatings=None):
    """coating_reference.fresnel with the coefficients from here; the result has `margin` per row as well: the sum of
    the margins of the coated interfaces the ray has crossed (every coefficient has modulus <= 1, so a row's fields carry
    at most that much of them)."""
    return cr.fresnel(frame, polarization, lossless, coatings, formulation=Longdouble)


# ---- the frames ------------------------------------------------------------------------------------------------------------
def four_ways(theta, azimuth=0.0, ambient=1.0, glass=1.5, surface=1):
    """coating_reference.four_ways for any ambient index: theta is the angle on the ambient side."""
    u = cr.tilted(theta, azimuth)
    inside = ref.snell(u, cr.X, ambient, glass)
    back = np.array([-1.0, 1.0, 1.0])
    return [[(u, ambient, surface), (inside, glass, surface + 1), (u, ambient, surface + 2)],
            [(inside * back, glass, surface), (u * back, ambient, surface + 2)],
            [(u, ambient, surface), (ref.mirror(u, cr.X), ambient, surface + 2)],
            [(inside * back, glass, surface), (ref.mirror(inside * back, cr.X), glass, surface + 2)]]


def inner_reflection(theta, azimuth=0.0, glass=1.5, surface=1):
    """One ray reflected on the substrate side at the angle theta inside the glass (past the critical angle nothing else
    is there)."""
    u = cr.tilted(theta, azimuth) * np.array([-1.0, 1.0, 1.0])
    return [(u, glass, surface), (ref.mirror(u, cr.X), glass, surface + 2)]


def frame_of(rays, id0=0):
    return cr.with_wavelengths(ref.synthetic(rays, id0=id0), (LAM,))


def thickness_for(material, theta, im_delta, ambient=1.0):
    """The thickness at which a layer has Im(delta) = im_delta for light at theta in the ambient."""
    w = np.sqrt(complex(material) ** 2 - (ambient * np.sin(theta)) ** 2)
    return im_delta * LAM / (2 * np.pi * abs(w.imag))


LADDER = (1.0, 20.0, 40.0, 200.0, 340.0, 360.0, 700.0, 720.0, 1500.0, 1e5)  # (Im delta of the one layer)
METALS = {"silver": 0.2 + 3.4j, "aluminium": 1.2 + 7.0j}
LADDER_ANGLE = 0.3


def ladder(metal, n_rays=None):
    """One layer of the metal over glass of index 1.5 at the thicknesses of LADDER, each on a surface of its own, the four
    ways through each at 0.3 rad; with n_rays, that many rays spread over the coatings, the ways and a few angles."""
    m = METALS[metal]
    stacks = {10 * k + 1: cr.Stack([(m, thickness_for(m, LADDER_ANGLE, a))], substrate=1.5) for k, a in enumerate(LADDER)}
    if n_rays is None:
        rays = [ray for surface in stacks for ray in four_ways(LADDER_ANGLE, 0.4, surface=surface)]
    else:
        rng = np.random.default_rng(n_rays)
        rays = [four_ways(rng.uniform(0.05, 1.3), rng.uniform(0, 2 * np.pi), surface=10 * (k % 10) + 1)[(k // 10) % 4]
                for k in range(n_rays)]
    return frame_of(rays, id0=3), stacks


def ladder_sum():
    """Three layers of Im delta about 300 each: no single layer overflows exp, their sum does."""
    silver, aluminium = METALS["silver"], METALS["aluminium"]
    layers = [(silver, thickness_for(silver, LADDER_ANGLE, 300.0)), (aluminium, thickness_for(aluminium, LADDER_ANGLE, 300.0)),
              (silver, thickness_for(silver, LADDER_ANGLE, 300.0))]
    return frame_of(four_ways(LADDER_ANGLE, 0.4) + four_ways(1.1, 2.0)), {1: cr.Stack(layers, substrate=1.5)}


GAPS = (0.01, 0.1, 1.0, 10.0, 100.0, 1000.0)  # (d / lambda of the gap)
GAP_ANGLES = np.radians([45.0, 60.0])
GAP_MEDIA = (1.5, 1.0, 1.6)  # (ambient, gap, substrate: the transmitted ray deviates, the reflected one has a substrate)


def evanescent():
    """Frustrated total internal reflection as a coating: a gap of index 1 between 1.5 and 1.6, in the plane of
    incidence xy (s is z).  Rays 4 k .. 4 k + 3 are the four ways of (gap k // 2, angle k % 2)."""
    ambient, gap, substrate = GAP_MEDIA
    stacks = {10 * k + 1: cr.Stack([(gap, g * LAM)], ambient=ambient, substrate=substrate) for k, g in enumerate(GAPS)}
    rays = [ray for surface in stacks for theta in GAP_ANGLES for ray in four_ways(theta, 0.0, ambient, substrate, surface)]
    return frame_of(rays), stacks


OFFSETS = (1e-6, -1e-6, 1e-9, -1e-9, 1e-12, -1e-12)  # (relative, in sin theta, from the critical angle)


def critical_layer():
    """A layer of index 1 in a 1.5 | 1 | 1.6 stack next to ITS critical angle: the far medium propagates, so all four
    ways exist and no flag hangs on the offset.  (A layer's matrix is even in its n cos theta: well conditioned.)"""
    ambient, gap, substrate = GAP_MEDIA
    stacks = {1: cr.Stack([(gap, 0.3)], ambient=ambient, substrate=substrate)}
    rays = [ray for off in OFFSETS for ray in four_ways(np.arcsin(gap / ambient * (1 + off)), 0.7, ambient, substrate)]
    return frame_of(rays), stacks


# The far medium next to its critical angle is where the definition itself is ill-conditioned: its n cos theta is
# sqrt(n^2 - q), so eight ulps of q move it by 4.4e-16 n^2 / (n cos theta), and the coefficients with it: r by about
# that, and the power-normalised t, which goes with sqrt(n cos theta), by more.  The margins at the offsets the frames
# below leave out are over the cap (tests/test_host_thinfilm_reference.py asserts that they are): a ray that leaves the
# glass 1e-9 or 1e-12 under the critical angle (2e-9, 4e-7), a total reflection 1e-12 above it (1.3e-9), and a ray that
# leaves the glass at 1e-6 from grazing (5e-7).  What takes their place is the closest offset under the cap.
FAR_ABOVE = (1e-6, 1e-9, 2e-12)  # (total reflection inside the glass)
FAR_BELOW_FROM_AIR = (-1e-6, -1e-9, -1e-12)  # (the ray in the air is nearly grazing: into the glass, reflected off it)
FAR_BELOW_FROM_GLASS = (-1e-6, -1e-8)  # (out of the glass, reflected inside it)
FAR_LEFT_OUT = ((-1e-9, (1, 3)), (-1e-12, (1, 3)), (1e-12, None))  # ((offset, the ways of four_ways or the reflection))
FAR_STACK = cr.Stack([(1.38, 0.1)], substrate=1.5)


def far_rays(off, ways):
    if ways is None:
        return [inner_reflection(np.arcsin((1 + off) / 1.5), 0.7)]
    return [four_ways(np.arcsin(1 + off), 0.7)[k] for k in ways]


def critical_far():
    """The far medium (air behind glass of 1.5 under a propagating layer of 1.38) next to its critical angle."""
    rays = [ray for off in FAR_ABOVE for ray in far_rays(off, None)]
    rays += [ray for off in FAR_BELOW_FROM_AIR for ray in far_rays(off, (0, 2))]
    rays += [ray for off in FAR_BELOW_FROM_GLASS for ray in far_rays(off, (1, 3))]
    return frame_of(rays), {1: FAR_STACK}


GRAZING = (1e-2, 1e-4, 1e-6)  # (pi / 2 - theta in the air)
GRAZING_FROM_GLASS = (1e-2, 1e-4)  # (the ray that leaves the glass at 1e-6 from grazing: see above)
GRAZING_STACK = cr.Stack([(1.38, 0.1), (2.1 + 0.05j, 0.07)], substrate=1.5)


def grazing():
    rays = [four_ways(np.pi / 2 - eps, 0.7)[k] for eps in GRAZING for k in (0, 2)]
    rays += [four_ways(np.pi / 2 - eps, 0.7)[k] for eps in GRAZING_FROM_GLASS for k in (1, 3)]
    return frame_of(rays), {1: GRAZING_STACK}


def thick():
    """Lossless layers of 1 mm and 25 mm: phases of 1.6e4 to 5e5 rad."""
    stacks = {1: cr.Stack([(1.38, 1000.0)], substrate=1.5), 11: cr.Stack([(1.7, 25000.0)], substrate=1.5),
              21: cr.Stack([(1.38, 1000.0), (2.0, 25000.0)], substrate=1.5)}
    rays = [ray for surface in stacks for theta in (0.0, 0.3, 1.0) for ray in four_ways(theta, 0.7, surface=surface)]
    return frame_of(rays), stacks


CAVITY_WAVELENGTHS = (0.548, 0.549, 0.55, 0.551, 0.552)  # (T = 0.45, 0.75, 0.96, 0.75, 0.46 at normal incidence)


def cavity():
    """H L H L H L H (2L) H L H L H L H of 2.35 / 1.38 over 1.52, quarter waves at 0.55: fifteen layers, a spacer of
    half a wave between two mirrors, at five wavelengths across its passband in one table."""
    high, low = (2.35, 0.55 / (4 * 2.35)), (1.38, 0.55 / (4 * 1.38))
    mirror = [high, low, high, low, high, low, high]
    stacks = {1: cr.Stack(mirror + [(1.38, 0.55 / (2 * 1.38))] + mirror, substrate=1.52)}
    rays = [ray for _ in CAVITY_WAVELENGTHS for theta in (0.0, 0.1) for ray in four_ways(theta, 0.7, glass=1.52)]
    frame = ref.synthetic(rays)
    ids = frame[:, ref.IX["id"]].astype(int)
    frame[:, ref.IX["wavelength"]] = np.asarray(CAVITY_WAVELENGTHS)[ids // 8]
    return frame, stacks


# name -> (regime, builder, the margin's cap)
CASES = {
    "ladder silver": ("attenuation", lambda: ladder("silver"), TIGHT_CAP),
    "ladder aluminium": ("attenuation", lambda: ladder("aluminium"), TIGHT_CAP),
    "ladder silver, 65 rays": ("attenuation", lambda: ladder("silver", 65), TIGHT_CAP),
    "ladder aluminium, 257 rays": ("attenuation", lambda: ladder("aluminium", 257), TIGHT_CAP),
    "three layers of 300": ("attenuation", ladder_sum, TIGHT_CAP),
    "evanescent gap": ("evanescent", evanescent, TIGHT_CAP),
    "a layer at its critical angle": ("critical", critical_layer, CAP),
    "the far medium at its critical angle": ("critical", critical_far, CAP),
    "grazing incidence": ("grazing", grazing, CAP),
    "large real phase": ("thick", thick, CAP),
    "cavity of 15 layers": ("cavity", cavity, CAP),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][1]()


@functools.lru_cache(maxsize=None)
def reference(name, polarization):
    """The reference's result for a case, computed once and shared (do not write into it)."""
    frame, stacks = case(name)
    return fresnel(frame, polarization, coatings=stacks)
