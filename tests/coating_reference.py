"""An independent numpy restatement, in complex128, of the coating definitions of include/prt.h: one ray and one
interface at a time, the characteristic matrices of the layers as 2x2 numpy matrices multiplied per row.  Written from
the definitions, not from csrc/prt_coatings.hpp: the angle of incidence comes from the cosine, the layers' matrices are
multiplied as matrices, and a second formulation (Rouard's recursion over the interfaces) checks the first.
tests/test_host_coatings.py holds it to closed forms; tests/test_gpu_coatings.py holds the device to it."""
import numpy as np

import fresnel_reference as ref

IX = ref.IX
EPS_DIR = ref.EPS_DIR


class Stack:
    """What a coating is to this module: layers [(material, thickness)] from the ambient side to the substrate side,
    ambient, substrate or None.  pyrayt_amd.materials.Coating has the same three attributes and is taken as well."""

    def __init__(self, layers=(), ambient=1.0, substrate=None):
        self.layers, self.ambient, self.substrate = tuple(layers), ambient, substrate


def index(material, lam):
    if hasattr(material, "index_at"):
        return complex(np.asarray(material.index_at(np.array([lam])), dtype=complex).reshape(-1)[0])
    if callable(material):
        return complex(np.asarray(material(np.array([lam])), dtype=complex).reshape(-1)[0])
    return complex(material)


def cosine(n, invariant):
    """cos(theta) in a medium of index n for the Snell invariant ni sin(theta_i), on the branch Im(n cos theta) >= 0."""
    c = np.sqrt(complex(1.0 - (invariant / n) ** 2))
    if (n * c).imag < 0 or ((n * c).imag == 0 and (n * c).real < 0):
        c = -c
    return c


def admittances(n, c):
    return n * c, n / c  # (s, p)


def matrix_coefficients(n_near, cos_near, far, layers, lam):
    """(r_s, r_p, t_s, t_p) of a stack in the tangential-field convention, both polarisations alike:
    r = (eta0 B - C) / (eta0 B + C), t = 2 eta0 / (eta0 B + C), (B, C) = M_1 ... M_L (1, eta_far).  layers: [(n, d)] from
    the near medium to the far medium.  Fields as exp(-i omega t): n + ik absorbs, and a layer's matrix is
    [[cos d, -i sin d / eta], [-i eta sin d, cos d]]."""
    invariant = n_near * np.sqrt(1.0 - cos_near * cos_near)
    out = []
    for pol in (0, 1):
        eta0 = admittances(n_near, cos_near)[pol]
        m = np.eye(2, dtype=complex)
        for n, d in layers:
            c = cosine(n, invariant)
            delta = 2.0 * np.pi * n * d * c / lam
            eta = admittances(n, c)[pol]
            m = m @ np.array([[np.cos(delta), -1j * np.sin(delta) / eta], [-1j * eta * np.sin(delta), np.cos(delta)]])
        eta_far = admittances(far, cosine(far, invariant))[pol]
        b, c = m @ np.array([1.0, eta_far])
        out.append(((eta0 * b - c) / (eta0 * b + c), 2.0 * eta0 / (eta0 * b + c), eta_far, eta0))
    return out


def rouard_coefficients(n_near, cos_near, far, layers, lam):
    """The same four numbers from Rouard's recursion: the stack is built up from the far medium, one interface at a
    time, out of the single-interface r_ab = (eta_a - eta_b) / (eta_a + eta_b), t_ab = 2 eta_a / (eta_a + eta_b)."""
    invariant = n_near * np.sqrt(1.0 - cos_near * cos_near)
    out = []
    for pol in (0, 1):
        media = [(n_near, cos_near + 0j)] + [(n, cosine(n, invariant)) for n, _ in layers] + [(far, cosine(far, invariant))]
        eta = [admittances(n, c)[pol] for n, c in media]
        rho = (eta[-2] - eta[-1]) / (eta[-2] + eta[-1])
        tau = 2.0 * eta[-2] / (eta[-2] + eta[-1])
        for j in range(len(layers), 0, -1):  # (layer j lies between media j - 1 and j + 1)
            n, c = media[j]
            phase = np.exp(1j * 2.0 * np.pi * n * layers[j - 1][1] * c / lam)
            r, t = (eta[j - 1] - eta[j]) / (eta[j - 1] + eta[j]), 2.0 * eta[j - 1] / (eta[j - 1] + eta[j])
            below = 1.0 + r * rho * phase * phase
            rho, tau = (r + rho * phase * phase) / below, t * tau * phase / below
        out.append((rho, tau, eta[-1], eta[0]))
    return out


def project_coefficients(raw, reflection):
    """(cs, cp) in the basis s, pi, pt of include/prt.h from the tangential-field coefficients: the reflected p basis
    vector has the opposite tangential sense (rp = -r, so a perfect conductor gives rs = -1, rp = +1); transmitted
    coefficients are power-normalised with sqrt(Re eta_far / Re eta_near)."""
    (rs, ts, far_s, near_s), (rp, tp, far_p, near_p) = raw
    if reflection:
        return rs, -rp
    return ts * np.sqrt(far_s.real / near_s.real), tp * np.sqrt(far_p.real / near_p.real)


def interface_coefficients(stack, ni, nt, cos_i, reflection, lam, formulation=matrix_coefficients, sin2=None):
    """(cs, cp, total internal reflection?) of a coated interface, or None where the definitions call it invalid.  A
    formulation with a method `projected` (tests/thinfilm_reference.py) takes sin^2 of the angle of incidence as the
    kernel has it, |ui x N|^2, as well, projects for itself and adds a fourth number, its margin."""
    if not (np.isfinite(lam) and lam > 0):
        return None
    ambient = index(stack.ambient, lam)
    layers = [(index(material, lam), d) for material, d in stack.layers]
    from_ambient = ni == ambient.real
    if not from_ambient:
        layers = layers[::-1]
    if not reflection:
        far = complex(nt)
    elif from_ambient:
        if stack.substrate is None:
            return None
        far = index(stack.substrate, lam)
    else:
        far = ambient
    values = [far] + [n for n, _ in layers]
    if not np.all(np.isfinite(values)):
        return None
    extra = ()
    with np.errstate(all="ignore"):
        if hasattr(formulation, "projected"):
            cs, cp, margin = formulation.projected(ni, cos_i, 1.0 - cos_i * cos_i if sin2 is None else sin2, far, layers,
                                                   lam, reflection)
            extra = (margin,)
        else:
            cs, cp = project_coefficients(formulation(ni, cos_i, far, layers, lam), reflection)
    if not (np.isfinite(cs) and np.isfinite(cp)):
        return None
    invariant = ni * np.sqrt(1.0 - cos_i * cos_i)
    return (cs, cp, bool(reflection and far.imag == 0 and far.real < invariant)) + extra


def transverse_basis(u):
    """The launch basis of include/prt.h for a unit direction u: e1 = u x e normalised, e2 = u x e1."""
    axis = int(np.argmin(np.abs(u)))  # (ties to the first)
    e = np.zeros(3)
    e[axis] = 1.0
    e1 = np.cross(u, e)
    e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(u, e1)


def stokes(direction, ea):
    u = np.asarray(direction, dtype=float)
    e1, e2 = transverse_basis(u / np.linalg.norm(u))
    c1, c2 = ea @ e1, ea @ e2
    return np.array([abs(c1) ** 2 + abs(c2) ** 2, abs(c1) ** 2 - abs(c2) ** 2, 2 * (np.conj(c1) * c2).real,
                     2 * (np.conj(c1) * c2).imag])


def fresnel(frame, polarization=None, lossless=(), coatings=None, formulation=matrix_coefficients):
    """Everything prt_frame_fresnel_coated reports for a frame given as (n_rows, 15): transmittance (n_rows), field
    (6, n_rows) complex and the six counters.  coatings: {surface id: Stack or Coating}.  `margin` (n_rows): the sum of
    the margins of the coated interfaces a ray has crossed, zero with a formulation that states none."""
    frame = np.asarray(frame, dtype=np.float64)
    coatings = coatings or {}
    n_rows = len(frame)
    generation = frame[:, IX["generation"]].astype(np.int64)
    t_out = np.full(n_rows, np.nan)
    field = np.full((6, n_rows), np.nan + 0j)
    margin = np.zeros(n_rows)
    names = ("n_reflections", "n_lossless", "n_undeviated", "n_invalid", "n_coated", "n_tir")
    count = dict.fromkeys(names, 0)
    previous = {}
    polarised = polarization is not None
    for g in range(int(generation.max()) + 1 if n_rows else 0):
        now = {}
        for row in np.flatnonzero(generation == g):
            ray = frame[row, IX["id"]]
            if ray in now:
                raise ValueError("an id repeats within a generation")
            now[ray] = row
            raw = frame[row, 12:15]
            with np.errstate(all="ignore"):
                ut = raw / np.sqrt(raw @ raw)
            if g == 0:
                ea, eb, t, bad = launch(raw, ut, polarization)
                if bad:
                    count["n_invalid"] += 1
                    continue
                field[:3, row], field[3:, row], t_out[row] = ea, eb, t
                continue
            if ray not in previous:
                raise ValueError("a ray has a row in a generation and none in the one before")
            before = previous[ray]
            was_dead = np.isnan(t_out[before])
            with np.errstate(all="ignore"):
                ui = frame[before, 12:15] / np.linalg.norm(frame[before, 12:15])
            ni, nt, surface = frame[before, IX["index"]], frame[row, IX["index"]], frame[before, IX["surface"]]
            is_lossless = surface in lossless
            count["n_lossless"] += int(is_lossless)
            ea, eb, t = field[:3, before], field[3:, before], t_out[before]
            margin[row] = margin[before]
            d = ui - ut
            dd = d @ d
            bad = not (dd < np.inf and 0 < ni < np.inf and 0 < nt < np.inf)
            if not bad and ni == nt and dd <= EPS_DIR:
                count["n_undeviated"] += 1
            elif not bad:
                reflection = ni == nt
                count["n_reflections"] += int(reflection)
                if reflection:
                    normal = d / np.sqrt(dd)
                    cos_i = ui @ normal
                    cs, cp, from_fields = -1.0, 1.0, False
                else:
                    normal = ni * ui - nt * ut
                    normal = normal / np.linalg.norm(normal)
                    if ui @ normal < 0:
                        normal = -normal
                    cos_i, cos_t = ui @ normal, ut @ normal
                    bad = not (cos_i > 0 and cos_t > 0)
                    a, b, c, e = ni * cos_i, nt * cos_t, nt * cos_i, ni * cos_t
                    with np.errstate(all="ignore"):
                        cs = 1.0 if is_lossless else 2.0 * np.sqrt(a * b) / (a + b)
                        cp = 1.0 if is_lossless else 2.0 * np.sqrt(a * b) / (c + e)
                    from_fields = not is_lossless
                if surface in coatings:
                    count["n_coated"] += 1
                    from_fields = True
                    x = np.cross(ui, normal)
                    found = None if bad else interface_coefficients(coatings[surface], ni, nt, min(cos_i, 1.0), reflection,
                                                                    frame[before, IX["wavelength"]], formulation, x @ x)
                    if found is None:
                        bad = True
                    else:
                        cs, cp, tir = found[:3]
                        margin[row] += sum(found[3:])
                        count["n_tir"] += int(tir)
                if not bad:
                    x = np.cross(ui, normal)
                    xx = x @ x
                    if xx <= EPS_DIR:
                        ea, eb = cs * ea, cs * eb
                    else:
                        s = x / np.sqrt(xx)
                        pi, pt = np.cross(ui, s), np.cross(ut, s)
                        ea = cs * (ea @ s) * s + cp * (ea @ pi) * pt
                        eb = cs * (eb @ s) * s + cp * (eb @ pi) * pt
                    if from_fields:
                        aa, bb = np.sum(np.abs(ea) ** 2), np.sum(np.abs(eb) ** 2)
                        t = aa if polarised else (aa + bb) / 2.0
            if bad and not was_dead:
                count["n_invalid"] += 1
            if not (bad or was_dead):
                field[:3, row], field[3:, row], t_out[row] = ea, eb, t
        previous = now
    return dict(transmittance=t_out, field=field, margin=margin, **count)


def launch(raw, u0, polarization):
    mm = raw @ raw
    if not (0 < mm < np.inf):
        return None, None, None, True
    if polarization is None:
        e1, e2 = transverse_basis(u0)
        return e1 + 0j, e2 + 0j, 1.0, False
    v = np.asarray(polarization, dtype=complex)
    v = v / np.sqrt(np.sum(np.abs(v) ** 2))
    w = v - (v @ u0) * u0
    ww = np.sum(np.abs(w) ** 2)
    if not ww > EPS_DIR:
        return None, None, None, True
    return w / np.sqrt(ww), np.zeros(3, dtype=complex), 1.0, False


def counters(got):
    return tuple(got[name] for name in ("n_reflections", "n_lossless", "n_undeviated", "n_invalid", "n_coated", "n_tir"))


def with_wavelengths(frame, wavelengths):
    """The frame with ray k's rows at wavelengths[k % len] (ids count from the frame's smallest)."""
    frame = frame.copy()
    ids = frame[:, IX["id"]]
    frame[:, IX["wavelength"]] = np.asarray(wavelengths, dtype=float)[(ids - ids.min()).astype(int) % len(wavelengths)]
    return frame


def random_stack(seed, n_layers, lam=0.633, absorbing=True, ambient=1.0, substrate=None, dispersive=False):
    """A stack with fixed seed: n_layers <= 16 layers of index 1.3..2.5, optical thickness of a layer at most one wave,
    every third layer absorbing with k d / lambda <= 0.25; with `dispersive` the first layer's index follows a Cauchy
    law."""
    rng = np.random.default_rng(seed)
    layers = []
    for k in range(n_layers):
        n = rng.uniform(1.3, 2.5)
        d = rng.uniform(0.05, 1.0) * lam / n
        kappa = min(rng.uniform(0.0, 0.3), 0.25 * lam / d) if absorbing and k % 3 == 1 else 0.0
        material = complex(n, kappa) if kappa else n
        if dispersive and k == 0:
            material = Cauchy(n, 0.01)
        layers.append((material, d))
    return Stack(layers, ambient=ambient, substrate=substrate)


class Cauchy:
    def __init__(self, a, b):
        self.a, self.b = a, b

    def index_at(self, wavelength):
        return self.a + self.b / np.asarray(wavelength, dtype=float) ** 2


# ---- the frames both suites use -------------------------------------------------------------------------------------------
X = np.array([1.0, 0.0, 0.0])


def tilted(theta, azimuth=0.0):
    return np.array([np.cos(theta), np.sin(theta) * np.cos(azimuth), np.sin(theta) * np.sin(azimuth)])


def four_ways(theta, azimuth=0.0, n_glass=1.5, surface=1):
    """Four rays at one coated face (normal x, air before it, glass behind it): refracted into the glass and out of its
    uncoated back (surface + 1), refracted out of the glass, reflected on the air side, reflected on the glass side."""
    u = tilted(theta, azimuth)
    inside = ref.snell(u, X, 1.0, n_glass)
    back = np.array([-1.0, 1.0, 1.0])
    return [[(u, 1.0, surface), (inside, n_glass, surface + 1), (u, 1.0, surface + 2)],
            [(inside * back, n_glass, surface), (u * back, 1.0, surface + 2)],
            [(u, 1.0, surface), (ref.mirror(u, X), 1.0, surface + 2)],
            [(u * back, n_glass, surface), (ref.mirror(u * back, X), n_glass, surface + 2)]]


RANDOM_STACKS = [(1, 1), (2, 2), (3, 5), (4, 9), (5, 16), (6, 16)]  # (seed, layers)
WAVELENGTHS = (0.633, 0.45)


def random_case(seed, n_layers):
    """(frame, coatings) of a random stack on surface 1 of a plate of index 1.5 (an absorbing substrate of the mirror
    kind for odd seeds is not possible there: the substrate is the glass), rays at six angles and azimuths arriving from
    both sides, refracted and reflected, at two wavelengths, the first layer dispersive."""
    rng = np.random.default_rng(100 + seed)
    stack = random_stack(seed, n_layers, substrate=1.5, dispersive=True)
    rays = []
    for theta in rng.uniform(0.02, 1.4, 6):
        rays += four_ways(theta, rng.uniform(0, 2 * np.pi))
    return with_wavelengths(ref.synthetic(rays, id0=seed), WAVELENGTHS), {1: stack}
