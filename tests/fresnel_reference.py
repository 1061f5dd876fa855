"""A numpy restatement of the Fresnel definitions of include/prt.h, operation for operation: every product and sum is
one numpy ufunc call (rounded on its own, as the kernel's are under -ffp-contract=off), dot products as
(x x' + y y') + z z', in the order csrc/prt_fresnel.hpp writes them.  A generation's rows are handled as arrays, every
branch computed for every row and picked by np.where.  tests/test_host_fresnel.py checks it against closed forms;
tests/test_gpu_fresnel.py checks the device against it."""
import numpy as np

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}
EPS_DIR = 1e-12


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def unit(a):
    return a / np.sqrt(dot(a, a))


def through(e, s, pi, pt, cs, cp):
    fs, fp = cs * dot(e, s), cp * dot(e, pi)
    return fs * s + fp * pt


def launch(u_raw, polarization):
    """Generation 0: (ea, eb, bad) of the rows whose raw directions are the columns of u_raw."""
    mm = dot(u_raw, u_raw)
    u0 = u_raw / np.sqrt(mm)
    bad = ~((mm > 0.0) & (mm < np.inf))
    if polarization is not None:
        x, y, z = (float(c) for c in polarization)
        v = np.array([x, y, z]) / np.sqrt((x * x + y * y) + z * z)
        v = np.repeat(v[:, None], u0.shape[1], axis=1)
        along = dot(v, u0)
        w = v - along * u0
        ww = dot(w, w)
        bad = bad | ~(ww > EPS_DIR)
        return w / np.sqrt(ww), np.zeros_like(u0), bad
    magnitude = np.abs(u0)
    axis = np.zeros(u0.shape[1], dtype=int)
    least = magnitude[0].copy()
    pick = magnitude[1] < least
    axis[pick], least[pick] = 1, magnitude[1][pick]
    axis[magnitude[2] < least] = 2
    e = np.stack([(axis == k).astype(np.float64) for k in range(3)])
    ea = unit(cross(u0, e))
    return ea, cross(u0, ea), bad


def interface(ui, ut, ni, nt, lossless, ea, eb, t_before, polarised):
    """One interface for arrays of rays: (ea, eb, t, reflection, undeviated, newly invalid)."""
    d = ui - ut
    dd = dot(d, d)
    ok = (dd < np.inf) & (ni > 0.0) & (ni < np.inf) & (nt > 0.0) & (nt < np.inf)
    same = ni == nt
    undeviated = ok & same & (dd <= EPS_DIR)
    reflection = ok & same & ~undeviated
    refraction = ok & ~same
    n = unit(np.stack([ni * ui[0] - nt * ut[0], ni * ui[1] - nt * ut[1], ni * ui[2] - nt * ut[2]]))
    ci = dot(ui, n)
    flip = ci < 0.0
    n = np.where(flip, -n, n)
    ci = np.where(flip, -ci, ci)
    ct = dot(ut, n)
    bad = ~ok | (refraction & ~((ci > 0.0) & (ct > 0.0)))
    a, b, c, e = ni * ci, nt * ct, nt * ci, ni * ct
    twice = 2.0 * np.sqrt(a * b)
    cs = np.where(reflection, -1.0, np.where(lossless, 1.0, twice / (a + b)))
    cp = np.where(reflection, 1.0, np.where(lossless, 1.0, twice / (c + e)))
    n = np.where(reflection, d / np.sqrt(dd), n)
    x = cross(ui, n)
    xx = dot(x, x)
    normal = xx <= EPS_DIR
    s = x / np.sqrt(xx)
    pi, pt = cross(ui, s), cross(ut, s)
    new_a = np.where(normal, cs * ea, through(ea, s, pi, pt, cs, cp))
    new_b = np.where(normal, cs * eb, through(eb, s, pi, pt, cs, cp))
    new_a, new_b = np.where(undeviated, ea, new_a), np.where(undeviated, eb, new_b)
    aa = dot(new_a, new_a)
    from_fields = aa if polarised else (aa + dot(new_b, new_b)) / 2.0
    t = np.where(refraction & ~lossless, from_fields, t_before)
    dead = bad | (t_before != t_before)
    new_a, new_b = np.where(dead, np.nan, new_a), np.where(dead, np.nan, new_b)
    return new_a, new_b, np.where(dead, np.nan, t), reflection, undeviated, bad & (t_before == t_before)


def fresnel(frame, polarization=None, lossless=()):
    """Everything prt_frame_fresnel reports for a frame given as (n_rows, 15): transmittance (n_rows), field
    (6, n_rows) and the counters.  ValueError where the definitions refuse the frame."""
    frame = np.asarray(frame, dtype=np.float64)
    n_rows = len(frame)
    generation = frame[:, IX["generation"]].astype(np.int64)
    ids = frame[:, IX["id"]]
    if n_rows and not np.all(np.isfinite(ids) & (ids == np.floor(ids))):
        raise ValueError("an id is not an integer")
    t_out = np.full(n_rows, np.nan)
    field = np.full((6, n_rows), np.nan)
    counters = dict(n_reflections=0, n_lossless=0, n_undeviated=0, n_invalid=0)
    coated = np.array(sorted(float(s) for s in lossless))
    previous = {}  # id -> its row in the generation before
    with np.errstate(all="ignore"):
        for g in range(int(generation.max()) + 1 if n_rows else 0):
            rows = np.flatnonzero(generation == g)
            if len(set(ids[rows])) != len(rows):
                raise ValueError("an id repeats within a generation")
            tilt = frame[rows, 12:15].T
            if g == 0:
                ea, eb, bad = launch(tilt, polarization)
                ea, eb = np.where(bad, np.nan, ea), np.where(bad, np.nan, eb)
                t = np.where(bad, np.nan, 1.0)
                counters["n_invalid"] += int(bad.sum())
            else:
                if any(ray not in previous for ray in ids[rows]):
                    raise ValueError("a ray has a row in a generation and none in the one before")
                before = np.array([previous[ray] for ray in ids[rows]], dtype=np.int64)
                ut = tilt / np.sqrt(dot(tilt, tilt))
                ui = unit(frame[before, 12:15].T)
                is_coated = np.isin(frame[before, IX["surface"]], coated)
                ea, eb, t, reflection, undeviated, invalid = interface(
                    ui, ut, frame[before, IX["index"]], frame[rows, IX["index"]], is_coated, field[:3, before],
                    field[3:, before], t_out[before], polarization is not None)
                counters["n_reflections"] += int(reflection.sum())
                counters["n_lossless"] += int(is_coated.sum())
                counters["n_undeviated"] += int(undeviated.sum())
                counters["n_invalid"] += int(invalid.sum())
            field[:3, rows], field[3:, rows], t_out[rows] = ea, eb, t
            previous = {ray: row for ray, row in zip(ids[rows], rows)}
    return dict(transmittance=t_out, field=field, **counters)


# ---- frames built by hand ---------------------------------------------------------------------------------------------
def snell(u, normal, n1, n2):
    """The refracted unit direction of unit u at a surface with unit normal `normal` (either sense), from n1 into n2."""
    u, normal = np.asarray(u, dtype=float), np.asarray(normal, dtype=float)
    if u @ normal < 0:
        normal = -normal
    r = n1 / n2
    ci = u @ normal
    ct = np.sqrt(1.0 - r * r * (1.0 - ci * ci))
    out = r * u + (ct - r * ci) * normal
    return out / np.linalg.norm(out)


def mirror(u, normal):
    u, normal = np.asarray(u, dtype=float), np.asarray(normal, dtype=float)
    return u - 2.0 * (u @ normal) * normal


def synthetic(rays, id0=0):
    """A whole frame (n_rows, 15), generation-major, from rays given as lists of segments (direction, index, surface):
    ray k has id id0 + k and one row per segment; `surface` is what the segment ends on."""
    depth = max(len(segments) for segments in rays)
    lines = []
    for g in range(depth):
        for k, segments in enumerate(rays):
            if g < len(segments):
                direction, index, surface = segments[g]
                line = np.zeros(15)
                line[IX["generation"]], line[IX["intensity"]], line[IX["wavelength"]] = g, 100.0, 0.633
                line[IX["index"]], line[IX["id"]], line[IX["surface"]] = index, id0 + k, surface
                line[12:15] = direction
                lines.append(line)
    return np.array(lines)


def power_coefficients(theta_i, n1, n2):
    """(T_s, T_p) of an uncoated interface from the textbook reflection coefficients: T = 1 - r^2."""
    theta_t = np.arcsin(n1 * np.sin(theta_i) / n2)
    rs = (n1 * np.cos(theta_i) - n2 * np.cos(theta_t)) / (n1 * np.cos(theta_i) + n2 * np.cos(theta_t))
    rp = (n2 * np.cos(theta_i) - n1 * np.cos(theta_t)) / (n2 * np.cos(theta_i) + n1 * np.cos(theta_t))
    return 1.0 - rs * rs, 1.0 - rp * rp
