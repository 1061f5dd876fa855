"""A numpy restatement of the enclosed-energy definitions of include/prt.h: integer weights by a power-of-two scaling,
a stable sort of the distances, an integer cumulative sum and searchsorted.  tests/test_host_enclosed_energy.py checks
it against closed forms on the CPU; tests/test_gpu_enclosed_energy.py checks the device against it."""
import numpy as np

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}
SHAPES = ("circle", "square", "slit_e1", "slit_e2")


def integer_weights(w):
    """q = (uint64) floor(ldexp(w, 62 - E - B)) with w_max = f 2^E (0.5 <= f < 1) and B = bit_length(len(w))."""
    w = np.asarray(w, dtype=np.float64)
    if not len(w) or not w.max() > 0:
        return np.zeros(len(w), dtype=np.uint64)
    _, e = np.frexp(w.max())
    return np.floor(np.ldexp(w, 62 - int(e) - int(len(w)).bit_length())).astype(np.uint64)


def distances(p, s, delta, c, shape):
    """d of every ray at the plane shifted by delta, about c: x = (p + delta s) - c, in that order."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = (p + delta * s) - c
        bad = np.isnan(x).any(axis=1)
        if shape == "circle":
            d = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
        elif shape == "square":
            d = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))
        elif shape == "slit_e2":
            d = np.abs(x[:, 0])
        elif shape == "slit_e1":
            d = np.abs(x[:, 1])
        else:
            raise ValueError(shape)
    return np.where(bad, np.inf, d)


def plane_centre(p, s, w, delta, follow_centroid):
    if not follow_centroid:
        return np.zeros(2)
    with np.errstate(over="ignore", invalid="ignore"):
        return (w @ p) / w.sum() + delta * ((w @ s) / w.sum())


def enclosed(p, s, w, radii=(), fractions=(), focus=(0.0,), shape="circle", follow_centroid=True):
    """energy (n_focus, n_radii), radius (n_focus, n_fractions) and the smallest relative distance between a ray and a
    radius, for one group's staged rays p (n, 2), s (n, 2), w (n)."""
    p, s, w = (np.asarray(v, dtype=np.float64) for v in (p, s, w))
    radii, fractions = np.asarray(radii, dtype=np.float64), np.asarray(fractions, dtype=np.float64)
    energy = np.full((len(focus), len(radii)), np.nan)
    radius = np.full((len(focus), len(fractions)), np.nan)
    q = integer_weights(w)
    total = int(q.sum(dtype=np.uint64))
    margin = np.inf
    if total == 0:
        return energy, radius, margin
    need = np.array([min(max(int(np.ceil(phi * float(total))), 1), total) for phi in fractions], dtype=np.uint64)
    for f, delta in enumerate(focus):
        d = distances(p, s, delta, plane_centre(p, s, w, delta, follow_centroid), shape)
        order = np.argsort(d, kind="stable")
        d_sorted, run = d[order], np.cumsum(q[order], dtype=np.uint64)
        inside = np.searchsorted(d_sorted, radii, side="right")  # rays with d <= R
        below = np.concatenate([[np.uint64(0)], run])[inside]
        energy[f] = below.astype(np.float64) / np.float64(total)
        radius[f] = d_sorted[np.searchsorted(run, need, side="left")]
        finite = d_sorted[np.isfinite(d_sorted)]
        for edge in radii:
            if len(finite):
                margin = min(margin, float(np.min(np.abs(finite - edge)) / max(edge, np.finfo(float).tiny)))
    return energy, radius, margin


def clear_radii(samples, count, gap=1e-6):
    """`count` ascending radii at midpoints between neighbours of the sorted finite distances `samples`, no ray within
    `gap` (relative) of any of them."""
    d = np.unique(np.asarray(samples, dtype=np.float64))
    d = d[np.isfinite(d)]
    mid = 0.5 * (d[1:] + d[:-1])
    mid = mid[(d[1:] - mid > gap * mid) & (mid - d[:-1] > gap * mid)]
    picks = np.unique(np.linspace(0, len(mid) - 1, count).round().astype(int))
    assert len(picks) == count, "not enough clear gaps between the distances"
    return mid[picks]


def stage(frame, surface, axes=None, rays_per_source=None, n_groups=1, weights="intensity", reference=None):
    """Per group (p, s, w, centre, rays used, rays left out) from a host frame (n, 15): the MTF's staging restated."""
    if axes is None:
        axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    a, e1, e2 = axes[:3], axes[3:6], axes[6:]
    rows = frame if surface is None else frame[frame[:, IX["surface"]] == surface]
    groups = np.floor(rows[:, IX["id"]] / rays_per_source) if rays_per_source else np.zeros(len(rows))
    keep = (groups >= 0) & (groups < n_groups)
    rows, groups = rows[keep], groups[keep].astype(int)
    q, u = rows[:, 9:12], rows[:, 12:15]
    w = np.ones(len(rows)) if weights is None else rows[:, IX[weights]]
    with np.errstate(invalid="ignore", divide="ignore"):
        ua = u @ a
        s = np.stack([u @ e1, u @ e2], 1) / ua[:, None]
    ok = (np.all(np.isfinite(q), 1) & np.all(np.isfinite(u), 1) & np.isfinite(w) & (w >= 0) & (ua != 0)
          & np.all(np.isfinite(s), 1))
    out = []
    for g in range(n_groups):
        m = ok & (groups == g)
        used, missed = int(m.sum()), int(((groups == g) & ~ok).sum())
        if not used:
            out.append((np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.full(3, np.nan), 0, missed))
            continue
        if reference is None:
            with np.errstate(invalid="ignore", divide="ignore"):
                c = (w[m] @ q[m]) / w[m].sum()
        else:
            c = np.asarray(reference[g], dtype=float)
        d = q[m] - c
        p = np.stack([d @ e1, d @ e2], 1) - s[m] * (d @ a)[:, None]
        out.append((p, s[m], w[m], c, used, missed))
    return out


def vogel_disk(n, a):
    """n points of equal weight filling a disk of radius a evenly: r_i = a sqrt((i + 0.5) / n), golden-angle turns."""
    i = np.arange(n)
    r, t = a * np.sqrt((i + 0.5) / n), i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(t), r * np.sin(t)], 1), r
