"""A numpy restatement of the ghost definitions of include/prt.h, operation for operation: every product and sum is one
numpy ufunc call (rounded on its own, as the kernel's are under -ffp-contract=off), dot products as
(x x' + y y') + z z', in the order csrc/prt_ghosts.hpp writes them.  It works on a frame given as (R, 15) and the
transmittance vector of a Fresnel pass of that frame.  tests/test_host_ghosts.py checks it against closed forms and the
energy balance; tests/test_gpu_ghosts.py holds the device to its bits.  The longdouble helpers at the end are the sums
those tests compare with."""
import numpy as np

from fresnel_reference import IX, dot, unit

MAX_SURFACES, MAX_BUCKETS = 64, 65535


def finite(v):
    return np.abs(v) < np.inf  # (False for NaN)


def child(frame, t, p, j, ray_offset):
    """The children of the interfaces between rows p and their successors j (index arrays): (13, n) and e."""
    ui, ut = unit(frame[p, 12:15].T), unit(frame[j, 12:15].T)
    ni, nt = frame[p, IX["index"]], frame[j, IX["index"]]
    n = unit(np.stack([ni * ui[0] - nt * ut[0], ni * ui[1] - nt * ut[1], ni * ui[2] - nt * ut[2]]))
    twice = 2.0 * dot(ui, n)
    ur = np.stack([ui[0] - twice * n[0], ui[1] - twice * n[1], ui[2] - twice * n[2]])
    origin = np.stack([frame[p, IX[name]] + ray_offset * ur[k] for k, name in enumerate(("x1", "y1", "z1"))])
    e = frame[p, IX["intensity"]] * (t[p] - t[j])
    rays = np.zeros((13, len(p)))
    rays[0:3], rays[3], rays[4:7] = origin, 1.0, ur
    rays[9], rays[10], rays[11] = e, frame[p, IX["wavelength"]], ni
    return rays, e


def ghosts(frame, transmittance, surfaces, rays_per_group=None, n_groups=1, min_intensity=0.0, ray_offset=1e-6, id0=0.0):
    """Everything prt_frame_ghosts_count and prt_frame_ghosts_emit report: rays (13, n), parent_row, counts (per
    bucket), keys (per group: parent group, surface), bucket (of every group), stride, n_groups and the counters.
    ValueError where the definitions refuse the call."""
    frame = np.asarray(frame, dtype=np.float64)
    t = np.asarray(transmittance, dtype=np.float64)
    surfaces = [int(s) for s in surfaces]
    if not 1 <= len(surfaces) <= MAX_SURFACES or len(set(surfaces)) != len(surfaces):
        raise ValueError("1 to 64 distinct surfaces")
    n_groups = int(n_groups) if rays_per_group else 1
    n_buckets = n_groups * len(surfaces)
    if not 1 <= n_buckets <= MAX_BUCKETS:
        raise ValueError("n_groups * n_surfaces in [1, 65535]")
    n_rows = len(frame)
    generation = frame[:, IX["generation"]].astype(np.int64)
    ids = frame[:, IX["id"]]
    if n_rows and not np.all(finite(ids) & (ids == np.floor(ids)) & (ids >= id0)):
        raise ValueError("an id is not an integer")
    listed = np.array([float(s) for s in surfaces])
    mark = np.full(n_rows, -1, dtype=np.int64)
    successor = np.full(n_rows, -1, dtype=np.int64)
    counters = dict(n_spawned=0, n_dropped=0, n_dark=0, n_invalid=0, n_open=0)
    number = (ids - id0).astype(np.int64)  # (the join: per ray its row in the generation before, -1 for none)
    previous = np.full(int(number.max()) + 1 if n_rows else 0, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for g in range(int(generation.max()) + 1 if n_rows else 0):
            rows = np.flatnonzero(generation == g)
            if len(np.unique(number[rows])) != len(rows):
                raise ValueError("an id repeats within a generation")
            p = previous[number[rows]]
            if g > 0 and len(rows):
                if np.any(p < 0):
                    raise ValueError("a ray has a row in a generation and none in the one before")
                successor[p] = rows
                ni, nt = frame[p, IX["index"]], frame[rows, IX["index"]]
                match = frame[p, IX["surface"]][:, None] == listed[None, :]
                at = np.where(match.any(axis=1), match.argmax(axis=1), -1)
                refraction = (ni > 0.0) & (ni < np.inf) & (nt > 0.0) & (nt < np.inf) & (ni != nt)
                seen = (at >= 0) & refraction & finite(t[p]) & finite(t[rows])
                k = ids[rows] - id0
                group = np.floor(k / rays_per_group) if rays_per_group else np.zeros(len(rows))
                if np.any(seen & ~(group < n_groups)):
                    raise ValueError("a ray's group is not below n_groups")
                rays, e = child(frame, t, p, rows, ray_offset)
                dark = seen & (e <= 0.0)
                dropped = seen & ~dark & (e < min_intensity)
                rest = seen & ~dark & ~dropped
                good = rest & np.all(finite(rays[[0, 1, 2, 4, 5, 6, 9, 10]]), axis=0)
                counters["n_dark"] += int(dark.sum())
                counters["n_dropped"] += int(dropped.sum())
                counters["n_invalid"] += int((rest & ~good).sum())
                counters["n_spawned"] += int(good.sum())
                mark[p[good]] = group[good].astype(np.int64) * len(surfaces) + at[good]
            previous[:] = -1
            previous[number[rows]] = rows
    counters["n_open"] = int((np.isin(frame[:, IX["surface"]], listed) & (successor < 0)).sum()) if n_rows else 0
    marked = np.flatnonzero(mark >= 0)
    parent_row = marked[np.argsort(mark[marked], kind="stable")]  # (by bucket, in frame order inside a bucket)
    counts = np.bincount(mark[marked], minlength=n_buckets).astype(np.int64)
    bucket = np.flatnonzero(counts > 0)
    stride = int(counts.max()) if len(marked) else 0
    group_of = np.cumsum(counts > 0) - 1
    start = np.concatenate([[0], np.cumsum(counts)])
    with np.errstate(all="ignore"):
        rays, _ = child(frame, t, parent_row, successor[parent_row], ray_offset)
    of = mark[parent_row]
    rays[12] = group_of[of].astype(np.float64) * float(stride) + (np.arange(len(parent_row)) - start[of]).astype(np.float64)
    keys = np.stack([bucket // len(surfaces), np.array(surfaces, dtype=np.int64)[bucket % len(surfaces)]], axis=1)
    return dict(rays=rays, parent_row=parent_row, counts=counts, keys=keys.reshape(-1, 2), bucket=bucket, stride=stride,
                n_groups=len(bucket), **counters)


# ---- extended-precision sums -------------------------------------------------------------------------------------------
def last_rows(frame):
    """The row every ray ends with (a whole frame: the row of its highest generation)."""
    frame = np.asarray(frame)
    order = np.lexsort((frame[:, IX["generation"]], frame[:, IX["id"]]))
    ids = frame[order, IX["id"]]
    return order[np.concatenate([ids[1:] != ids[:-1], [True]])] if len(order) else order


def energy(values):
    """The sum of the values in longdouble."""
    return np.sum(np.asarray(values, dtype=np.longdouble), dtype=np.longdouble)


def ended_energy(frame, transmittance):
    """The energy the rays of a frame end with: the sum over rays of intensity * transmittance of the last row, every
    product exact in longdouble (two 53-bit factors, 64 bits of mantissa hold the leading part; the rest is below
    2^-64 of the term)."""
    rows = last_rows(frame)
    return energy(np.asarray(frame)[rows, IX["intensity"]].astype(np.longdouble) * np.asarray(transmittance)[rows].astype(np.longdouble))


def interfaces_per_ray(frame):
    """The largest number of interfaces of a ray: its rows - 1."""
    frame = np.asarray(frame)
    return int(np.bincount((frame[:, IX["id"]] - frame[:, IX["id"]].min()).astype(np.int64)).max()) - 1 if len(frame) else 0
