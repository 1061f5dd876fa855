"""A numpy restatement of the scatter definitions of include/prt.h, operation for operation: every product and sum is
one numpy ufunc call (rounded on its own, as the kernel's are under -ffp-contract=off), dot products as
(x x' + y y') + z z', in the order csrc/prt_scatter.hpp writes them.  Philox4x32-10 is integer arithmetic on uint64
arrays; the surface normal follows the trace's world_normal_len, whose 4x4 products are fma chains: ``fma`` below is an
exact fused multiply-add built from error-free transformations and one rounding to odd (Boldo & Melquiond 2008), checked
against rational arithmetic by tests/test_host_scatter.py.  It works on a frame given as (R, 15) and a surface table
``id -> (type, normal_scale, params[6], minv[16])``.  tests/test_host_scatter.py checks it against the published
known-answer vectors and closed forms; tests/test_gpu_scatter.py holds the device to its bits."""
import numpy as np

from fresnel_reference import IX, dot, unit

KNOTS, MAX_MODELS, MAX_SURFACES, MAX_BUCKETS, MAX_RAYS_PER_HIT = 1024, 16, 64, 65535, 64
SPHERE, CYLINDER, PLANE, CUBE, PARABOLOID = range(5)
COUNTERS = ("n_spawned", "n_rejected", "n_below", "n_dark", "n_dropped", "n_invalid")
_M0, _M1, _W0, _W1, _MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_32 = np.uint64(32)


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------
def philox(counter, key):
    """The four output words of every counter (n, 4) under key (2,): uint64 arrays that hold 32-bit values."""
    c = [np.asarray(counter, dtype=np.uint64)[:, k] & _MASK for k in range(4)]
    k0, k1 = (np.uint64(int(v)) & _MASK for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # (32 x 32 bits: no overflow in 64)
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=1)


def uniform(hi, lo):
    """(((hi << 32) | lo) >> 11) * 2^-53, in [0, 1)."""
    return (((hi << _32) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def samples(ids, generations, children, seed):
    """(a, b) in [-1, 1) of the items."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    counter = np.stack([ids & _MASK, ids >> _32, np.asarray(generations, dtype=np.int64).astype(np.uint64) & _MASK,
                        np.asarray(children, dtype=np.uint64)], axis=1)
    x = philox(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return 2.0 * uniform(x[:, 0], x[:, 1]) - 1.0, 2.0 * uniform(x[:, 2], x[:, 3]) - 1.0


# ---- an exact fused multiply-add -------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """round(a b + c) with one rounding, element by element (finite operands away from over- and underflow): the exact
    product as a sum of two doubles, the exact sum of its leading part and c, the two small parts added with rounding
    to odd, and one last addition."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, p)
    s, err = _two_sum(tl, e)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    v = np.where((err != 0) & even, nudged, s)
    return np.where(v == 0, th, th + v)  # (nothing left to add: th is c + a b exactly, with the sign of a zero sum)


def _row_dot(m, r, x, y, z, w):
    return fma(m[4 * r + 3], w, fma(m[4 * r + 2], z, fma(m[4 * r + 1], y, m[4 * r] * x)))


def _col_dot(m, r, x, y, z):
    return fma(m[12 + r], 0.0, fma(m[8 + r], z, fma(m[4 + r], y, m[r] * x)))


def _close(a, b):
    return np.abs(a - b) <= 1e-8 + 1e-5 * np.abs(b)


def world_normal(entry, x):
    """The world normal times normal_scale at the world points x (3, n), as world_normal_len of csrc/prt_device.hpp."""
    kind, scale, q, m = entry
    m = np.asarray(m, dtype=np.float64).reshape(16)
    with np.errstate(all="ignore"):  # (0 / 0 where a point has no normal, as upstream)
        return _world_normal(kind, scale, q, m, x)


def _world_normal(kind, scale, q, m, x):
    one = np.ones(x.shape[1])
    lx, ly, lz = (_row_dot(m, r, x[0], x[1], x[2], one) for r in range(3))
    zero = np.zeros_like(lx)
    normalise = True
    if kind == SPHERE:
        ax, ay, az = lx, ly, lz
    elif kind == CYLINDER:
        low, high = _close(lz, q[1]), _close(lz, q[2])
        cap = low | high
        ax, ay = np.where(cap, 0.0, lx), np.where(cap, 0.0, ly)
        az = np.where(high, 1.0, np.where(low, -1.0, 0.0))
    elif kind == PLANE:
        ax, ay, az, normalise = zero, zero, zero + 1.0, False
    elif kind == CUBE:
        ax, ay, az = (np.where(_close(l, q[2 * k + 1]), 1.0, np.where(_close(l, q[2 * k]), -1.0, 0.0))
                      for k, l in enumerate((lx, ly, lz)))
    elif kind == PARABOLOID:
        cap = _close(lz, q[1])
        ax, ay, az = np.where(cap, 0.0, lx), np.where(cap, 0.0, ly), np.where(cap, 1.0, -2 * q[0] + zero)
    else:
        raise ValueError(kind)
    if normalise:
        length = np.sqrt(((ax * ax + ay * ay) + az * az) + 0.0 * 0.0)
        ax, ay, az = ax / length, ay / length, az / length
    wx, wy, wz = (_col_dot(m, r, ax, ay, az) for r in range(3))
    length = np.sqrt(((wx * wx + wy * wy) + wz * wz) + 0.0 * 0.0)
    return np.stack([wx / length, wy / length, wz / length]) * float(scale)


def table_of(prims):
    return {int(p["surface_id"]): (int(p["type"]), int(p["normal_scale"]), np.array(p["params"], dtype=float),
                                   np.array(p["minv"], dtype=float).reshape(16)) for p in prims}


# ---- the pieces ------------------------------------------------------------------------------------------------------
def basis(n):
    """(t1, t2) of the unit vectors n (3, k)."""
    sign = np.copysign(1.0, n[2])
    a = -1.0 / (sign + n[2])
    b = (n[0] * n[1]) * a
    sx = sign * n[0]
    return np.stack([1.0 + (sx * n[0]) * a, sign * b, -sx]), np.stack([b, sign + (n[1] * n[1]) * a, -n[1]])


def lookup(table, b):
    """The table's value at b; NaN where b is not a number."""
    with np.errstate(invalid="ignore"):
        q = np.sqrt(0.5 * b) * float(KNOTS)
    bad = ~(q >= 0.0)
    k = np.where(bad, 0.0, np.where(q < KNOTS - 1, q, KNOTS - 1)).astype(np.int64)
    lo = table[k]
    f = lo + (q - k.astype(np.float64)) * (table[k + 1] - lo)
    return np.where(bad, np.nan, f)


def finite(v):
    return np.abs(v) < np.inf  # (False for NaN)


def target_of(centre, normal, radius):
    """The 13 doubles of a target disk: centre, unit normal, its basis, radius."""
    normal = np.asarray(normal, dtype=np.float64)
    normal = normal / float(np.sqrt(np.sum(normal * normal)))
    e1, e2 = basis(normal.reshape(3, 1))
    return np.concatenate([np.asarray(centre, dtype=np.float64), normal, e1[:, 0], e2[:, 0], [float(radius)]])


def children(frame, p, c, at, surfaces, table, models, tables, target, rays_per_hit, seed, ray_offset):
    """Child c of row p on listed surface number `at` (index arrays): (fate per item, rays (13, n)); fates: 0 not decided
    yet, 1 rejected, 2 below."""
    n_items = len(p)
    a, b = samples(frame[p, IX["id"]], frame[p, IX["generation"]], c, seed)
    s = a * a + b * b
    fate = np.where(s < 1.0, 0, 1)
    x = frame[p, 9:12].T
    ui = unit(frame[p, 12:15].T)
    rows, item_row = np.unique(p, return_inverse=True)  # (the normal is the row's: once a row, not once a child)
    row_at = np.zeros(len(rows), dtype=np.int64)
    row_at[item_row] = at
    row_n = np.full((3, len(rows)), np.nan)
    for k, sid in enumerate(surfaces):
        here = row_at == k
        if here.any():
            row_n[:, here] = world_normal(table[int(sid)], frame[rows[here], 9:12].T)
    n = row_n[:, item_row]
    n = np.where(dot(n, ui) > 0.0, -n, n)
    intensity = frame[p, IX["intensity"]]
    if target is not None:
        centre, normal, e1, e2, radius = target[0:3], target[3:6], target[6:9], target[9:12], target[12]
        y = np.stack([centre[k] + radius * (a * e1[k] + b * e2[k]) for k in range(3)])
        v = y - x
        r2 = dot(v, v)
        uo = v / np.sqrt(r2)
        cos_o = dot(n, uo)
        fate = np.where((fate == 0) & (cos_o <= 0.0), 2, fate)
        cos_t = np.abs(dot(normal.reshape(3, 1) + np.zeros((3, n_items)), uo))
    else:
        cz = np.sqrt(1.0 - s)
        fate = np.where((fate == 0) & ~(cz > 0.0), 1, fate)
        t1, t2 = basis(n)
        uo = (a * t1 + b * t2) + cz * n
    d = uo - ui
    dn = dot(d, n)
    across = d - dn * n
    beta = np.sqrt(dot(across, across))
    f = np.full(n_items, np.nan)
    for number in set(models):
        here = np.isin(at, [k for k, m in enumerate(models) if m == number])
        f[here] = lookup(tables[number], beta[here])
    if target is not None:
        e = ((((intensity * f) * cos_o) * cos_t) * (4.0 * (radius * radius))) / (float(rays_per_hit) * r2)
    else:
        e = ((4.0 * intensity) * f) / float(rays_per_hit)
    rays = np.zeros((13, n_items))
    rays[0:3], rays[3], rays[4:7] = x + ray_offset * uo, 1.0, uo
    rays[9], rays[10], rays[11] = e, frame[p, IX["wavelength"]], frame[p, IX["index"]]
    return fate, rays


def scatter(frame, table, surfaces, models, tables, target=None, rays_per_hit=1, seed=0, rays_per_group=None, n_groups=1,
            min_intensity=0.0, ray_offset=1e-6):
    """Everything prt_frame_scatter_count and prt_frame_scatter_emit report: rays (13, n), parent_row, child, counts (per
    bucket), keys (per group: parent group, surface), bucket, stride, n_groups and the counters.  ``models``: per listed
    surface the number of its table in ``tables`` (n_models, 1025).  ValueError where the definitions refuse the call."""
    frame = np.asarray(frame, dtype=np.float64)
    surfaces = [int(s) for s in surfaces]
    tables = np.asarray(tables, dtype=np.float64).reshape(-1, KNOTS + 1)
    if not 1 <= len(surfaces) <= MAX_SURFACES or len(set(surfaces)) != len(surfaces):
        raise ValueError("1 to 64 distinct surfaces")
    if not 1 <= rays_per_hit <= MAX_RAYS_PER_HIT or len(frame) * rays_per_hit >= 2 ** 31 - 1:
        raise ValueError("1 to 64 rays a hit, rows x rays a hit below 2^31")
    if not 1 <= len(tables) <= MAX_MODELS or not np.all(finite(tables) & (tables >= 0.0)):
        raise ValueError("1 to 16 tables, finite and >= 0")
    if len(models) != len(surfaces) or not all(0 <= m < len(tables) for m in models):
        raise ValueError("a surface's model is not in [0, n_models)")
    if any(s not in table for s in surfaces):
        raise ValueError("a listed surface is not in the surface table")
    if target is not None:
        target = np.asarray(target, dtype=np.float64)
        if not (np.all(finite(target)) and target[12] > 0.0 and abs(dot(target[3:6], target[3:6]) - 1.0) <= 1e-12):
            raise ValueError("the target: finite, radius > 0, a unit normal")
    n_groups = int(n_groups) if rays_per_group else 1
    n_buckets = n_groups * len(surfaces)
    if not 1 <= n_buckets <= MAX_BUCKETS:
        raise ValueError("n_groups * n_surfaces in [1, 65535]")
    listed = np.array([float(s) for s in surfaces])
    match = frame[:, IX["surface"]][:, None] == listed[None, :] if len(frame) else np.zeros((0, len(listed)), dtype=bool)
    rows = np.flatnonzero(match.any(axis=1))
    ids, generations = frame[rows, IX["id"]], frame[rows, IX["generation"]]
    if not np.all((ids >= 0) & (ids < 2.0 ** 53) & (ids == np.floor(ids)) & (generations >= 0) & (generations < 2.0 ** 31) &
                  (generations == np.floor(generations))):
        raise ValueError("an id or a generation of a row on a listed surface is not an integer >= 0")
    group = np.floor(ids / rays_per_group) if rays_per_group else np.zeros(len(rows))
    if np.any(~(group < n_groups)):
        raise ValueError("a ray's group is not below n_groups")
    p = np.repeat(rows, rays_per_hit)
    c = np.tile(np.arange(rays_per_hit), len(rows))
    at = np.repeat(match[rows].argmax(axis=1), rays_per_hit)
    with np.errstate(all="ignore"):
        fate, rays = children(frame, p, c, at, surfaces, table, models, tables, target, rays_per_hit, seed, ray_offset)
        e = rays[9]
        open_ = fate == 0
        dark = open_ & (e <= 0.0)
        dropped = open_ & ~dark & (e < min_intensity)
        rest = open_ & ~dark & ~dropped
        good = rest & np.all(finite(rays[[0, 1, 2, 4, 5, 6, 9, 10, 11]]), axis=0)
    counters = dict(n_spawned=int(good.sum()), n_rejected=int((fate == 1).sum()), n_below=int((fate == 2).sum()),
                    n_dark=int(dark.sum()), n_dropped=int(dropped.sum()), n_invalid=int((rest & ~good).sum()))
    mark = np.repeat(group, rays_per_hit).astype(np.int64) * len(surfaces) + at
    kept = np.flatnonzero(good)  # (in item order: row, then child)
    order = kept[np.argsort(mark[kept], kind="stable")]
    counts = np.bincount(mark[kept], minlength=n_buckets).astype(np.int64)
    bucket = np.flatnonzero(counts > 0)
    stride = int(counts.max()) if len(kept) else 0
    group_of = np.cumsum(counts > 0) - 1
    start = np.concatenate([[0], np.cumsum(counts)])
    out = rays[:, order]
    of = mark[order]
    out[12] = group_of[of].astype(np.float64) * float(stride) + (np.arange(len(order)) - start[of]).astype(np.float64)
    keys = np.stack([bucket // len(surfaces), np.array(surfaces, dtype=np.int64)[bucket % len(surfaces)]], axis=1)
    return dict(rays=out, parent_row=p[order], child=c[order], counts=counts, keys=keys.reshape(-1, 2), bucket=bucket,
                stride=stride, n_groups=len(bucket), **counters)


# ---- the estimators' sums and their standard errors -------------------------------------------------------------------
def estimate(energies, n_rows, rays_per_hit):
    """(sum of the children's energies per parent row, its standard error): the items of a row are independent draws of
    E (0 for an item without a child), so the sum over n_rows * rays_per_hit items has the variance items * var(E)."""
    items = n_rows * rays_per_hit
    e = np.zeros(items, dtype=np.longdouble)
    e[:len(energies)] = np.asarray(energies, dtype=np.longdouble)
    total = e.sum()
    variance = (np.sum(e * e) - total * total / items) / (items - 1)
    return float(total / n_rows), float(np.sqrt(variance * items) / n_rows)
