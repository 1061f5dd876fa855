"""References and error bounds for the ray-aberration pass of prt_aberrations.hpp (prt_frame_launch_index,
prt_frame_ray_aberrations), with Python copies of its partition rules and the frames the tests run on.  It extends
tests/frame_sums_reference.py (``gamma``, ``Err``, ``require_exact``, the Zernike recurrence); frames are (R, 15) float64
arrays as there.

1. The partition (``ab_waves`` .. ``ab_tiles``), from (n_rows, n_groups, n_zones): the rows are cut into waves as the
   wavefront's are, cut again so that the (wave, bucket) counts fit kAbCountBytes, a bucket being a (group, zone); the
   waves' counts are scanned by one workgroup of kSortScanBlock threads (``ab_scan_per`` items a thread); a bucket is cut
   into chunks of kMtfChunk rays, a chunk summed in tiles of kAbBlock.  tests/test_host_aberration_sums.py holds the
   named constants and the restated lines to the headers' text.

2. Exact sums (``integer_aberrations``).  On a dyadic frame (``dyadic_rows``) -- end and start points multiples of 2^-8
   within +-2, directions (1, t, m 2^-8) with t one of +-1, +-1/2, +-1/4, 0, weights in {0, 1, 2, 4}, the default axes, a
   launch origin and a given reference on the grid, pupil_radius a power of two -- h, p, eps, s and la of every ray are
   exact in fp64, and every term of every sum (w, w eps, w s, w |eps|^2, w eps.s, w |s|^2, w la, w la^2, w Q) is an
   integer in units of 2^-8 or 2^-16.  While the absolute values add up to less than 2^53 units (``require_exact``: a
   condition, not a tolerance) the device's additions are exact in any order and the outputs equal the integers' bit for
   bit.  Z_1 = 1 exactly, so the six entries of ``normal`` at one term are such sums too.  The zone of a ray,
   floor(|p| n_zones), is taken from integers (``isqrt``) and the float64 expression is asserted to agree.

3. Bounds (``bounded_aberrations``), u = 2^-53, gamma(k) = k u / (1 - k u).  The per-ray chain (h, p, eps, s, la, the
   Zernike basis by the device's recurrence) is evaluated in longdouble with the running bound ``Err`` keeps of the
   device's own operation sequence.  The sums of k_mtf_centre<AbRaw> / k_aberration_stage move a term through at most
   ceil(kMtfChunk / kAbBlock) = 16 additions in its thread, 8 in the tree of 256, and one per chunk of the group in the
   serial fold (of the bucket, for a zone's sums): ``stage_depth``.  k_aberration_normal adds an entry over a chunk's rays
   in series, then the fold: ``normal_depth`` = the rays of the group's largest chunk + its chunks.  A sum is then off by
   at most gamma(depth) (sum |t| + sum e) + sum e, e the terms' own running bounds; for the normal equations these are the
   basis-evaluation terms that frame_sums_reference.wavefront_reference derives, with two products a term.
   centre (centroid): N = sum w Q by fma (depth + 1), D = sum w, C = fl(N~ / D~):
        |C~ - C| <= (gamma(depth + 1) sum |w Q| + |C| gamma(depth) sum w) / (D - gamma(depth) D) + u |C|
   rho (from the extent): the largest running bound of sqrt(h1^2 + h2^2) over the group's rays (|max a~ - max a| <=
   max |a~ - a|).  The per-ray chain and the sums then take the device's C and rho as their inputs, as
   k_aberration_stage does.  Coefficients: the perturbation bound of the normal equations, as for the wavefront.
   Every bound carries the factor 1.001 for the terms of second order.

Largest deviation-to-bound ratios seen on an MI355X (tests/test_gpu_aberration_partitions.py prints them; none is fixed
in advance):
    centroid 0.016, rho 0.087, p 0.59, eps 0.59, s 0.55, la 0.92 (three roundings, each near half an ulp), group sums
    0.035, zone sums 0.12, normal equations 0.086 (0.012 at 21 / 36 terms), coefficients 0.00046
The sums on dyadic frames have no ratio: they are equal or the test fails.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import frame_sums_reference as ref
from frame_sums_reference import IX, LD, SECOND_ORDER, U, Err, Fp64, NotExact, gamma, require_exact  # noqa: F401

ROOT = ref.ROOT
DEFAULT_AXES = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])

# ---- named copies of the constants (test_host_aberration_sums.py holds them to the headers) ---------------------------
AB_BLOCK = 256                  # prt_aberrations.hpp: static const int kAbBlock = 256;
AB_COUNT_BYTES = 64 << 20       # prt_aberrations.hpp: static const size_t kAbCountBytes = 64u << 20;
MTF_CHUNK = 4096                # prt_mtf.hpp: static const int kMtfChunk = 4096;
MTF_SCAN_BLOCK = 512            # prt_sort.hpp: static const int kSortScanBlock = 512;
WF_MAX_WAVES = ref.WF_MAX_WAVES
WF_ROWS_PER_WAVE = ref.WF_ROWS_PER_WAVE
BLOCK = ref.BLOCK
HEADER_NAMES = dict(kAbBlock="AB_BLOCK", kAbCountBytes="AB_COUNT_BYTES", kMtfChunk="MTF_CHUNK",
                    kSortScanBlock="MTF_SCAN_BLOCK", kWfMaxWaves="WF_MAX_WAVES", kWfRowsPerWave="WF_ROWS_PER_WAVE")
HOST_RULES = {
    "prt_aberrations.hpp": (
        "const SortPlan plan = sort_plan(n_rows, n_buckets, 8, kAbCountBytes);",
        "const int n_buckets = n_groups * nz;",
        "for (int64_t r = lo + t; r < hi; r += kAbBlock) {",
        "__shared__ double red[AB_SUMS][kAbBlock];",
        "for (int64_t q = chunk_start[g * nz]; q < chunk_start[(g + 1) * nz]; ++q) v += sums_slab[(size_t)q * AB_SUMS + k];",
        "for (int64_t q = chunk_start[b]; q < chunk_start[b + 1]; ++q) v += sums_slab[(size_t)q * AB_SUMS + k];",
        "for (int k = 0; k < rays_here; ++k) {"),
    "prt_sort.hpp": (
        "int64_t waves = (n_rows + kWfRowsPerWave - 1) / kWfRowsPerWave;",
        "waves = std::min<int64_t>(std::max<int64_t>(waves, 1), kWfMaxWaves);",
        "waves = std::max<int64_t>(1, std::min<int64_t>(waves, (int64_t)(cap_bytes / ((size_t)buckets * cell_bytes))));",
        "const int64_t per_wave = ((n_rows + waves - 1) / waves + 63) / 64 * 64;",
        "const unsigned grid = (unsigned)((waves + PRT_BLOCK / 64 - 1) / (PRT_BLOCK / 64));",
        "const int64_t all_waves = (int64_t)grid * (PRT_BLOCK / 64);",
        "const int64_t per = (n + kSortScanBlock - 1) / kSortScanBlock;",
        "for (int half = BLOCK / 2; half > 0; half >>= 1) {"),
    "prt_mtf.hpp": (
        "n_groups, [&](int64_t g) { return (bucket_total[g] + kMtfChunk - 1) / kMtfChunk; },",
        "hi = lo + kMtfChunk < end ? lo + kMtfChunk : end;"),
    "prt_wavefront.hpp": (),
}


def header_constants():
    """The static const ints of the four headers, by name."""
    found = {}
    for name in HOST_RULES:
        text = open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read()
        for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
            try:
                found[key] = int(eval(re.sub(r"(\d+)u\b", r"\1", value), {"__builtins__": {}}, {}))
            except (NameError, SyntaxError, TypeError):
                pass  # (not a plain constant)
    return found


# ---- 1. the partition rules -------------------------------------------------------------------------------------------
def ab_buckets(n_groups, n_zones):
    return n_groups * max(n_zones, 1)


def ab_waves(n_rows, n_groups, n_zones):
    waves = min(max(-(-n_rows // WF_ROWS_PER_WAVE), 1), WF_MAX_WAVES)
    return max(1, min(waves, AB_COUNT_BYTES // (ab_buckets(n_groups, n_zones) * 8)))


def ab_per_wave(n_rows, n_groups, n_zones):
    return (-(-n_rows // ab_waves(n_rows, n_groups, n_zones)) + 63) // 64 * 64


def ab_all_waves(n_rows, n_groups, n_zones):
    """The waves the launch holds: whole workgroups of PRT_BLOCK / 64 (the ones past the rows count nothing)."""
    return -(-ab_waves(n_rows, n_groups, n_zones) // (BLOCK // 64)) * (BLOCK // 64)


def ab_scan_per(n_rows, n_groups, n_zones):
    """The waves one thread of sort_scan owns in k_sort_positions / k_sort_offsets."""
    return -(-ab_all_waves(n_rows, n_groups, n_zones) // MTF_SCAN_BLOCK)


def ab_bucket_scan_per(n_groups, n_zones):
    """The buckets one thread of sort_scan owns in k_mtf_starts."""
    return -(-ab_buckets(n_groups, n_zones) // MTF_SCAN_BLOCK)


def ab_chunks(n_rays):
    """The chunks of a bucket of n_rays (an array of buckets: per bucket)."""
    return -(-np.asarray(n_rays) // MTF_CHUNK)


def ab_tiles(n_rays):
    """The LDS tiles of a bucket's last (or only) chunk."""
    last = n_rays - (int(ab_chunks(n_rays)) - 1) * MTF_CHUNK if n_rays else 0
    return -(-last // AB_BLOCK)


def stage_depth(chunks):
    return -(-MTF_CHUNK // AB_BLOCK) + int(math.log2(AB_BLOCK)) + int(chunks)


def normal_depth(largest_chunk, chunks):
    return int(largest_chunk) + int(chunks)


# ---- the join and the selection -----------------------------------------------------------------------------------------
def join(frame):
    """Per row the number of the generation-0 row with the same id, -1 without one: a dictionary."""
    launch_rows = np.flatnonzero(frame[:, IX["generation"]] == 0)
    table = dict(zip(frame[launch_rows, IX["id"]].tolist(), launch_rows.tolist()))
    assert len(table) == len(launch_rows), "an id repeats within generation 0"
    return np.fromiter((table.get(ray_id, -1) for ray_id in frame[:, IX["id"]].tolist()), dtype=np.int64,
                       count=len(frame))


def _dot(v, e):
    return v[0] * float(e[0]) + v[1] * float(e[1]) + v[2] * float(e[2])   # (ab_dot: left to right)


def used_rays(frame, index, group, pupil, origin, axes, weights):
    """The rows with ``group`` >= 0 that the definitions keep (include/prt.h): the rest count in n_missed."""
    a = axes[0:3]
    launch = frame[np.maximum(index, 0)]
    q, u = frame[:, 9:12], frame[:, 12:15]
    w = np.ones(len(frame)) if weights is None else frame[:, IX[weights]]
    with np.errstate(all="ignore"):
        ua = _dot(u.T, a)
        s = np.stack([_dot(u.T, axes[3:6]) / ua, _dot(u.T, axes[6:9]) / ua], 1)
        if pupil == "position":
            d = launch[:, 6:9] - np.asarray(origin, dtype=float)
            h = np.stack([_dot(d.T, axes[3:6]), _dot(d.T, axes[6:9])], 1)
            needed = np.isfinite(d).all(1)
        else:
            v = launch[:, 12:15]
            va = _dot(v.T, a)
            h = np.stack([_dot(v.T, axes[3:6]) / va, _dot(v.T, axes[6:9]) / va], 1)
            needed = np.isfinite(v).all(1) & (va != 0)
    ok = (index >= 0) & np.isfinite(q).all(1) & np.isfinite(u).all(1) & (ua != 0) & np.isfinite(s).all(1) & needed
    ok &= np.isfinite(h).all(1) & np.isfinite(w) & (w >= 0)
    return ok & (group >= 0)


# ---- 2. exact sums on a dyadic grid ---------------------------------------------------------------------------------------
GRID = 256  # 2^8
TILTS = (1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.0)
WEIGHTS = (0.0, 1.0, 2.0, 4.0)


def dyadic_rows(generation, ids, surface, rng):
    """Rows of one generation on the grid: points multiples of 2^-8 within +-2, directions (1, t, m 2^-8) with t from
    ``TILTS``, intensity from ``WEIGHTS`` (zero for one row in eight), wavelength on the grid in (0, 2), index 1."""
    n = len(ids)
    rows = np.zeros((n, 15))
    rows[:, IX["generation"]], rows[:, IX["id"]], rows[:, IX["surface"]], rows[:, IX["index"]] = generation, ids, surface, 1.0
    rows[:, 6:12] = rng.integers(-2 * GRID + 1, 2 * GRID, (n, 6)) / GRID
    rows[:, IX["x_tilt"]] = 1.0
    rows[:, IX["y_tilt"]] = rng.choice(TILTS, n, p=(0.2, 0.2, 0.15, 0.15, 0.1, 0.1, 0.1))
    rows[:, IX["z_tilt"]] = rng.integers(-2 * GRID + 1, 2 * GRID, n) / GRID
    rows[:, IX["intensity"]] = rng.choice(WEIGHTS, n, p=(0.125, 0.375, 0.25, 0.25))
    rows[:, IX["wavelength"]] = rng.integers(1, 2 * GRID, n) / GRID
    return rows


def dyadic_aberration_frame(launch_ids, middle_ids, selected_ids, seed, surfaces=(1.0, 2.0, 5.0)):
    """Three generations on the grid: launch rows, an intermediate surface, the selected surface."""
    rng = np.random.default_rng(seed)
    return np.concatenate([dyadic_rows(g, np.asarray(ids, dtype=np.float64), surfaces[g], rng)
                           for g, ids in enumerate((launch_ids, middle_ids, selected_ids))])


def _units(values, what, unit=GRID):
    return ref.to_grid(values, what, unit)


def _power_of_two(x):
    return x > 0 and math.frexp(x)[0] == 0.5


def _isqrt(values):
    """floor(sqrt(v)) of non-negative int64, exactly."""
    root = np.floor(np.sqrt(values.astype(np.float64))).astype(np.int64)
    root -= root * root > values
    root += (root + 1) * (root + 1) <= values
    assert np.all(root * root <= values) and np.all((root + 1) * (root + 1) > values)
    return root


def _sum_by(columns, key, n):
    """Per key in [0, n) the int64 sums of the columns: (n, len(columns))."""
    out = np.zeros((n, len(columns)), dtype=np.int64)
    if len(key):
        order = np.argsort(key, kind="stable")
        sorted_key = key[order]
        starts = np.flatnonzero(np.r_[True, sorted_key[1:] != sorted_key[:-1]])
        out[sorted_key[starts]] = np.add.reduceat(np.stack(columns, 1)[order], starts, axis=0)
    return out


def integer_aberrations(frame, surface=None, generation=None, pupil="position", origin=(0.0, 0.0, 0.0),
                        reference=(0.0, 0.0, 0.0), pupil_radius=1.0, zones=64, weights=None, rays_per_source=None,
                        n_groups=1, index=None):
    """prt_frame_ray_aberrations on a dyadic frame from integers (default axes; reference: given points or "chief";
    pupil_radius a power of two).  Per group: n_rays, n_missed, n_la, chief (-1: none), centre, sums (the record's slots
    8..15), normal (the six entries at one term), zones (n_zones, 6), buckets (the rays per (group, zone)); over all
    groups in row order: rows and rays (p1, p2, eps1, eps2, s1, s2, la)."""
    if not _power_of_two(pupil_radius):
        raise ValueError("pupil_radius: a power of two")
    index = join(frame) if index is None else index
    group = ref.selection(frame, surface, generation, rays_per_source, n_groups)
    used = used_rays(frame, index, group, pupil, origin, DEFAULT_AXES, weights)
    rows = np.flatnonzero(used)
    g = group[rows]
    launch = frame[index[rows]]
    if pupil == "position":
        o = _units(origin, "launch_origin")
        h = np.stack([_units(launch[:, IX["y0"]], "y0") - o[1], _units(launch[:, IX["z0"]], "z0") - o[2]], 1)
    else:
        if not np.all(launch[:, IX["x_tilt"]] == 1.0):
            raise ValueError("launch directions: (1, k 2^-8, m 2^-8)")
        h = np.stack([_units(launch[:, IX["y_tilt"]], "y_tilt"), _units(launch[:, IX["z_tilt"]], "z_tilt")], 1)
    hh = h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]
    n_rays, n_missed = np.bincount(g, minlength=n_groups), np.bincount(group[(group >= 0) & ~used], minlength=n_groups)
    # the chief ray: the smallest row among those with the smallest |h|^2 (rows ascend: the first of them)
    chief = np.full(n_groups, -1, dtype=np.int64)
    order = np.lexsort((rows, hh, g))
    first = np.flatnonzero(np.r_[True, g[order][1:] != g[order][:-1]]) if len(rows) else np.zeros(0, dtype=np.int64)
    chief[g[order][first]] = rows[order][first]
    q = np.stack([_units(frame[rows, IX[name]], name) for name in ("x1", "y1", "z1")], 1)
    if isinstance(reference, str):
        assert reference == "chief", "the centroid is not exact: bounded_aberrations"
        centre = np.full((n_groups, 3), np.nan)
        centre[chief >= 0] = frame[chief[chief >= 0], 9:12]
    else:
        centre = np.broadcast_to(np.asarray(reference, dtype=np.float64), (n_groups, 3)).copy()
    c = np.zeros((n_groups, 3), dtype=np.int64)
    c[n_rays > 0] = _units(centre[n_rays > 0], "reference")
    if not np.all(frame[rows, IX["x_tilt"]] == 1.0) or not np.all(np.isin(frame[rows, IX["y_tilt"]], TILTS)):
        raise ValueError("directions: (1, t, m 2^-8), t one of +-1, +-1/2, +-1/4, 0")
    eps = q[:, 1:3] - c[g, 1:3]
    s = np.stack([_units(frame[rows, IX["y_tilt"]], "y_tilt"), _units(frame[rows, IX["z_tilt"]], "z_tilt")], 1)
    tilt = frame[rows, IX["y_tilt"]]
    fin = tilt != 0
    inverse = np.zeros(len(rows), dtype=np.int64)
    inverse[fin] = (1.0 / tilt[fin]).astype(np.int64)
    la = _units(frame[rows, IX["x0"]], "x0") - _units(frame[rows, IX["y0"]], "y0") * inverse   # (x_tilt = 1)
    w = np.ones(len(rows), dtype=np.int64) if weights is None else _units(frame[rows, IX[weights]], weights, 1)
    ee, es, ss = (eps * eps).sum(1), (eps * s).sum(1), (s * s).sum(1)
    columns = [w, w * eps[:, 0], w * eps[:, 1], w * s[:, 0], w * s[:, 1], w * ee, w * es, w * ss,
               fin.astype(np.int64), w * fin, w * la * fin, w * la * la * fin, np.ones(len(rows), dtype=np.int64)]
    require_exact(columns + [w * q[:, 0], w * q[:, 1], w * q[:, 2]])
    # zones from integers: floor(sqrt(hh) n_zones / (rho GRID)); the float64 expression has to agree
    nz = max(zones, 1)
    rho_units = pupil_radius * GRID
    zone = np.zeros(len(rows), dtype=np.int64)
    if zones:
        if rho_units >= 1:
            zone = _isqrt(hh * nz * nz) // int(rho_units)
        else:
            zone = _isqrt(hh * nz * nz * int(1 / rho_units) ** 2)
        zone = np.minimum(zone, nz - 1)
        p64 = h / GRID / pupil_radius
        as_device = np.minimum(np.floor(np.sqrt(p64[:, 0] * p64[:, 0] + p64[:, 1] * p64[:, 1]) * zones), zones - 1)
        assert np.array_equal(as_device.astype(np.int64), zone), "a ray on a zone's edge within rounding"
    per_bucket = _sum_by(columns, g * nz + zone, n_groups * nz)
    per_group = per_bucket.reshape(n_groups, nz, -1).sum(1)
    unit = np.array([1.0, 1 / GRID, 1 / GRID, 1 / GRID, 1 / GRID, GRID ** -2.0, GRID ** -2.0, GRID ** -2.0,
                     1.0, 1.0, 1 / GRID, GRID ** -2.0, 1.0])
    sums = per_group.astype(np.float64) * unit   # (below 2^53: exact, and the units are powers of two)
    zone_sums = (per_bucket.astype(np.float64) * unit).reshape(n_groups, nz, -1)[:, :, [12, 9, 10, 11, 5, 8]]
    rays = np.stack([h[:, 0] / GRID / pupil_radius, h[:, 1] / GRID / pupil_radius, eps[:, 0] / GRID, eps[:, 1] / GRID,
                     s[:, 0] / GRID, s[:, 1] / GRID, np.where(fin, la / GRID, np.nan)], 1)
    return SimpleNamespace(rows=rows, rays=rays, group=g, n_rays=n_rays, n_missed=n_missed, chief=chief, centre=centre,
                           n_la=per_group[:, 8], sums=sums[:, 0:8], normal=sums[:, [0, 1, 2, 3, 4, 0]],
                           zones=zone_sums if zones else np.zeros((n_groups, 0, 6)),
                           buckets=per_bucket[:, 12].reshape(n_groups, nz), zone=zone)


# ---- 3. longdouble with running bounds ----------------------------------------------------------------------------------------
def ray_chain(kind, frame, rows, launch_rows, pupil, origin, axes, weights):
    """ab_ray's operation sequence on ``kind`` values (Err: longdouble and a running bound; Fp64: the same in float64)
    for the rows ``rows`` with launch rows ``launch_rows``: h, |h|, s, la (inf / NaN without one), w, q."""
    col = lambda name, at: kind(frame[at, IX[name]])  # noqa: E731
    a, e1, e2 = axes[0:3], axes[3:6], axes[6:9]
    with np.errstate(all="ignore"):
        if pupil == "position":
            d = [col(name, launch_rows) - float(o) for name, o in zip(("x0", "y0", "z0"), origin)]
            h1, h2 = _dot(d, e1), _dot(d, e2)
        else:
            v = [col(name, launch_rows) for name in ("x_tilt", "y_tilt", "z_tilt")]
            va = _dot(v, a)
            h1, h2 = _dot(v, e1) / va, _dot(v, e2) / va
        u = [col(name, rows) for name in ("x_tilt", "y_tilt", "z_tilt")]
        ua = _dot(u, a)
        s1, s2 = _dot(u, e1) / ua, _dot(u, e2) / ua
        la = col("x0", rows) - col("x_tilt", rows) * col("y0", rows) / col("y_tilt", rows)
    hh = h1 * h1 + h2 * h2
    w = kind(np.ones(len(rows)) if weights is None else frame[rows, IX[weights]])
    return SimpleNamespace(h1=h1, h2=h2, hh=hh, radius=hh.sqrt(), s1=s1, s2=s2, la=la, w=w,
                           q=[col(name, rows) for name in ("x1", "y1", "z1")])


def stage_chain(kind, ray, g, centre, rho, axes):
    """ab_out and the twelve terms of k_aberration_stage from the device's centre (n_groups, 3) and rho (n_groups):
    p, eps, the terms (a list of twelve ``kind``) and which rays have a finite la."""
    d = [ray.q[k] - centre[g, k] for k in range(3)]
    e1, e2 = _dot(d, axes[3:6]), _dot(d, axes[6:9])
    p1, p2 = ray.h1 / rho[g], ray.h2 / rho[g]
    fin = np.isfinite(ray.la.v.astype(np.float64))
    la = ray.la.where(fin, 0.0)
    one = kind(np.ones(len(g)))
    w, s1, s2 = ray.w, ray.s1, ray.s2
    zero = kind(np.zeros(len(g)))
    terms = [w, w * e1, w * e2, w * s1, w * s2, w * (e1 * e1 + e2 * e2), w * (e1 * s1 + e2 * s2), w * (s1 * s1 + s2 * s2),
             one.where(fin, zero), w.where(fin, zero), (w * la).where(fin, zero), (w * (la * la)).where(fin, zero)]
    return SimpleNamespace(p1=p1, p2=p2, e1=e1, e2=e2, la=la, fin=fin, terms=terms)


def _bounded_sums(values, errors, key, n, depth):
    """Per key the longdouble sums of ``values`` (m, k) and gamma(depth) (sum |t| + sum e) + sum e; depth per key."""
    sums, size, own = np.zeros((n, values.shape[1]), dtype=LD), np.zeros((n, values.shape[1])), np.zeros((n, values.shape[1]))
    np.add.at(sums, key, values)
    np.add.at(size, key, np.abs(values).astype(np.float64))
    np.add.at(own, key, errors.astype(np.float64))
    g = np.array([gamma(int(d)) for d in depth])[:, None]
    return sums, SECOND_ORDER * (g * (size + own) + own)


def bounded_aberrations(frame, centre, rho, surface=None, generation=None, pupil="position", origin=(0.0, 0.0, 0.0),
                        reference="centroid", axes=DEFAULT_AXES, pupil_radius=None, terms=21, zones=64, weights=None,
                        rays_per_source=None, n_groups=1, index=None, fit=True):
    """prt_frame_ray_aberrations in longdouble with bounds (the module docstring derives them).  ``centre`` (n_groups, 3)
    and ``rho`` (n_groups) are the device's: they are held to ``centre_ref`` / ``centre_bound`` and ``rho_ref`` /
    ``rho_bound`` here, and the per-ray chain and the sums take them as inputs.  Returns the counts (exact), per ray
    ``rays`` (n, 7) and ``rays_bound``, per group ``sums`` (8) and ``normal`` with their bounds, ``zones`` (n_zones, 6)
    with bounds, and for the groups with a full-rank fit ``coef`` (4, terms) and ``coef_bound`` (4)."""
    axes = np.asarray(axes, dtype=np.float64)
    centre, rho = np.atleast_2d(np.asarray(centre, dtype=np.float64)), np.atleast_1d(np.asarray(rho, dtype=np.float64))
    index = join(frame) if index is None else index
    group = ref.selection(frame, surface, generation, rays_per_source, n_groups)
    used = used_rays(frame, index, group, pupil, origin, axes, weights)
    rows = np.flatnonzero(used)
    g = group[rows]
    out = SimpleNamespace(rows=rows, group=g, n_rays=np.bincount(g, minlength=n_groups),
                          n_missed=np.bincount(group[(group >= 0) & ~used], minlength=n_groups))
    full = out.n_rays > 0
    ray = ray_chain(Err, frame, rows, index[rows], pupil, origin, axes, weights)
    # rho: the given radius, or the largest |h| of the group (0: 1)
    extent, extent_e = np.zeros(n_groups, dtype=LD), np.zeros(n_groups, dtype=LD)
    np.maximum.at(extent, g, ray.radius.v)
    np.maximum.at(extent_e, g, ray.radius.e)
    if pupil_radius:
        out.rho_ref, out.rho_bound = np.full(n_groups, pupil_radius, dtype=LD), np.zeros(n_groups)
    else:
        out.rho_ref = np.where(extent > 0, extent, 1)
        out.rho_bound = (SECOND_ORDER * extent_e).astype(np.float64)
    # the chief ray: the first row of the smallest |h|^2 -- as long as rounding cannot change which it is
    out.chief = np.full(n_groups, -1, dtype=np.int64)
    order = np.lexsort((rows, ray.hh.v, g))
    first = np.flatnonzero(np.r_[True, g[order][1:] != g[order][:-1]]) if len(rows) else np.zeros(0, dtype=np.int64)
    out.chief[g[order][first]] = rows[order][first]
    for k in first:   # (a tie of exactly equal values is decided by the row; one within rounding is not decided)
        if k + 1 < len(order) and g[order[k + 1]] == g[order[k]]:
            a, b = order[k], order[k + 1]
            if ray.hh.v[b] != ray.hh.v[a] and ray.hh.v[b] - ray.hh.v[a] <= ray.hh.e[a] + ray.hh.e[b]:
                raise ValueError("two rays share the smallest |h|^2 within rounding: the chief ray is not determined")
    # the zones (from the device's rho) and the chunks they make
    nz = max(zones, 1)
    p1, p2 = ray.h1 / rho[g], ray.h2 / rho[g]
    zone = np.zeros(len(rows), dtype=np.int64)
    if zones:
        ring = (p1 * p1 + p2 * p2).sqrt() * float(zones)
        edge = np.rint(ring.v)   # (the edges between two zones: 1 .. zones - 1; at and past ``zones`` both sides clip)
        if np.any((np.abs(ring.v - edge) <= ring.e) & (edge >= 1) & (edge <= zones - 1)):
            raise ValueError("a ray lies on a zone's edge within rounding: its zone is not determined")
        zone = np.minimum(np.floor(ring.v), zones - 1).astype(np.int64)
    out.buckets = np.bincount(g * nz + zone, minlength=n_groups * nz).reshape(n_groups, nz)
    chunks_b = ab_chunks(out.buckets)
    chunks_g = chunks_b.sum(1)
    # the centre
    if isinstance(reference, str) and reference == "centroid":
        depth = np.array([stage_depth(c) for c in chunks_g])
        wq = np.stack([ray.w.v * ray.q[k].v for k in range(3)] + [ray.w.v], 1)
        total = np.zeros((n_groups, 4), dtype=LD)
        size = np.zeros((n_groups, 4), dtype=LD)
        np.add.at(total, g, wq)
        np.add.at(size, g, np.abs(wq))
        with np.errstate(all="ignore"):
            out.centre_ref = total[:, 0:3] / total[:, 3:4]
            g1, g0 = np.array([gamma(d + 1) for d in depth])[:, None], np.array([gamma(d) for d in depth])[:, None]
            moved = (g1 * size[:, 0:3] + np.abs(out.centre_ref) * g0 * size[:, 3:4]) / (total[:, 3:4] * (1 - g0))
            out.centre_bound = (SECOND_ORDER * (moved + U * np.abs(out.centre_ref))).astype(np.float64)
    elif isinstance(reference, str):
        out.centre_ref = np.full((n_groups, 3), np.nan, dtype=LD)
        out.centre_ref[out.chief >= 0] = frame[out.chief[out.chief >= 0], 9:12]
        out.centre_bound = np.zeros((n_groups, 3))
    else:
        out.centre_ref = np.broadcast_to(np.asarray(reference, dtype=np.float64), (n_groups, 3)).astype(LD)
        out.centre_bound = np.zeros((n_groups, 3))
    # the per-ray outputs and the stage sums, from the device's centre and rho
    st = stage_chain(Err, ray, g, centre, rho, axes)
    with np.errstate(invalid="ignore"):
        la = np.where(st.fin, ray.la.v, np.nan)
        la_e = np.where(st.fin, ray.la.e, 0)
    out.rays = np.stack([st.p1.v, st.p2.v, st.e1.v, st.e2.v, ray.s1.v, ray.s2.v, la], 1)
    out.rays_bound = (SECOND_ORDER * np.stack([st.p1.e, st.p2.e, st.e1.e, st.e2.e, ray.s1.e, ray.s2.e, la_e], 1)).astype(np.float64)
    values, errors = np.stack([t.v for t in st.terms], 1), np.stack([t.e for t in st.terms], 1)
    sums, bound = _bounded_sums(values, errors, g, n_groups, [stage_depth(c) for c in chunks_g])
    out.sums, out.sums_bound, out.n_la = sums[:, 0:8], bound[:, 0:8], sums[:, 8].astype(np.int64)
    zsums, zbound = _bounded_sums(values, errors, g * nz + zone, n_groups * nz, [stage_depth(c) for c in chunks_b.reshape(-1)])
    pick = [9, 10, 11, 5, 8]
    out.zones = np.concatenate([out.buckets.reshape(-1, 1).astype(LD), zsums[:, pick]], 1).reshape(n_groups, nz, 6)
    out.zones_bound = np.concatenate([np.zeros((n_groups * nz, 1)), zbound[:, pick]], 1).reshape(n_groups, nz, 6)
    if not zones:
        out.zones, out.zones_bound = out.zones[:, :0], out.zones_bound[:, :0]
    # the normal equations: Z^T W Z (upper triangle), Z^T W t for eps1, eps2, s1, s2, sum w
    z = ref.zernike_recurrence(terms, st.p1, st.p2)
    zv, ze = np.stack([t.v for t in z], 1), np.stack([t.e for t in z], 1).astype(np.float64)
    targets = (st.e1, st.e2, ray.s1, ray.s2)
    tv, te = np.stack([t.v for t in targets], 1), np.stack([t.e for t in targets], 1).astype(np.float64)
    upper = np.triu_indices(terms)
    tri = len(upper[0])
    entries = tri + 4 * terms + 1
    out.normal, out.normal_bound = np.zeros((n_groups, entries), dtype=LD), np.zeros((n_groups, entries))
    out.coef, out.coef_bound, out.condition = {}, {}, {}
    for k in np.flatnonzero(full):
        r = np.flatnonzero(g == k)
        largest = min(int(out.buckets[k].max()), MTF_CHUNK)
        depth = normal_depth(largest, chunks_g[k])
        w, zk, tk = ray.w.v[r], zv[r], tv[r]
        wz = zk * w[:, None]
        out.normal[k] = np.concatenate([(wz.T @ zk)[upper], (wz.T @ tk).T.reshape(-1), [w.sum()]])
        w64, az, ez, at, et = w.astype(np.float64), np.abs(zk).astype(np.float64), ze[r], np.abs(tk).astype(np.float64), te[r]
        waz, wez = az * w64[:, None], ez * w64[:, None]
        size = np.concatenate([(waz.T @ az)[upper], (waz.T @ at).T.reshape(-1), [w64.sum()]])
        own = np.concatenate([(waz.T @ ez + wez.T @ az + wez.T @ ez)[upper],
                              (waz.T @ et + wez.T @ at + wez.T @ et).T.reshape(-1), [0.0]])
        own = own + 3 * U * size   # (two products a term, and their second order)
        out.normal_bound[k] = SECOND_ORDER * (gamma(depth) * (size + own) + own)
        if not fit:
            continue
        matrix = np.zeros((terms, terms), dtype=LD)
        matrix[upper] = out.normal[k, :tri]
        matrix = matrix + np.triu(matrix, 1).T
        n64 = matrix.astype(np.float64)
        out.condition[k] = np.linalg.cond(n64)
        if not out.condition[k] < 1e10:   # (the product's RANK_RCOND: below full rank the fit is the minimum-norm one)
            continue
        d_n = np.zeros((terms, terms))
        d_n[upper] = out.normal_bound[k, :tri]
        d_n = d_n + np.triu(d_n, 1).T
        inverse = np.linalg.norm(np.linalg.inv(n64), 2)
        moved_n = np.linalg.norm(d_n, "fro") + gamma(4 * terms * terms) * np.linalg.norm(n64, "fro")
        out.coef[k], out.coef_bound[k] = np.zeros((4, terms), dtype=LD), np.zeros(4)
        for t in range(4):
            rhs = out.normal[k, tri + t * terms:tri + (t + 1) * terms]
            coef = np.zeros(terms, dtype=LD)
            for _ in range(3):   # (fp64 solves refined on the longdouble residual)
                coef = coef + np.linalg.solve(n64, (rhs - matrix @ coef).astype(np.float64)).astype(LD)
            moved_r = (np.linalg.norm(out.normal_bound[k, tri + t * terms:tri + (t + 1) * terms])
                       + gamma(4 * terms * terms) * float(np.linalg.norm(rhs.astype(np.float64))))
            size = float(np.linalg.norm(coef.astype(np.float64)))
            out.coef[k][t] = coef
            out.coef_bound[k][t] = SECOND_ORDER * inverse * (moved_r + moved_n * size) / (1 - inverse * moved_n)
    return out


# ---- a float64 emulation of the chunk / tile / fold order ---------------------------------------------------------------------
def emulate_chunk_sums(terms, bucket, n_buckets, drop_last_chunk=False):
    """The sums of ``terms`` (m, k) float64 -- rays in row order, ``bucket`` per ray -- as k_aberration_stage and
    k_aberration_fold form them: the stable sort by bucket, per chunk of kMtfChunk each thread over its strided rays in
    order, the tree of kAbBlock, then the chunks in order over all buckets.  drop_last_chunk: the defect of a fold that
    stops one chunk early."""
    order = np.argsort(bucket, kind="stable")
    counts = np.bincount(bucket, minlength=n_buckets)
    partial = []
    at = 0
    for count in counts:
        for lo in range(at, at + count, MTF_CHUNK):
            rays = terms[order[lo:min(lo + MTF_CHUNK, at + count)]]
            padded = np.zeros((-(-len(rays) // AB_BLOCK) * AB_BLOCK, terms.shape[1]))
            padded[:len(rays)] = rays
            red = np.zeros((AB_BLOCK, terms.shape[1]))
            for tile in padded.reshape(-1, AB_BLOCK, terms.shape[1]):   # (thread t: rays lo + t, lo + t + 256, ..)
                red = red + tile
            half = AB_BLOCK // 2
            while half:
                red[:half] = red[:half] + red[half:2 * half]
                half //= 2
            partial.append(red[0].copy())
        at += count
    total = np.zeros(terms.shape[1])
    for chunk in (partial[:-1] if drop_last_chunk else partial):
        total = total + chunk
    return total


def random_aberration_frame(n_rays, seed, n_other=0, id0=0):
    """A frame on no grid: n_rays launched in a disc, an intermediate surface, an image surface 5.0 with third-order
    aberrations and noise, weights in (50, 100); ``n_other`` rows of surface 6.0 spread among the last generation.  A
    few rays have no axis intercept."""
    rng = np.random.default_rng(seed)
    ids = id0 + np.arange(n_rays, dtype=np.float64)
    r, t = np.sqrt(rng.random(n_rays)), rng.random(n_rays) * 2 * np.pi
    start = np.stack([-5.0 + rng.normal(0, 0.1, n_rays), 2 * r * np.cos(t) + 0.3, 2 * r * np.sin(t) - 0.2], 1)
    rd, td = 0.08 * np.sqrt(rng.random(n_rays)), rng.random(n_rays) * 2 * np.pi
    direction = np.stack([np.ones(n_rays), rd * np.cos(td), rd * np.sin(td)], 1)
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    lens = start + 4.0 * direction
    h = start[:, 1:] - np.array([0.3, -0.2])
    image = np.array([8.0, 0.05, -0.02]) + np.concatenate(
        [np.zeros((n_rays, 1)), 1e-3 * h * (h ** 2).sum(1)[:, None] + 2e-3 * h + rng.normal(0, 1e-4, (n_rays, 2))], 1)
    middle = lens + 0.5 * (image - lens)

    def block(gen, ray_ids, a, b, surface):
        rows = np.zeros((len(ray_ids), 15))
        u = (b - a) / np.linalg.norm(b - a, axis=1)[:, None]
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = gen, 50 + 50 * rng.random(len(ray_ids)), 0.5 + rng.random(len(ray_ids)), 1.0
        rows[:, 4], rows[:, 5], rows[:, 6:9], rows[:, 9:12], rows[:, 12:15] = ray_ids, surface, a, b, u
        return rows

    last = block(2, ids, middle, image, 5.0)
    last[::997, IX["y_tilt"]] = 0.0
    if n_other:
        other = block(2, ids[:n_other] + n_rays, middle[:n_other], image[:n_other], 6.0)
        place = np.sort(rng.choice(n_rays + n_other, n_other, replace=False))
        merged = np.zeros((n_rays + n_other, 15))
        mask = np.zeros(n_rays + n_other, dtype=bool)
        mask[place] = True
        merged[mask], merged[~mask] = other, last
        last = merged
    return np.concatenate([block(0, ids, start, lens, 1.0), block(1, ids, lens, middle, 2.0), last])
