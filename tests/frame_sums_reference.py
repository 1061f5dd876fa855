"""References and error bounds for the two oldest analysis passes: the frame statistics of prt_frame.hpp
(prt_frame_reduce, prt_frame_stats, prt_frame_mean_square) and the optical path and wavefront of prt_wavefront.hpp
(prt_frame_optical_path, prt_frame_wavefront), with Python copies of their partition rules and the frames the tests run
on.  Frames here are (R, 15) float64 arrays, one row per frame row, columns in ``COLUMNS``' order.

1. Exact sums.  A frame whose coordinates, pivots, wavelengths and intensities are multiples of 2^-5 below 2 in
   magnitude and whose y_tilt is one of +-1, +-1/2, 0 has every term of every sum of prt_frame_reduce / mean_square on a
   dyadic grid (2^-5, 2^-10 or 2^-20): ``x0 - x_tilt y0 / y_tilt`` is exact, so are the squares.  While the sum of the
   terms' absolute values stays below 2^53 grid units (``require_exact`` raises ``NotExact`` otherwise: a condition, not
   a tolerance) every partial sum is representable, the device's fp64 additions are exact in any order, and the result
   equals ``integer_reduce`` / ``integer_mean_square`` -- numpy int64 in grid units -- bit for bit.

2. Bounds, u = 2^-53, gamma(k) = k u / (1 - k u).  A sum formed in any order moves every term through at most
   ``depth`` additions, so |S~ - S| <= gamma(depth) sum |t|.  For k_frame_reduce, per group (``reduce_depth`` counts it
   from the rows): 16 rows a lane (kFrameRowsPerWave / 64), 6 for the xor tree, the largest number of flushes that meet
   in one word of one slot (one per run of the group in a wave), and 64 for k_frame_fold where the slot path is taken.
   The library is built with -ffp-contract=off and IEEE division and square root: every operation rounds once.
   prt_frame_stats (``stats_bound``), per group of n rows, pivot p~ = the first pass's mean:
     first pass     |p~ - mu| <= gamma(depth + 1) sum |y1| / n =: e                    (the sum, the division)
     second pass    terms y = fl(y1 - p~), |y| <= |y1 - mu| + e:   |S1~ - S1| <= gamma(depth + 1) (sum |y1 - mu| + n e) =: E1
     mean           fl(p~ + fl(S1~ / n)):                         E1 / n + u (e' + |mu|),   e' = e + E1 / n
     variance       V = S3 / n - dy^2 - dz^2 holds about any pivot; the terms y^2 + z^2 carry 4 roundings:
                    dV = (gamma(depth + 4) + 12 u) (V + e'_y^2 + e'_z^2)               (12 u: the division, the two
                    squares and subtractions, and their second order, generously)
     rms            |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|), and u sqrt V for the root itself
     focus          the term x0 - x_tilt y0 / y_tilt is off by phi = u (|focus| + 2.01 |x_tilt y0 / y_tilt|) (product,
                    quotient, difference), which goes through the sums as an error of the terms: the same steps with
                    psi = phi + u |f| on every f = focus - p~
     wavelength, intensity   gamma(depth + 1) sum |w| / n
   Every bound carries a factor 1.001 for the terms of second order.  mean_square(transform="sin") is the same with
   the device's sine off by at most 4 ulp = 8 u |sin q| (what OpenCL requires of a double sine; the error HIP documents
   for its sin() lies within it) and no slots: ``mean_square_reference`` returns it.
   prt_frame_optical_path: a segment index sqrt(dx^2 + dy^2 + dz^2) carries at most 6 roundings in relative terms
   (difference 1, square 2.., root, product), generation g adds g more: gamma(6 + g) opl (all terms are positive).
   prt_frame_wavefront (``wavefront_reference``): the per-row chain (sphere intersection, OPD, pupil point, Zernike
   basis by the device's recurrence) is evaluated in longdouble together with a running error bound of the device's
   own operation sequence (``Err``: every fp64 operation adds u |result| to what its operands carry).  The group's
   reference point P and radius R are held to the summation bound of pass 1 (``sphere_bound``); the per-row chain then
   takes the device's P, R and optical paths as its inputs, as k_frame_wavefront_pupil does.  The normal-equation sums:
   gamma(depth_z) sum |w z_i z_j| plus the terms' own errors, depth_z = the rows of a workgroup's share + its tiles (one
   flush per tile at most) + ceil(workgroups / 64) + 6.  rms and pv follow as above; the Zernike coefficients from the
   perturbation bound of the normal equations, |dc| <= |N^-1| (|dr| + |dN| |c|) / (1 - |N^-1| |dN|), with dN the bound on
   the sums plus gamma(4 J^2) |N| for a backward-stable J x J solve (Higham, Accuracy and Stability, ch. 19 / 20).

Largest deviation-to-bound ratios seen on an MI355X (tests/test_gpu_frame_partitions.py and
tests/test_gpu_wavefront_partitions.py print them; none is fixed in advance):
    prt_frame_stats      mean y 0.43, mean z 0.45 (both on the 1e-6 spot at 1e3; 0.002 elsewhere), rms radius 0.015,
                         focus 0.12, focus_std 0.018, wavelength 0.041, intensity 0.043
    mean_square (sin)    mean 0.028, mean square 0.039
    optical path         0.55
    wavefront            reference point 0.15, radius 0.14, per-row opd 0.072, pupil 0.56, normal sums 0.12, rms 0.013,
                         pv 0.086, Zernike coefficients 0.011
The sums on dyadic frames have no ratio: they are equal or the test fails.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the references need an extended-precision long double (x87: eps = 2^-63)"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}
U = 2.0 ** -53
SECOND_ORDER = 1.001

# ---- named copies of the constants the tests' sizes follow from (test_host_frame_sums.py holds them to the headers) ----
FRAME_ROWS_PER_WAVE = 16 * 64   # prt_frame.hpp: static const int kFrameRowsPerWave = 16 * 64;
FRAME_SLOTS = 64                # prt_frame.hpp: static const int kFrameSlots = 64;
FRAME_SLOT_GROUPS = 2048        # prt_frame.hpp: static const int kFrameSlotGroups = 2048;
FRAME_SLOT_WAVES = 256          # prt_frame.hpp, prt_frame_reduce: waves / n_groups >= 256
WF_MAX_WAVES = 2048             # prt_wavefront.hpp: static const int kWfMaxWaves = 2048;
WF_ROWS_PER_WAVE = 1024         # prt_wavefront.hpp: static const int kWfRowsPerWave = 1024;
WF_ZBLOCK = 256                 # prt_wavefront.hpp: static const int kWfZBlock = 256;
WF_MAX_ZBLOCKS = 512            # prt_wavefront.hpp: static const int kWfMaxZBlocks = 512;
WF_SLAB_BYTES = 64 << 20        # prt_wavefront.hpp: static const size_t kWfSlabBytes = 64u << 20;
WF_REF_BLOCK = 512              # prt_wavefront.hpp: static const int kWfRefBlock = 512;
WF_LOC = 8                      # prt_wavefront.hpp: enum { WF_LOC = 8, ...
BLOCK = 256                     # prt_device.hpp: #define PRT_BLOCK 256
HEADER_NAMES = dict(kFrameRowsPerWave="FRAME_ROWS_PER_WAVE", kFrameSlots="FRAME_SLOTS", kFrameSlotGroups="FRAME_SLOT_GROUPS",
                    kWfMaxWaves="WF_MAX_WAVES", kWfRowsPerWave="WF_ROWS_PER_WAVE", kWfZBlock="WF_ZBLOCK",
                    kWfMaxZBlocks="WF_MAX_ZBLOCKS", kWfSlabBytes="WF_SLAB_BYTES", kWfRefBlock="WF_REF_BLOCK")
# lines of the headers the partition rules below restate
HOST_RULES = {
    "prt_frame.hpp": (
        "const int slots = (n_groups <= kFrameSlotGroups && waves / n_groups >= 256) ? kFrameSlots : 1;",
        "double* const mine = out + (size_t)(wave & (slots - 1)) * n_groups * FRAME_STATS;",
        "for (int k = 0; k < slots; ++k) v += partial[(size_t)k * n + e];"),
    "prt_sort.hpp": (
        "waves = std::min<int64_t>(std::max<int64_t>(waves, 1), kWfMaxWaves);",
        "waves = std::max<int64_t>(1, std::min<int64_t>(waves, (int64_t)(cap_bytes / ((size_t)buckets * cell_bytes))));",
        "const int64_t per_wave = ((n_rows + waves - 1) / waves + 63) / 64 * 64;",
        "const int64_t per = (n + kSortScanBlock - 1) / kSortScanBlock;"),
    "prt_wavefront.hpp": (
        "const SortPlan plan = sort_plan(n_rows, n_groups, WF_LOC * sizeof(double), kWfSlabBytes);",
        "static_assert(kWfRefBlock == kSortScanBlock,",
        "const int64_t tiles = (n_rows + kWfZBlock * 4 - 1) / (kWfZBlock * 4);",
        "int64_t zblocks = std::min<int64_t>(std::max<int64_t>(tiles, 1), std::min<int64_t>(kWfMaxZBlocks, 2 * (int64_t)cus));",
        "const int64_t per = ((n + gridDim.x - 1) / gridDim.x + kWfZBlock - 1) / kWfZBlock * kWfZBlock;"),
}


def header_constants(names=None):
    """The static const ints of the headers ``names`` (default: those of HOST_RULES), by name."""
    found = {}
    for name in (HOST_RULES if names is None else names):
        text = open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read()
        for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
            try:
                found[key] = int(eval(re.sub(r"(\d+)u\b", r"\1", value), {"__builtins__": {}}, {}))
            except (NameError, SyntaxError, TypeError):
                pass  # (not a plain constant)
    return found


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the partition rules ------------------------------------------------------------------------------------------------
def frame_waves(n_rows):
    return -(-n_rows // FRAME_ROWS_PER_WAVE)


def frame_slots(n_rows, n_groups):
    """The copies of the output prt_frame_reduce spreads its atomics over."""
    return FRAME_SLOTS if n_groups <= FRAME_SLOT_GROUPS and frame_waves(n_rows) // n_groups >= FRAME_SLOT_WAVES else 1


def slot_switch_rows(n_groups):
    """The smallest n_rows at which prt_frame_reduce takes the slot path for n_groups."""
    return (FRAME_SLOT_WAVES * n_groups - 1) * FRAME_ROWS_PER_WAVE + 1


def wf_waves(n_rows, n_groups):
    waves = min(max(-(-n_rows // WF_ROWS_PER_WAVE), 1), WF_MAX_WAVES)
    return max(1, min(waves, WF_SLAB_BYTES // (n_groups * WF_LOC * 8)))


def wf_per_wave(n_rows, n_groups):
    waves = wf_waves(n_rows, n_groups)
    return (-(-n_rows // waves) + 63) // 64 * 64


def wf_scan_per(n_rows, n_groups):
    """The waves one thread of the offset scan adds up (the launch rounds the waves up to whole workgroups)."""
    all_waves = -(-wf_waves(n_rows, n_groups) // (BLOCK // 64)) * (BLOCK // 64)
    return -(-all_waves // WF_REF_BLOCK)


def wf_zblocks(n_rows, n_groups, terms, cus):
    tiles = -(-n_rows // (WF_ZBLOCK * 4))
    entries = terms * (terms + 1) // 2 + terms + 3
    blocks = min(max(tiles, 1), min(WF_MAX_ZBLOCKS, 2 * cus))
    return max(1, min(blocks, WF_SLAB_BYTES // (n_groups * entries * 8)))


def wf_zshare(n_selected, zblocks):
    """The rows of one k_frame_zernike workgroup."""
    return -(-(-(-n_selected // zblocks)) // WF_ZBLOCK) * WF_ZBLOCK


# ---- selection -----------------------------------------------------------------------------------------------------------
def selection(frame, surface=None, generation=None, rays_per_source=None, n_groups=1):
    """Per row the group it is counted in, -1 for none: the device's rule (floor of the fp64 quotient)."""
    keep = np.ones(len(frame), dtype=bool)
    if surface is not None:
        keep &= frame[:, IX["surface"]] == surface
    if generation is not None:
        keep &= frame[:, IX["generation"]] == generation
    group = np.zeros(len(frame), dtype=np.int64)
    if rays_per_source:
        g = np.floor(frame[:, IX["id"]] / float(rays_per_source))
        group = np.where((g >= 0) & (g < n_groups), g, -1).astype(np.int64)
    group[~keep] = -1
    return group


def reduce_depth(group, n_groups, slots):
    """Per group the additions a term of k_frame_reduce (or k_frame_mean_square: slots = 1) passes at most."""
    sel = np.flatnonzero(group >= 0)
    flushes = np.zeros((slots, n_groups), dtype=np.int64)
    if len(sel):
        g = group[sel]
        _, first = np.unique((sel // 64) * n_groups + g, return_index=True)
        first.sort()  # (a slice's groups are worked off in the order of their first lanes)
        seq_g, seq_wave = g[first], sel[first] // FRAME_ROWS_PER_WAVE
        start = np.ones(len(first), dtype=bool)
        start[1:] = (seq_g[1:] != seq_g[:-1]) | (seq_wave[1:] != seq_wave[:-1])
        np.add.at(flushes, (seq_wave[start] & (slots - 1), seq_g[start]), 1)
    return FRAME_ROWS_PER_WAVE // 64 + 6 + flushes.max(axis=0) + (slots if slots > 1 else 0)


# ---- 1. exact sums on a dyadic grid --------------------------------------------------------------------------------------
GRID = 32  # 2^5
TILTS = (1.0, -1.0, 0.5, -0.5, 0.0)


class NotExact(AssertionError):
    """A sum of the frame is not exactly representable in fp64: choose a narrower grid."""


def to_grid(values, what, unit=GRID):
    k = np.asarray(values, dtype=np.float64) * unit
    if not np.all(k == np.rint(k)) or np.any(np.abs(k) >= 2.0 ** 30):
        raise ValueError(f"{what}: not a multiple of 1/{unit} (or beyond 2^30 of them)")
    return k.astype(np.int64)


def abs_total(column):
    """sum |column| as a Python integer."""
    column = np.abs(np.asarray(column))
    if len(column) == 0:
        return 0
    if int(column.max()) * len(column) < 2 ** 62:
        return int(column.sum())
    return sum(int(v) for v in column)


def require_exact(columns):
    for k, column in enumerate(columns):
        total = abs_total(column)
        if total >= 2 ** 53:
            raise NotExact(f"column {k}: the absolute values add up to {total} >= 2^53 grid units")


def dyadic_frame(n_rows, seed):
    """Random rows on the grid: coordinates and x_tilt / z_tilt multiples of 2^-5 in (-2, 2), wavelength and intensity in
    (0, 2), y_tilt from ``TILTS``; generation, id and surface are zero, for the caller to fill."""
    rng = np.random.default_rng(seed)
    frame = np.zeros((n_rows, 15))
    frame[:, 6:13] = rng.integers(-2 * GRID + 1, 2 * GRID, (n_rows, 7)) / GRID
    frame[:, IX["z_tilt"]] = rng.integers(-2 * GRID + 1, 2 * GRID, n_rows) / GRID
    frame[:, IX["y_tilt"]] = rng.choice(TILTS, n_rows, p=(0.3, 0.2, 0.2, 0.2, 0.1))
    frame[:, IX["intensity"]] = rng.integers(1, 2 * GRID, n_rows) / GRID
    frame[:, IX["wavelength"]] = rng.integers(1, 2 * GRID, n_rows) / GRID
    return frame


def dyadic_pivots(n_groups, seed):
    return np.random.default_rng(seed).integers(-2 * GRID + 1, 2 * GRID, (n_groups, 3)) / GRID


def _intercept_units(rows):
    """The axis intercept x0 - x_tilt y0 / y_tilt in units of 2^-10, and which rows have one."""
    tilt = rows[:, IX["y_tilt"]]
    if not np.all(np.isin(tilt, TILTS)):
        raise ValueError("y_tilt: one of +-1, +-1/2, 0")
    inverse = np.zeros(len(rows), dtype=np.int64)
    inverse[tilt != 0] = (1.0 / tilt[tilt != 0]).astype(np.int64)
    focus = (to_grid(rows[:, IX["x0"]], "x0") * GRID
             - to_grid(rows[:, IX["x_tilt"]], "x_tilt") * to_grid(rows[:, IX["y0"]], "y0") * inverse)
    return focus, tilt != 0


def _group_sums(columns, group, n_groups, units):
    out = np.zeros((n_groups, len(columns)))
    for k, (column, unit) in enumerate(zip(columns, units)):
        total = np.zeros(n_groups, dtype=np.int64)
        np.add.at(total, group, column)
        out[:, k] = total.astype(np.float64) * unit  # (below 2^53: exact, and the unit is a power of two)
    return out


def integer_reduce(frame, surface=None, generation=None, rays_per_source=None, n_groups=1, pivots=None):
    """The nine sums of prt_frame_reduce per group, (n_groups, 9) float64, from integers."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    rows, g = frame[group >= 0], group[group >= 0]
    pivots = np.zeros((n_groups, 3)) if pivots is None else np.asarray(pivots, dtype=np.float64)
    p = to_grid(pivots, "pivots")
    y = to_grid(rows[:, IX["y1"]], "y1") - p[g, 0]
    z = to_grid(rows[:, IX["z1"]], "z1") - p[g, 1]
    focus, has = _intercept_units(rows)
    f = np.where(has, focus - p[g, 2] * GRID, 0)
    columns = [np.ones(len(rows), dtype=np.int64), y, z, y * y + z * z, f, f * f,
               to_grid(rows[:, IX["wavelength"]], "wavelength"), to_grid(rows[:, IX["intensity"]], "intensity"),
               has.astype(np.int64)]
    require_exact(columns)
    return _group_sums(columns, g, n_groups, (1.0, 1.0 / GRID, 1.0 / GRID, GRID ** -2.0, GRID ** -2.0, GRID ** -4.0,
                                              1.0 / GRID, 1.0 / GRID, 1.0))


def integer_mean_square(frame, quantity, about=0.0, surface=None, generation=None, rays_per_source=None, n_groups=1):
    """The three sums of prt_frame_mean_square (no transform) per group, (n_groups, 3) float64, from integers."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    rows, g = frame[group >= 0], group[group >= 0]
    if quantity == "axis_intercept":
        value, has = _intercept_units(rows)
        value, unit = value - int(to_grid(about, "about", GRID * GRID)), GRID ** -2.0
        rows, g, value = rows[has], g[has], value[has]
    else:
        value, unit = to_grid(rows[:, IX[quantity]], quantity) - int(to_grid(about, "about")), 1.0 / GRID
    columns = [np.ones(len(value), dtype=np.int64), value, value * value]
    require_exact(columns)
    return _group_sums(columns, g, n_groups, (1.0, unit, unit * unit))


def mean_square_table(sums):
    """(count, mean, mean_square) as DeviceFrame.mean_square forms them from the three sums."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums[:, 0].astype(np.int64), sums[:, 1] / sums[:, 0], sums[:, 2] / sums[:, 0]


# ---- 2. longdouble references of the frame statistics ---------------------------------------------------------------------
def _terms(rows, pivot, kind):
    """The nine terms of a row of k_frame_reduce about ``pivot`` (3,), in ``kind`` (LD or float64): (n, 9), ok."""
    c = lambda name: rows[:, IX[name]].astype(kind)  # noqa: E731
    pivot = np.asarray(pivot).astype(kind)
    y, z = c("y1") - pivot[0], c("z1") - pivot[1]
    with np.errstate(all="ignore"):
        f = (c("x0") - c("x_tilt") * c("y0") / c("y_tilt")) - pivot[2]
    ok = np.isfinite(f)
    f = np.where(ok, f, 0)
    one = np.ones(len(rows), dtype=kind)
    return np.stack([one, y, z, y * y + z * z, f, f * f, c("wavelength"), c("intensity"), ok.astype(kind)], 1), ok


def reduce_reference(frame, surface=None, generation=None, rays_per_source=None, n_groups=1, pivots=None):
    """prt_frame_reduce's nine sums per group in longdouble."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    out = np.zeros((n_groups, 9), dtype=LD)
    for g in range(n_groups):
        terms, _ = _terms(frame[group == g], np.zeros(3) if pivots is None else pivots[g], LD)
        out[g] = terms.sum(axis=0)
    return out


def stats_reference(frame, surface=None, generation=None, rays_per_source=None, n_groups=1):
    """prt_frame_stats in longdouble: ``stats`` (n_groups, 8) and per group what ``stats_bound`` needs."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    stats = np.full((n_groups, 8), np.nan, dtype=LD)
    parts = []
    for g in range(n_groups):
        rows = frame[group == g]
        n = len(rows)
        stats[g, 0] = n
        if n == 0:
            parts.append(None)
            continue
        y, z = rows[:, IX["y1"]].astype(LD), rows[:, IX["z1"]].astype(LD)
        with np.errstate(all="ignore"):
            q = rows[:, IX["x_tilt"]].astype(LD) * rows[:, IX["y0"]].astype(LD) / rows[:, IX["y_tilt"]].astype(LD)
            focus = rows[:, IX["x0"]].astype(LD) - q
        ok = np.isfinite(focus)
        focus, q = focus[ok], q[ok]
        my, mz = y.mean(), z.mean()
        var = ((y - my) ** 2 + (z - mz) ** 2).mean()
        stats[g, 1:4] = my, mz, np.sqrt(var)
        part = SimpleNamespace(n=n, nf=int(ok.sum()), my=my, mz=mz, var=var, abs_y=np.abs(y).sum(), abs_z=np.abs(z).sum(),
                               dev_y=np.abs(y - my).sum(), dev_z=np.abs(z - mz).sum())
        if part.nf:
            mf = focus.mean()
            part.mf, part.var_f = mf, ((focus - mf) ** 2).mean()
            part.abs_f, part.dev_f = np.abs(focus).sum(), np.abs(focus - mf)
            part.phi = U * (np.abs(focus) + 2.01 * np.abs(q))
            stats[g, 4:6] = mf, np.sqrt(part.var_f)
        w, i = rows[:, IX["wavelength"]].astype(LD), rows[:, IX["intensity"]].astype(LD)
        stats[g, 6:8] = w.mean(), i.mean()
        part.abs_w, part.abs_i = np.abs(w).sum(), np.abs(i).sum()
        parts.append(part)
    return SimpleNamespace(stats=stats, parts=parts, group=group)


def _root_bound(var, d_var):
    """|sqrt(var~) - sqrt(var)| for |var~ - var| <= d_var (var~ clamped at 0), and the root's own rounding."""
    root = np.sqrt(var)
    moved = min(d_var / root, np.sqrt(d_var)) if root > 0 else np.sqrt(d_var)
    return float(SECOND_ORDER * (moved + U * root))


def stats_bound(ref, depth):
    """(n_groups, 8): the bound on every statistic of prt_frame_stats (the module docstring derives it); ``depth`` per
    group, from ``reduce_depth``.  The count's is 0."""
    bound = np.zeros((len(ref.parts), 8))
    for g, p in enumerate(ref.parts):
        if p is None:
            continue
        d = int(depth[g])
        moved = {}
        for name, mean in (("y", p.my), ("z", p.mz)):
            e = gamma(d + 1) * getattr(p, "abs_" + name) / p.n
            e1 = gamma(d + 1) * (getattr(p, "dev_" + name) + p.n * e)
            moved[name] = e + e1 / p.n
            bound[g, 1 if name == "y" else 2] = SECOND_ORDER * (e1 / p.n + U * (moved[name] + abs(mean)))
        q = moved["y"] ** 2 + moved["z"] ** 2
        bound[g, 3] = _root_bound(p.var, (gamma(d + 4) + 12 * U) * (p.var + q))
        if p.nf:
            phi = p.phi.sum()
            e = (gamma(d + 1) * (p.abs_f + phi) + phi) / p.nf
            f = p.dev_f + e
            psi = p.phi + U * f
            e4 = gamma(d + 1) * (f.sum() + psi.sum()) + psi.sum()
            e_f = e + e4 / p.nf
            bound[g, 4] = SECOND_ORDER * (e4 / p.nf + U * (e_f + abs(p.mf)))
            e5 = gamma(d + 2) * ((f + psi) ** 2).sum() + (2 * f * psi + psi * psi).sum()
            bound[g, 5] = _root_bound(p.var_f, e5 / p.nf + 12 * U * (p.var_f + e_f ** 2) + 2 * e_f * e_f * 12 * U)
        bound[g, 6] = SECOND_ORDER * gamma(d + 1) * p.abs_w / p.n
        bound[g, 7] = SECOND_ORDER * gamma(d + 1) * p.abs_i / p.n
    return bound


SIN_ULPS = 4  # what OpenCL requires of sin for double; the error HIP documents for its sin() lies within it


def mean_square_reference(frame, quantity, about=0.0, transform=None, surface=None, generation=None,
                          rays_per_source=None, n_groups=1):
    """DeviceFrame.mean_square in longdouble: per group (count, mean, mean_square) and the bounds on the two means."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    depth = reduce_depth(group, n_groups, 1)
    out, bound = np.full((n_groups, 3), np.nan, dtype=LD), np.zeros((n_groups, 3))
    for g in range(n_groups):
        rows = frame[group == g]
        if quantity == "axis_intercept":
            with np.errstate(all="ignore"):
                t = rows[:, IX["x_tilt"]].astype(LD) * rows[:, IX["y0"]].astype(LD) / rows[:, IX["y_tilt"]].astype(LD)
                q = rows[:, IX["x0"]].astype(LD) - t
            off = U * (np.abs(q) + 2.01 * np.abs(t))
        else:
            q = rows[:, IX[quantity]].astype(LD)
            off = np.zeros(len(rows), dtype=LD)
        if transform == "sin":
            q = np.sin(q)
            off = off + 2 * SIN_ULPS * U * np.abs(q)  # (|sin'| <= 1: what q carried stays)
        v = q - LD(about)
        ok = np.isfinite(v)
        v, off = v[ok], off[ok]
        out[g, 0] = len(v)
        if not len(v):
            continue
        psi = off + U * np.abs(v)
        d = int(depth[g])
        out[g, 1], out[g, 2] = v.mean(), (v * v).mean()
        e1 = gamma(d) * (np.abs(v) + psi).sum() + psi.sum()
        e2 = gamma(d + 1) * ((np.abs(v) + psi) ** 2).sum() + (2 * np.abs(v) * psi + psi * psi).sum()
        bound[g, 1] = SECOND_ORDER * (e1 / len(v) + U * abs(out[g, 1]))
        bound[g, 2] = SECOND_ORDER * (e2 / len(v) + U * out[g, 2])
    return out, bound


def emulate_reduce(frame, group, n_groups, pivots, slots):
    """A float64 emulation of the device's partition: the terms as the kernel forms them, added per wave of 1024 rows
    and group, the waves into their slots in wave order, the slots folded in order."""
    partial = np.zeros((slots, n_groups, 9))
    sel = np.flatnonzero(group >= 0)
    if len(sel):
        g = group[sel]
        terms = np.zeros((len(sel), 9))
        for k in range(n_groups):
            terms[g == k], _ = _terms(frame[sel[g == k]], np.zeros(3) if pivots is None else pivots[k], np.float64)
        key = (sel // FRAME_ROWS_PER_WAVE) * n_groups + g
        order = np.argsort(key, kind="stable")
        starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
        sums = np.add.reduceat(terms[order], starts, axis=0)
        for s, k in zip(sums, key[order][starts]):
            partial[(k // n_groups) & (slots - 1), k % n_groups] += s
    out = np.zeros((n_groups, 9))
    for k in range(slots):
        out += partial[k]
    return out


def emulate_stats(frame, surface=None, generation=None, rays_per_source=None, n_groups=1):
    """prt_frame_stats in float64 on the emulated partition: two passes, k_frame_pivots and k_frame_finish."""
    group = selection(frame, surface, generation, rays_per_source, n_groups)
    slots = frame_slots(len(frame), n_groups)
    first = emulate_reduce(frame, group, n_groups, None, slots)
    safe, safe_f = np.where(first[:, 0] > 0, first[:, 0], 1.0), np.where(first[:, 8] > 0, first[:, 8], 1.0)
    pivots = np.stack([first[:, 1] / safe, first[:, 2] / safe, first[:, 4] / safe_f], 1)
    s = emulate_reduce(frame, group, n_groups, pivots, slots)
    dy, dz, df = s[:, 1] / safe, s[:, 2] / safe, s[:, 4] / safe_f
    var_r = np.maximum(s[:, 3] / safe - dy * dy - dz * dz, 0.0)
    var_f = np.maximum(s[:, 5] / safe_f - df * df, 0.0)
    out = np.stack([s[:, 0], pivots[:, 0] + dy, pivots[:, 1] + dz, np.sqrt(var_r), pivots[:, 2] + df, np.sqrt(var_f),
                    s[:, 6] / safe, s[:, 7] / safe], 1)
    out[s[:, 0] == 0, 1:] = np.nan
    out[s[:, 8] == 0, 4:6] = np.nan
    return out


def random_frame(n_rows, n_groups, seed, centre=(0.3, -0.2), width=1.0):
    """A frame that is on no grid: one generation, ascending ids in n_groups equal runs (rays_per_source =
    ceil(n_rows / n_groups)), a spot of the given width about ``centre``, a few rows without an axis intercept."""
    rng = np.random.default_rng(seed)
    frame = np.zeros((n_rows, 15))
    frame[:, IX["id"]] = np.arange(n_rows)
    frame[:, IX["intensity"]] = 50 + 50 * rng.random(n_rows)
    frame[:, IX["wavelength"]] = 0.4 + 0.3 * rng.random(n_rows)
    frame[:, IX["x0"]] = -3 + rng.normal(0, 0.01, n_rows)
    frame[:, IX["y0"]], frame[:, IX["z0"]] = rng.normal(0, 0.5, (2, n_rows))
    frame[:, IX["x1"]] = 10.0
    frame[:, IX["y1"]] = centre[0] + width * rng.normal(0, 1, n_rows)
    frame[:, IX["z1"]] = centre[1] + width * rng.normal(0, 1, n_rows)
    d = frame[:, 9:12] - frame[:, 6:9]
    frame[:, 12:15] = d / np.linalg.norm(d, axis=1)[:, None]
    frame[::997, IX["y_tilt"]] = 0.0
    return frame, -(-n_rows // n_groups)


# ---- 3. optical path and wavefront ------------------------------------------------------------------------------------------
def opl_reference(frame):
    """The cumulative optical path of every row in longdouble, joined by id over the generations as the device joins
    them (a generation that lacks the id starts the sum again), and the bound gamma(6 + generation) opl."""
    ids = frame[:, IX["id"]].astype(np.int64)
    generation = frame[:, IX["generation"]].astype(np.int64)
    d = [frame[:, IX[b]].astype(LD) - frame[:, IX[a]].astype(LD) for a, b in (("x0", "x1"), ("y0", "y1"), ("z0", "z1"))]
    segment = frame[:, IX["index"]].astype(LD) * np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    id0 = ids.min() if len(ids) else 0
    acc = np.zeros(int(ids.max() - id0) + 1 if len(ids) else 1, dtype=LD)
    stamp = np.full(len(acc), -2, dtype=np.int64)
    opl = np.zeros(len(frame), dtype=LD)
    for g in range(int(generation.max()) + 1 if len(ids) else 0):
        rows = np.flatnonzero(generation == g)
        at = ids[rows] - id0
        opl[rows] = np.where(stamp[at] == g - 1, acc[at], 0) + segment[rows]
        acc[at], stamp[at] = opl[rows], g
    return opl, (SECOND_ORDER * np.array([gamma(6 + g) for g in range(int(generation.max()) + 1)])[generation]
                 * np.abs(opl)).astype(np.float64)


class Err:
    """A longdouble value and a bound on how far the device's fp64 value is from it; every operation rounds once."""
    KIND = LD

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=self.KIND)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=self.KIND)

    def _rounded(self, v, moved):
        return type(self)(v, moved + U * (np.abs(v) + moved))

    def of(self, x):
        return x if isinstance(x, Err) else type(self)(x)

    def __add__(self, o):
        o = self.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = self.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = self.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = self.of(o)
        v = self.v / o.v
        room = np.abs(o.v) - o.e
        with np.errstate(all="ignore"):
            moved = np.where(room > 0, (self.e + np.abs(v) * o.e) / np.where(room > 0, room, 1), np.inf)
        return self._rounded(v, moved)

    def __neg__(self):
        return type(self)(-self.v, self.e)

    def sqrt(self):
        with np.errstate(invalid="ignore"):
            v = np.sqrt(self.v)
            low, high = np.sqrt(np.maximum(self.v - self.e, 0)), np.sqrt(self.v + self.e)
        return self._rounded(v, np.maximum(high - v, v - low))

    def take(self, index):
        return type(self)(self.v[index], self.e[index])

    def where(self, mask, other):
        other = self.of(other)
        return type(self)(np.where(mask, self.v, other.v), np.where(mask, self.e, other.e))


class Fp64(Err):
    """The same operations in float64: what an Err's bound is checked against on the host."""
    KIND = np.float64


def noll(j):
    n, k = 0, j - 1
    while k > n:
        n += 1
        k -= n
    m = n % 2 + 2 * ((k + (n + 1) % 2) // 2)
    return n, (-m if j % 2 else m)


def zernike_closed_form(terms, x, y):
    """Z_1 .. Z_terms at (x, y) from the factorial formula, longdouble, (n, terms): what the recurrence is checked
    against on the host."""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    rho, theta = np.hypot(x, y), np.arctan2(y, x)
    out = []
    for j in range(1, terms + 1):
        n, m = noll(j)
        am = abs(m)
        radial = sum(LD((-1) ** k * math.factorial(n - k))
                     / LD(math.factorial(k) * math.factorial((n + am) // 2 - k) * math.factorial((n - am) // 2 - k))
                     * rho ** (n - 2 * k) for k in range((n - am) // 2 + 1))
        angular = LD(1) if m == 0 else (np.cos(am * theta) if m > 0 else np.sin(am * theta))
        out.append(np.sqrt(LD(n + 1 if m == 0 else 2 * (n + 1))) * radial * angular)
    return np.stack(out, 1)


def zernike_recurrence(terms, x, y):
    """wf_zernike's operation sequence on ``Err`` values: a list of ``terms`` Err, the basis in longdouble and the
    running bound on the device's rounding (and on what x and y carried in)."""
    rho2 = x * x + y * y
    rho = rho2.sqrt()
    inside = rho.v > 0
    safe = type(x)(np.where(inside, rho.v, 1), rho.e)
    c1, s1 = (x / safe).where(inside, 1.0), (y / safe).where(inside, 0.0)
    one = type(x)(np.ones_like(x.v))
    cm, sm, rm = [one], [type(x)(np.zeros_like(x.v))], [one]
    for m in range(1, 8):
        cm.append(cm[m - 1] * c1 - sm[m - 1] * s1)
        sm.append(sm[m - 1] * c1 + cm[m - 1] * s1)
        rm.append(rm[m - 1] * rho)
    radial = {}
    for m in range(8):
        radial[m, m] = rm[m]
        if m + 2 < 8:
            radial[m + 2, m] = rm[m + 2] * float(m + 2) - rm[m] * float(m + 1)
        for n in range(m + 4, 8, 2):
            k1, k2 = 0.5 * (n + m) * (n - m) * (n - 2), 2.0 * n * (n - 1) * (n - 2)
            k3, k4 = -float(m) * m * (n - 1) - float(n) * (n - 1) * (n - 2), -0.5 * n * (n + m - 2) * (n - m - 2)
            radial[n, m] = ((rho2 * k2 + k3) * radial[n - 2, m] + radial[n - 4, m] * k4) / k1
    out = []
    for j in range(1, terms + 1):
        n, m = noll(j)
        am = abs(m)
        norm = type(x)(np.sqrt(LD(n + 1 if am == 0 else 2 * (n + 1))), U * 2.0 * math.sqrt(2 * (n + 1)))  # (a fp64 constant)
        out.append(norm * radial[n, am] * (cm[am] if m > 0 else sm[am] if m < 0 else 1.0))
    return out


def sphere_bound(frame, group, n_groups, per_wave, waves):
    """Pass 1 in longdouble: per group the rows, the centroid P of the end points, the default radius R (from P to the
    mean start point) and the bounds on the device's P and R.  A sum of k_frame_wavefront_locate and the fold of
    k_frame_wavefront_reference move a term through per_wave / 64 (a lane's rows) + 6 + per_wave / 64 (a flush per slice
    at most) + ceil(waves / 64) + 6 additions; the division adds one."""
    depth = 2 * (per_wave // 64) + 6 + -(-waves // 64) + 6 + 1
    count = np.zeros(n_groups, dtype=np.int64)
    p, radius = np.full((n_groups, 3), np.nan, dtype=LD), np.full(n_groups, np.nan, dtype=LD)
    p_bound, r_bound = np.zeros((n_groups, 3)), np.zeros(n_groups)
    sel = np.flatnonzero(group >= 0)
    g = group[sel]
    np.add.at(count, g, 1)
    ends, starts = frame[sel, 9:12].astype(LD), frame[sel, 6:9].astype(LD)
    sums = np.zeros((n_groups, 12), dtype=LD)
    np.add.at(sums, g, np.concatenate([ends, starts, np.abs(ends), np.abs(starts)], 1))
    full = count > 0
    n = count[full].astype(LD)[:, None]
    p[full] = sums[full, 0:3] / n
    mean_start = sums[full, 3:6] / n
    p_bound[full] = SECOND_ORDER * gamma(depth) * (sums[full, 6:9] / n)
    s_bound = SECOND_ORDER * gamma(depth) * (sums[full, 9:12] / n)
    d = mean_start - p[full]
    radius[full] = np.sqrt((d * d).sum(1))
    # |d~ - d| <= the two means' bounds and the difference's rounding; |R~ - R| <= |d~ - d| (the norm is 1-Lipschitz),
    # and 4 u R for the squares, the sums and the root
    moved = p_bound[full] + s_bound + U * np.abs(d)
    r_bound[full] = SECOND_ORDER * (np.sqrt((moved * moved).sum(1)) + 4 * U * radius[full])
    return SimpleNamespace(count=count, p=p, radius=radius, p_bound=p_bound, r_bound=r_bound)


def wavefront_reference(frame, opl, group, n_groups, p, radius, terms, weights, n_rows, cus, fit_groups=None):
    """prt_frame_wavefront after pass 1, in longdouble with running bounds, over the rows with ``group`` >= 0 in row
    order.  Inputs as the device's second pass takes them: the frame, ``opl`` (n_rows, the device's), ``p`` (n_groups, 3)
    and ``radius`` (n_groups) -- the device's group records.  Returns per selected row ``hit``, ``opd`` and ``pupil``
    (NaN where the row misses) with ``opd_bound`` / ``pupil_bound``; per group ``n_rays``, ``n_missed``, ``sums`` and
    ``sums_bound`` (entries), ``rms``, ``pv`` and their bounds; for the groups of ``fit_groups`` (default: all) ``coef``,
    ``coef_bound`` and ``condition``."""
    sel = np.flatnonzero(group >= 0)
    g = group[sel]
    col = lambda name: frame[sel, IX[name]].astype(LD)  # noqa: E731
    q, u = [col("x1"), col("y1"), col("z1")], [col("x_tilt"), col("y_tilt"), col("z_tilt")]
    centre = [np.asarray(p, dtype=np.float64)[g, k].astype(LD) for k in range(3)]
    big_r = Err(np.asarray(radius, dtype=np.float64)[g].astype(LD))
    d = [Err(q[k]) - centre[k] for k in range(3)]
    a = Err(u[0]) * u[0] + Err(u[1]) * u[1] + Err(u[2]) * u[2]
    b = d[0] * u[0] + d[1] * u[1] + d[2] * u[2]
    c = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - big_r * big_r
    disc = b * b - a * c
    hit = (disc.v >= 0) & (a.v > 0)
    if np.any(np.abs(disc.v) <= disc.e):
        raise ValueError("a ray grazes the reference sphere within rounding: whether it counts is not determined")
    root = disc.where(hit, 1.0).sqrt()
    plus = b.v >= 0
    with np.errstate(all="ignore"):
        s = ((b + root) / a).where(plus, -c / (root - b).where(~plus, 1.0))
    e = [Err(q[k]) - s * u[k] for k in range(3)]
    opl_e = Err(np.asarray(opl, dtype=np.float64)[sel].astype(LD)) - Err(col("index")) * s
    # the pivot: the group's first row that meets the sphere
    n_rays, n_missed = np.zeros(n_groups, dtype=np.int64), np.zeros(n_groups, dtype=np.int64)
    np.add.at(n_rays, g[hit], 1)
    np.add.at(n_missed, g[~hit], 1)
    first = np.full(n_groups, -1, dtype=np.int64)
    with_rays, where = np.unique(g[hit], return_index=True)
    first[with_rays] = np.flatnonzero(hit)[where]
    pivot = opl_e.take(np.maximum(first[g], 0))
    v = opl_e - pivot  # (the OPD about the pivot: what the sums run over)
    w3 = [e[k] - centre[k] for k in range(3)]
    zero = Err(np.zeros(len(sel)))
    p1 = w3[0] * zero + w3[1] * 1.0 + w3[2] * zero
    p2 = w3[0] * zero + w3[1] * zero + w3[2] * 1.0
    radial = (p1 * p1 + p2 * p2).sqrt()
    extent, extent_e = np.zeros(n_groups, dtype=LD), np.zeros(n_groups, dtype=LD)
    np.maximum.at(extent, g[hit], radial.v[hit])
    np.maximum.at(extent_e, g[hit], radial.e[hit])  # (|max a~ - max a| <= max |a~ - a|)
    scale = Err(np.where(extent[g] > 0, extent[g], 1), extent_e[g])
    x, y = (p1 / scale).where(extent[g] > 0, 0.0), (p2 / scale).where(extent[g] > 0, 0.0)
    z = zernike_recurrence(terms, x.where(hit, 0.0), y.where(hit, 0.0))
    weight = Err(np.where(hit, col(weights) if weights else np.ones(len(sel), dtype=LD), 0))
    # the sums, per group: the rows sorted by group (stably: row order inside a group)
    entries = terms * (terms + 1) // 2 + terms + 3
    upper = np.triu_indices(terms)
    zv = np.stack([t.v for t in z], 1) * hit[:, None]
    ze = np.stack([t.e for t in z], 1).astype(np.float64) * hit[:, None]
    vv, ve = np.where(hit, v.v, 0), np.where(hit, v.e, 0).astype(np.float64)
    order = np.argsort(g, kind="stable")
    bounds = np.searchsorted(g[order], np.arange(n_groups + 1))
    zblocks = wf_zblocks(n_rows, n_groups, terms, cus)
    share = wf_zshare(len(sel), zblocks)
    sums, sums_bound = np.zeros((n_groups, entries), dtype=LD), np.zeros((n_groups, entries))
    for k in range(n_groups):
        r = order[bounds[k]:bounds[k + 1]]
        if not len(r):
            continue
        rows_here = min(share, len(r))
        depth = rows_here + -(-rows_here // WF_ZBLOCK) + 1 + -(-zblocks // 64) + 6
        w, zk, vk = weight.v[r], zv[r], vv[r]
        wz = zk * w[:, None]
        sums[k] = np.concatenate([(wz.T @ zk)[upper], wz.T @ vk, [w.sum(), (w * vk).sum(), (w * vk * vk).sum()]])
        # the bounds in fp64: sum |t| and the terms' own errors (two products: 2 u |t|, and what z and v carry)
        w64, az, ez, av, ev = w.astype(np.float64), np.abs(zk).astype(np.float64), ze[r], np.abs(vk).astype(np.float64), ve[r]
        waz, wez = az * w64[:, None], ez * w64[:, None]
        size = np.concatenate([(waz.T @ az)[upper], waz.T @ av, [w64.sum(), (w64 * av).sum(), (w64 * av * av).sum()]])
        own = np.concatenate([(waz.T @ ez + wez.T @ az + wez.T @ ez)[upper], waz.T @ ev + wez.T @ av + wez.T @ ev,
                              [0.0, (w64 * ev).sum(), (w64 * (2 * av * ev + ev * ev)).sum()]])
        own = own + 3 * U * size
        sums_bound[k] = SECOND_ORDER * (gamma(depth) * (size + own) + own)
    out = SimpleNamespace(rows=sel, group=g, hit=hit, n_rays=n_rays, n_missed=n_missed, sums=sums, sums_bound=sums_bound,
                          extent=extent, terms=terms)
    # rms, pv and the piston that comes off the per-row OPD
    s0, s1, s2 = sums[:, -3], sums[:, -2], sums[:, -1]
    b0, b1, b2 = sums_bound[:, -3], sums_bound[:, -2], sums_bound[:, -1]
    with np.errstate(all="ignore"):
        mean = s1 / s0
        d_mean = SECOND_ORDER * ((b1 + np.abs(mean) * b0) / (s0 - b0) + U * np.abs(mean))
        var = np.maximum(s2 / s0 - mean * mean, 0)
        d_var = SECOND_ORDER * ((b2 + (s2 / s0) * b0) / (s0 - b0) + 2 * np.abs(mean) * d_mean + d_mean ** 2
                                + 4 * U * (s2 / s0 + mean * mean))
        out.rms = np.sqrt(var)
        out.rms_bound = np.array([_root_bound(var[k], d_var[k]) if n_rays[k] else 0.0 for k in range(n_groups)])
    hi, lo = np.full(n_groups, -np.inf, dtype=LD), np.full(n_groups, np.inf, dtype=LD)
    worst = np.zeros(n_groups, dtype=LD)
    np.maximum.at(hi, g[hit], v.v[hit])
    np.minimum.at(lo, g[hit], v.v[hit])
    np.maximum.at(worst, g[hit], v.e[hit])
    out.pv = hi - lo
    out.pv_bound = (SECOND_ORDER * (2 * worst + U * np.abs(out.pv))).astype(np.float64)
    out.opd = np.where(hit, v.v - mean[g], np.nan)
    out.opd_bound = np.where(hit, SECOND_ORDER * (v.e + d_mean[g] + U * np.abs(v.v - mean[g])), 0).astype(np.float64)
    out.pupil = np.where(hit[:, None], np.stack([x.v, y.v], 1), np.nan)
    out.pupil_bound = np.where(hit[:, None], np.stack([x.e, y.e], 1), 0).astype(np.float64)
    # the fits
    out.coef, out.coef_bound, out.condition = {}, {}, {}
    tri = len(upper[0])
    for k in (range(n_groups) if fit_groups is None else fit_groups):
        if n_rays[k] == 0:
            continue
        normal = np.zeros((terms, terms), dtype=LD)
        normal[upper] = sums[k, :tri]
        normal = normal + np.triu(normal, 1).T
        rhs = sums[k, tri:tri + terms]
        n64 = normal.astype(np.float64)
        out.condition[k] = np.linalg.cond(n64)
        if not out.condition[k] < 1e10:  # (the product's RANK_RCOND: below full rank the fit is the minimum-norm one)
            continue
        coef = np.zeros(terms, dtype=LD)
        for _ in range(3):  # (fp64 solves refined on the longdouble residual)
            coef = coef + np.linalg.solve(n64, (rhs - normal @ coef).astype(np.float64)).astype(LD)
        d_n = np.zeros((terms, terms))
        d_n[upper] = sums_bound[k, :tri]
        d_n = d_n + np.triu(d_n, 1).T
        inverse = np.linalg.norm(np.linalg.inv(n64), 2)
        moved_n = np.linalg.norm(d_n, "fro") + gamma(4 * terms * terms) * np.linalg.norm(n64, "fro")
        moved_r = np.linalg.norm(sums_bound[k, tri:tri + terms]) + gamma(4 * terms * terms) * float(np.linalg.norm(rhs.astype(np.float64)))
        size = float(np.linalg.norm(coef.astype(np.float64)))
        out.coef[k] = coef
        out.coef_bound[k] = SECOND_ORDER * inverse * (moved_r + moved_n * size) / (1 - inverse * moved_n)
    return out


# ---- the frames of the wavefront tests ----------------------------------------------------------------------------------------
def slab_frame(n, seed=3, surfaces=(1.0, 2.0, 5.0), ids=None):
    """Three generations of n rays through an index-1.5 slab to a converging image space, with varied weights: the
    shape of tests/test_gpu_wavefront.py's synthetic_frame.  ids: ascending (default: a random subset of 0 .. 4n)."""
    rng = np.random.default_rng(seed)
    if ids is None:
        ids = np.sort(rng.choice(4 * n, n, replace=False))
    ids = np.asarray(ids, dtype=float)
    r, t = np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
    p0 = np.stack([np.full(n, -5.0), r * np.cos(t), r * np.sin(t)], 1)
    p1 = p0 + np.array([4.0, 0, 0]) + rng.normal(0, 1e-3, (n, 3))
    p2 = p1 + np.array([0.5, 0, 0])
    focus = np.array([10.0, 0.02, -0.01])
    dirn = focus - p2
    dirn /= np.linalg.norm(dirn, axis=1)[:, None]
    p3 = p2 + dirn * ((focus[0] + 0.3 - p2[:, 0]) / dirn[:, 0])[:, None] + rng.normal(0, 1e-4, (n, 3)) * [0, 1, 1]
    rows = []
    for g, (a, b, index, surf) in enumerate(((p0, p1, 1.0, surfaces[0]), (p1, p2, 1.5, surfaces[1]),
                                             (p2, p3, 1.0, surfaces[2]))):
        u = (b - a) / np.linalg.norm(b - a, axis=1)[:, None]
        block = np.zeros((n, 15))
        block[:, 0], block[:, 1], block[:, 2], block[:, 3] = g, 50 + 50 * rng.random(n), 0.633, index
        block[:, 4], block[:, 5], block[:, 6:9], block[:, 9:12], block[:, 12:15] = ids, surf, a, b, u
        rows.append(block)
    return np.concatenate(rows)


def sparse_frame(n_per_generation, places, seed=5, selected=5.0, other=6.0):
    """slab_frame(n_per_generation) with ids 0 .. n - 1, whose last generation lands on ``other`` but for the rows at
    ``places`` (row numbers of the whole frame, inside the last generation), which land on ``selected``."""
    frame = slab_frame(n_per_generation, seed, surfaces=(1.0, 2.0, other), ids=np.arange(n_per_generation))
    places = np.asarray(places, dtype=np.int64)
    assert places.min() >= 2 * n_per_generation and places.max() < 3 * n_per_generation
    frame[places, IX["surface"]] = selected
    return frame
