"""An integer restatement of the enclosed-energy definitions of include/prt.h (prt_frame_energy), with Python copies of
the partition rules of prt_energy.hpp / prt_mtf.hpp and the frames the tests run on.  It stands beside
tests/energy_reference.py (a float sort and searchsorted, valid where no ray lies near a radius) and decides every
comparison on bit images, so it holds with rays on radii, thresholds on cumulative sums and ties.

1. The partition (``slices`` .. ``digit_windows``): a group of ``count`` rays used is cut into chunks of kMtfChunk for
   the centroid sums and into ``slices(count)`` slices of ``slice_rays(count)`` rays for the curve and the select; the
   curve walks ``planes_per_tile`` planes a workgroup, the select kEnergyFractionTile fractions a launch; the radius
   bins and the digit windows each stay within kEnergySlabBytes.  tests/test_host_energy_sums.py holds the named
   constants and the restated lines to the headers' text.

2. Integers (``integer_weights``, ``enclosed``).  q = floor(ldexp(w, 62 - E - B)) and W = sum q, added as Python ints
   and asserted below 2^62.  d is evaluated in fp64 one rounded operation after another in energy_distance's order
   (numpy's ufuncs do not fuse; the library is built with -ffp-contract=off) and is used only through its uint64 bit
   image: for non-negative doubles bit order is numeric order, +inf sorts last, and a NaN coordinate gives +inf.
   EE = float(sum of q with bits(d) <= bits(R)) / float(W).  T_k = min(max(ceil(phi_k * float(W)), 1), W), and the radius
   is the smallest bit image whose cumulative q reaches T_k.  ``digit_path`` runs the select itself on Python ints: six
   passes of widths 11, 11, 11, 10, 10, 10, per pass the window of the keys that match the prefix, the digit where the
   running sum first reaches the residual, the residual left; it says at which passes more than one digit held weight
   (the passes that decided something).

3. The centre of a plane, c(delta) = pbar + delta sbar, in two forms.  *Exact* (``exact_centre``): p and s multiples of
   2^-8, w multiples of 1/8; every w p and w s is an integer of 2^-11 and, while the absolute values add up to less
   than 2^53 units (``require_exact``: a condition, not a tolerance), every partial sum of k_energy_centre's fma chain,
   its tree and k_energy_record's fold is a double, so pbar = float(S1) / float(S0) is one correctly rounded division
   whatever the order.  *Given*: the caller passes the device's own pbar and sbar (record[:, 3:7]); everything after them
   is a function of bits.  The device's pbar, sbar and sum w are then held to ``centre_bound``, u = 2^-53, gamma(k) =
   k u / (1 - k u): a term of k_energy_centre passes at most ceil(kMtfChunk / kEnergyBlock) = 16 additions in its
   thread (the products enter by fma: one more rounding for sum w p and sum w s), 8 in the tree of 256 and one per chunk
   of the group in k_energy_record's serial fold -- ``centre_depth`` -- and the quotient rounds once:
        |D~ - D| <= gamma(depth) D                                              (D = sum w, w >= 0)
        |m~ - m| <= (gamma(depth + 1) sum |w p| + |m| gamma(depth) D) / (D (1 - gamma(depth))) + u |m|
   with the factor 1.001 for the terms of second order; the sums themselves are formed in longdouble.

4. Staging (``stage``): mtf_stage_ray's operation sequence in fp64 about given centres C_g (a given reference, or the
   device's own centroid from record[:, 0:3]), so that the staged (p, s, w) are the device's bits on any frame.

Largest deviation-to-bound ratios seen on an MI355X (tests/test_gpu_energy_partitions.py prints them; none is fixed in
advance):
    pbar 0.023, sbar 0.0040, sum w 0.033
Energies, radii, T_k and the counts have no ratio: they are equal or the test fails.
"""
import math
from types import SimpleNamespace

import numpy as np

import frame_sums_reference as sums
from frame_sums_reference import IX, LD, SECOND_ORDER, U, NotExact, gamma, require_exact  # noqa: F401

ROOT = sums.ROOT
SHAPES = ("circle", "square", "slit_e1", "slit_e2")
DEFAULT_AXES = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
INF_BITS = 0x7FF0000000000000

# ---- named copies of the constants (test_host_energy_sums.py holds them to the headers) -----------------------------------
MTF_CHUNK = 4096                 # prt_mtf.hpp: static const int kMtfChunk = 4096;
MTF_MIN_SLICE = 2048             # prt_mtf.hpp: static const int kMtfMinSlice = 2048;
MTF_MAX_SLICES = 256             # prt_mtf.hpp: static const int kMtfMaxSlices = 256;
ENERGY_BLOCK = 256               # prt_energy.hpp: static const int kEnergyBlock = 256;
ENERGY_WINDOW = 4096             # prt_energy.hpp: static const int kEnergyWindow = 4096;
ENERGY_DIGITS = 2048             # prt_energy.hpp: static const int kEnergyDigits = 2048;
ENERGY_FRACTION_TILE = 4         # prt_energy.hpp: static const int kEnergyFractionTile = 4;
ENERGY_PASSES = 6                # prt_energy.hpp: static const int kEnergyPasses = 6;
ENERGY_SLAB_BYTES = 256 << 20    # prt_energy.hpp: static const size_t kEnergySlabBytes = 256u << 20;
ENERGY_WIDTH = (11, 11, 11, 10, 10, 10)   # prt_energy.hpp: kEnergyWidth
ENERGY_LOW = (52, 41, 30, 20, 10, 0)      # prt_energy.hpp: kEnergyLow
BLOCK = sums.BLOCK               # prt_device.hpp: #define PRT_BLOCK 256
HEADER_NAMES = dict(kMtfChunk="MTF_CHUNK", kMtfMinSlice="MTF_MIN_SLICE", kMtfMaxSlices="MTF_MAX_SLICES",
                    kEnergyBlock="ENERGY_BLOCK", kEnergyWindow="ENERGY_WINDOW", kEnergyDigits="ENERGY_DIGITS",
                    kEnergyFractionTile="ENERGY_FRACTION_TILE", kEnergyPasses="ENERGY_PASSES",
                    kEnergySlabBytes="ENERGY_SLAB_BYTES")
HOST_RULES = {
    "prt_mtf.hpp": (
        "const int64_t s = (count + kMtfMinSlice - 1) / kMtfMinSlice;",
        "return s < 1 ? 1 : (s > max_slices ? max_slices : s);",
        "const int64_t slices = slice_start[g + 1] - slice_start[g], per = (count + slices - 1) / slices;",
        "hi = lo + per < first[g] + count ? lo + per : first[g] + count;",
        "n_groups, [&](int64_t g) { return (bucket_total[g] + kMtfChunk - 1) / kMtfChunk; },",
        "hi = lo + kMtfChunk < end ? lo + kMtfChunk : end;"),
    "prt_sort.hpp": (
        "for (int half = BLOCK / 2; half > 0; half >>= 1) {",),
    "prt_energy.hpp": (
        "static const int kEnergyWidth[kEnergyPasses] = {11, 11, 11, 10, 10, 10};",
        "static const int kEnergyLow[kEnergyPasses] = {52, 41, 30, 20, 10, 0};",
        "const MtfRowPlan row = mtf_row_plan(n_rows, n_groups, kMtfMaxSlices);",
        "const int planes_per_tile = n_radii ? std::max(1, std::min(n_focus, kEnergyWindow / n_radii)) : 1;",
        "const int plane_tiles = (n_focus + planes_per_tile - 1) / planes_per_tile;",
        "for (int first = 0; first < n_fractions; first += kEnergyFractionTile)",
        "std::min(kEnergyFractionTile, n_fractions - first), kEnergyLow[pass], kEnergyWidth[pass],",
        "if ((size_t)n_groups * n_focus * n_radii * 8 > kEnergySlabBytes)",
        "if ((size_t)n_groups * n_focus * n_fractions * kEnergyDigits * 8 > kEnergySlabBytes)",
        "for (int64_t r = lo + t; r < hi; r += kEnergyBlock) {",
        "__shared__ double red[6][kEnergyBlock];",
        "sort_tree(red, t, [](int k, double& a, double b) { a = k < 5 ? a + b : (b > a ? b : a); });",
        "for (int64_t q = chunk_start[g]; q < chunk_start[g + 1]; ++q)",
        "return 62 - e - (64 - __clzll(count));",
        "shift[g] = energy_shift(w_max[g], (long long)bucket_total[g]);",
        "u64 need = (u64)ceil(fractions[item % n_fractions] * (double)all);",
        "need = need < 1 ? 1 : (need > all ? all : need);"),
}


# ---- 1. the partition rules ---------------------------------------------------------------------------------------------
def chunks(count):
    """The chunks of kMtfChunk rays of a group of ``count`` rays used (k_energy_centre, k_energy_scale)."""
    return -(-count // MTF_CHUNK)


def slices(count):
    """mtf_slices with kMtfMaxSlices: at least kMtfMinSlice rays a slice while the group has them, 256 at most."""
    return min(max(-(-count // MTF_MIN_SLICE), 1), MTF_MAX_SLICES)


def slice_rays(count):
    """mtf_slice's ``per``: the rays of a full slice."""
    return -(-count // slices(count))


def slice_bounds(count):
    """[lo, hi) of every slice within the group's rays; a slice past the group's end is empty (lo >= hi)."""
    per = slice_rays(count)
    return [(k * per, min(k * per + per, count)) for k in range(slices(count))]


def planes_per_tile(n_focus, n_radii):
    return max(1, min(n_focus, ENERGY_WINDOW // n_radii)) if n_radii else 1


def plane_tiles(n_focus, n_radii):
    """The planes of every curve tile: all ``planes_per_tile`` but a ragged last one."""
    per = planes_per_tile(n_focus, n_radii)
    return [min(per, n_focus - first) for first in range(0, n_focus, per)]


def fraction_tiles(n_fractions):
    """(first, count) of every select launch of a pass."""
    return [(first, min(ENERGY_FRACTION_TILE, n_fractions - first))
            for first in range(0, n_fractions, ENERGY_FRACTION_TILE)]


def digit_windows(n_groups, n_focus, n_fractions):
    return n_groups * n_focus * n_fractions


def within_caps(n_groups, n_focus, n_radii, n_fractions):
    """The two 256 MiB caps of prt_frame_energy: the radius bins and the digit windows."""
    return (n_groups * n_focus * n_radii * 8 <= ENERGY_SLAB_BYTES
            and digit_windows(n_groups, n_focus, n_fractions) * ENERGY_DIGITS * 8 <= ENERGY_SLAB_BYTES)


def centre_depth(count):
    """The additions a term of sum w passes at most: its thread, the tree, the fold of the group's chunks."""
    return -(-MTF_CHUNK // ENERGY_BLOCK) + int(math.log2(ENERGY_BLOCK)) + chunks(count)


# ---- 2. integers ------------------------------------------------------------------------------------------------------------
def bits(d):
    """The uint64 bit image of doubles."""
    return np.ascontiguousarray(np.asarray(d, dtype=np.float64)).view(np.uint64)


def from_bits(k):
    return np.asarray(k, dtype=np.uint64).view(np.float64)


def weight_shift(w):
    """62 - E - B with w_max = f 2^E (0.5 <= f < 1) and B = bit_length(rays used); None where no weight is positive."""
    w = np.asarray(w, dtype=np.float64)
    if not len(w) or not w.max() > 0:
        return None
    _, e = math.frexp(float(w.max()))
    return 62 - e - int(len(w)).bit_length()


def integer_weights(w):
    """(q as uint64, W as a Python int): q = floor(ldexp(w, shift)); the sum is taken over Python ints."""
    w = np.asarray(w, dtype=np.float64)
    shift = weight_shift(w)
    if shift is None:
        return np.zeros(len(w), dtype=np.uint64), 0
    scaled = [math.floor(math.ldexp(v, shift)) for v in w.tolist()]   # (Python ints: floor of an exact scaling)
    total = sum(scaled)
    assert 0 <= min(scaled) and total < 2 ** 62, (total, shift)
    return np.array(scaled, dtype=np.uint64), total


def distances(p, s, delta, c, shape):
    """d of every ray at the plane shifted by delta about c, in energy_distance's order: x = (p + delta s) - c."""
    p, s = np.asarray(p, dtype=np.float64), np.asarray(s, dtype=np.float64)
    delta = np.float64(delta)
    with np.errstate(all="ignore"):
        product = delta * s
        x = (p + product) - np.asarray(c, dtype=np.float64)
        bad = np.isnan(x).any(axis=1)
        if shape == "circle":
            a, b = x[:, 0] * x[:, 0], x[:, 1] * x[:, 1]
            d = np.sqrt(a + b)
        elif shape == "square":
            a1, a2 = np.abs(x[:, 0]), np.abs(x[:, 1])
            d = np.where(a1 > a2, a1, a2)
        elif shape == "slit_e2":
            d = np.abs(x[:, 0])
        elif shape == "slit_e1":
            d = np.abs(x[:, 1])
        else:
            raise ValueError(shape)
    d = np.where(bad, np.inf, d)
    assert not np.isnan(d).any() and not np.signbit(d).any()
    return d


def plane_centre(mean, delta, follow_centroid):
    """c(delta) = pbar + delta sbar from mean = (pbar1, pbar2, sbar1, sbar2): the product rounded, then the sum."""
    if not follow_centroid:
        return np.zeros(2)
    mean = np.asarray(mean, dtype=np.float64)
    with np.errstate(all="ignore"):
        product = np.float64(delta) * mean[2:4]
        return mean[0:2] + product


def thresholds(fractions, total):
    """T_k = min(max(ceil(phi_k * float(W)), 1), W) as Python ints; the product is fp64's."""
    return [min(max(math.ceil(float(np.float64(phi) * np.float64(total))), 1), total) for phi in fractions]


def digit_path(keys, q, need):
    """The select on Python ints.  keys: the bit images (ints) of the group's distances at a plane, q their integer
    weights, need: T_k.  Per pass (prefix after it, residual after it, digits of the window that held weight).  The last
    prefix is the radius' bit image."""
    prefix, out = 0, []
    for low, width in zip(ENERGY_LOW, ENERGY_WIDTH):
        window = {}
        for key, weight in zip(keys, q):
            if weight and key >> (low + width) == prefix:
                digit = (key >> low) & ((1 << width) - 1)
                window[digit] = window.get(digit, 0) + weight
        below = 0
        for digit in sorted(window):
            if below + window[digit] >= need:
                prefix, need = (prefix << width) | digit, need - below
                break
            below += window[digit]
        else:
            raise AssertionError("the window's total is below the residual threshold")
        out.append((prefix, need, len(window)))
    return out


def deciding_passes(path):
    """The passes at which more than one digit of the window held weight: where the select chose among keys."""
    return [k for k, (_, _, held) in enumerate(path) if held > 1]


def pass_of_bit(bit):
    """The pass whose digit holds bit ``bit`` of the key."""
    return next(k for k, low in enumerate(ENERGY_LOW) if bit >= low)


def enclosed(p, s, w, radii=(), fractions=(), focus=(0.0,), shape="circle", follow_centroid=True, mean=None):
    """One group from its staged rays p (n, 2), s (n, 2), w (n).  mean: (pbar1, pbar2, sbar1, sbar2) -- the device's
    (given form) or None for ``exact_centre`` (needed only with follow_centroid).  Returns q, W, T (Python ints),
    bins (n_focus, n_radii) uint64: the q with R_(j-1) < d <= R_j; energy (n_focus, n_radii); radius (n_focus,
    n_fractions); keys (n_focus, n) uint64: the distances' bit images; on (n_focus, n_radii): the rays whose distance
    equals the radius bit for bit."""
    p, s, w = (np.asarray(v, dtype=np.float64) for v in (p, s, w))
    radii, fractions = np.asarray(radii, dtype=np.float64), np.asarray(fractions, dtype=np.float64)
    q, total = integer_weights(w)
    out = SimpleNamespace(q=q, W=total, T=[], mean=None,
                          bins=np.zeros((len(focus), len(radii)), dtype=np.uint64),
                          energy=np.full((len(focus), len(radii)), np.nan),
                          radius=np.full((len(focus), len(fractions)), np.nan),
                          keys=np.zeros((len(focus), len(w)), dtype=np.uint64),
                          on=np.zeros((len(focus), len(radii)), dtype=np.int64))
    if total == 0:
        return out
    if follow_centroid and mean is None:
        mean = exact_centre(p, s, w).mean
    out.mean = mean
    out.T = thresholds(fractions, total)
    need = np.array(out.T, dtype=np.uint64)
    edge = bits(radii)
    for f, delta in enumerate(focus):
        key = bits(distances(p, s, delta, plane_centre(mean, delta, follow_centroid), shape))
        out.keys[f] = key
        order = np.argsort(key, kind="stable")
        key_sorted, run = key[order], np.cumsum(q[order], dtype=np.uint64)
        assert int(run[-1]) == total
        inside = np.searchsorted(key_sorted, edge, side="right")   # the rays with bits(d) <= bits(R)
        below = np.concatenate([np.zeros(1, dtype=np.uint64), run])[inside]
        out.bins[f] = np.diff(np.concatenate([np.zeros(1, dtype=np.uint64), below]))
        out.energy[f] = np.array([float(int(v)) / float(total) for v in below])
        out.on[f] = inside - np.searchsorted(key_sorted, edge, side="left")
        out.radius[f] = from_bits(key_sorted[np.searchsorted(run, need, side="left")])
    return out


# ---- 3. the centre of a plane -------------------------------------------------------------------------------------------------
GRID = 256       # p and s: multiples of 2^-8
WEIGHT_GRID = 8  # w: multiples of 1/8


def exact_centre(p, s, w):
    """pbar, sbar and sum w of a group on the grid, from integers: ``mean`` (4) and ``sum_w``; NotExact / ValueError
    where a sum would not be representable or a value is off the grid."""
    p, s, w = (np.asarray(v, dtype=np.float64) for v in (p, s, w))
    wk = sums.to_grid(w, "w", WEIGHT_GRID)
    columns = [wk] + [wk * sums.to_grid(v[:, k], name, GRID) for v, name in ((p, "p"), (s, "s")) for k in range(2)]
    require_exact(columns)
    totals = [sum(column.tolist()) for column in columns]   # (Python ints)
    sum_w = float(totals[0]) / WEIGHT_GRID
    with np.errstate(all="ignore"):
        mean = np.array([np.float64(float(t) / (GRID * WEIGHT_GRID)) / np.float64(sum_w) for t in totals[1:]])
    return SimpleNamespace(mean=mean, sum_w=sum_w)


def centre_bound(p, s, w):
    """longdouble pbar, sbar (``mean``, 4) and sum w with the bounds the module docstring derives: ``mean_bound`` (4),
    ``sum_w_bound``."""
    p, s, w = (np.asarray(v, dtype=LD) for v in (p, s, w))
    depth = centre_depth(len(w))
    g0, g1 = gamma(depth), gamma(depth + 1)
    total = w.sum()
    terms = np.concatenate([w[:, None] * p, w[:, None] * s], 1)
    mean = terms.sum(0) / total
    size = np.abs(terms).sum(0)
    moved = (g1 * size + np.abs(mean) * g0 * total) / (total * (1 - g0)) + U * np.abs(mean)
    return SimpleNamespace(mean=mean, mean_bound=(SECOND_ORDER * moved).astype(np.float64), sum_w=total,
                           sum_w_bound=float(SECOND_ORDER * g0 * total), depth=depth)


# ---- 4. staging ---------------------------------------------------------------------------------------------------------------
def _dot(v, e):
    return v[:, 0] * float(e[0]) + v[:, 1] * float(e[1]) + v[:, 2] * float(e[2])   # (left to right, nothing fused)


def stage(frame, surface, centres, axes=DEFAULT_AXES, rays_per_source=None, n_groups=1, weights="intensity"):
    """Per group (p, s, w, rays used, rays left out) in row order: mtf_ray's test and mtf_stage_ray's operations about
    ``centres`` (n_groups, 3)."""
    axes = np.asarray(axes, dtype=np.float64)
    a, e1, e2 = axes[0:3], axes[3:6], axes[6:9]
    centres = np.broadcast_to(np.asarray(centres, dtype=np.float64), (n_groups, 3))
    group = sums.selection(frame, surface, None, rays_per_source, n_groups)
    q, u = frame[:, 9:12], frame[:, 12:15]
    w = np.ones(len(frame)) if weights is None else frame[:, IX[weights]]
    with np.errstate(all="ignore"):
        ua = _dot(u, a)
        s = np.stack([_dot(u, e1) / ua, _dot(u, e2) / ua], 1)
        ok = (w >= 0) & (w < np.inf) & (np.abs(q) < np.inf).all(1) & (np.abs(u) < np.inf).all(1) & (ua != 0)
        ok &= (np.abs(s) < np.inf).all(1)
    out = []
    for g in range(n_groups):
        m = ok & (group == g)
        with np.errstate(all="ignore"):
            d = q[m] - centres[g]
            da = _dot(d, a)
            p = np.stack([_dot(d, e1) - s[m, 0] * da, _dot(d, e2) - s[m, 1] * da], 1)
        out.append((p, s[m], w[m], int(m.sum()), int(((group == g) & ~ok).sum())))
    return out


# ---- frames -----------------------------------------------------------------------------------------------------------------
def plane_frame(p, s, w, ids=None, surface=4.0):
    """Rows at ``surface`` whose staged rays about the origin with the default axes are exactly (p, s, w): Q = (0, p),
    u = (1, s) (tests/test_gpu_enclosed_energy.plane_frame)."""
    p, s = np.asarray(p, dtype=float).reshape(-1, 2), np.asarray(s, dtype=float).reshape(-1, 2)
    frame = np.zeros((len(p), 15))
    frame[:, IX["intensity"]], frame[:, IX["surface"]] = w, surface
    frame[:, IX["id"]] = np.arange(len(p)) if ids is None else ids
    frame[:, 10:12], frame[:, 12], frame[:, 13:15] = p, 1.0, s
    return frame


def dyadic_rays(n, seed, unit_weights=False, reach=4):
    """p and s multiples of 2^-8 within +-reach, w multiples of 1/8 below 8 (zero for about one ray in eight) or 1."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-reach * GRID + 1, reach * GRID, (n, 2)) / GRID
    s = rng.integers(-reach * GRID + 1, reach * GRID, (n, 2)) / GRID
    w = np.ones(n) if unit_weights else rng.integers(1, 8 * WEIGHT_GRID, n) / WEIGHT_GRID * (rng.random(n) > 0.125)
    return p, s, w


def pythagorean_rays(n, seed, reach=4):
    """Points on the 2^-8 grid whose distance from the origin is on the grid too: multiples of the triples (3, 4, 5),
    (5, 12, 13), (8, 15, 17), (7, 24, 25) and of the axes, in all eight orientations.  sqrt(x1 x1 + x2 x2) is exact."""
    rng = np.random.default_rng(seed)
    triples = np.array([(3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (0, 1, 1), (1, 0, 1)])
    pick = triples[rng.integers(0, len(triples), n)]
    scale = np.array([rng.integers(1, reach * GRID // t[2] + 1) for t in pick])
    p = pick[:, :2] * scale[:, None] * rng.choice([-1, 1], (n, 2))
    swap = rng.random(n) < 0.5
    p[swap] = p[swap][:, ::-1]
    root = pick[:, 2] * scale
    assert np.array_equal(p[:, 0] ** 2 + p[:, 1] ** 2, root ** 2) and root.max() <= reach * GRID
    return p / GRID, root / GRID
