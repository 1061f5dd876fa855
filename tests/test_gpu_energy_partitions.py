"""The enclosed energy on the device (DeviceFrame.enclosed_energy) against the integer restatement of its definitions
(tests/energy_sums_reference.py), where an exact count can break: rays on radii and one ulp beside them, thresholds on
cumulative sums, the floor and the power-of-two edges of the integer weights, every edge of the curve's plane tiles, of
the fraction tiles, of the slices and chunks and of the digit-window cap, ties across slices, and keys that one digit
level of the select decides alone.  Energies, radii and counts are compared on bit images.  On dyadic frames pbar, sbar
and sum w are integers' quotients and compared on bit images too; on frames on no grid they are held to the derived bound
(deviation / bound <= 1, printed) and everything after them is computed from the device's own values, bit for bit.
Every case asserts the arm it is named for.  No case is sampled or filtered by its result."""
import numpy as np
import pytest

import energy_sums_reference as ref
import helpers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORIGIN = dict(reference=(0.0, 0.0, 0.0))
SIXTEENTHS = tuple(k / 16 for k in range(1, 17))
RATIOS = dict(pbar=0.0, sbar=0.0, sum_w=0.0)


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(ref.bits(a[~nan]), ref.bits(b[~nan]))


class Case:
    """A frame on the device and its staged rays on the host.  centre: "exact" (a dyadic frame: pbar, sbar and sum w
    from integers, compared on bits), "given" (the device's pbar and sbar are held to the bound and passed on) or "none"
    (follow_centroid=False and weights whose float sums mean nothing: the record's means are not read)."""

    def __init__(self, frame, surface=4.0, centre="exact", **options):
        from pyrayt_amd.frame import pupil_axes

        self.frame, self.surface, self.centre, self.options = frame, surface, centre, options
        self.focus = tuple(options.get("focus", (0.0,)))
        self.shape, self.follow = options.get("shape", "circle"), options.get("follow_centroid", True)
        self.n_groups = options.get("n_groups", 1)
        assert centre in ("exact", "given") or not self.follow
        self.device = device_frame(frame)
        # the record (C_g, pbar, sbar) does not depend on the radii or fractions: one call ahead reads it
        self.record = self.device.enclosed_energy(surface, None, **dict(options, fractions=(0.5,))).record
        reference = options.get("reference", "centroid")
        centres = self.record[:, :3] if isinstance(reference, str) else reference
        self.groups = ref.stage(frame, surface, centres, pupil_axes(options.get("axis")), options.get("rays_per_source"),
                                self.n_groups, options.get("weights", "intensity"))
        self.means = []
        for g, (p, s, w, used, _) in enumerate(self.groups):
            live = used > 0 and w.max() > 0
            if not self.follow or not live:
                self.means.append(None)
            elif centre == "exact":
                self.means.append(ref.exact_centre(p, s, w).mean)
            else:
                self.means.append(self.record[g, 3:7].copy())

    def distances(self, g):
        """(n_focus, n) distances of group g's rays, from the centre the comparison will use."""
        p, s, w, _, _ = self.groups[g]
        return np.stack([ref.distances(p, s, delta, ref.plane_centre(self.means[g], delta, self.follow and
                                                                     self.means[g] is not None), self.shape)
                         for delta in self.focus])

    def radii_on_rays(self, count, zero=False):
        """Radii that are rays' own distances (up to ``count`` of every group that has rays, spread over its planes),
        the doubles next below and next above each, and 0."""
        picks = []
        for g in range(self.n_groups):
            if self.groups[g][3]:
                d = np.unique(self.distances(g).reshape(-1))
                d = d[np.isfinite(d)]
                picks.append(d[np.unique(np.linspace(0, len(d) - 1, count).round().astype(int))])
        picks = np.unique(np.concatenate(picks))
        more = [picks, np.nextafter(picks[picks > 0], 0.0), np.nextafter(picks, np.inf)] + ([[0.0]] if zero else [])
        return np.unique(np.concatenate(more))

    def check(self, radii, fractions):
        """The device against the integers: every energy, every radius, the counts; the centre by its form."""
        got = self.device.enclosed_energy(self.surface, radii, **dict(self.options, fractions=fractions))
        assert np.array_equal(ref.bits(got.record), ref.bits(self.record))   # (the same bits on every run)
        radii = () if radii is None else radii
        fractions = () if fractions is None else fractions
        assert got.energy.shape == (self.n_groups, len(self.focus), len(radii))
        assert got.radius.shape == (self.n_groups, len(self.focus), len(fractions))
        wants = []
        for g, (p, s, w, used, missed) in enumerate(self.groups):
            assert (got.n_rays[g], got.n_missed[g]) == (used, missed), g
            want = ref.enclosed(p, s, w, radii, fractions, self.focus, self.shape, self.follow, mean=self.means[g])
            wants.append(want)
            if want.W == 0:
                assert np.all(np.isnan(got.energy[g])) and np.all(np.isnan(got.radius[g])), g
                continue
            if self.centre == "exact":
                exact = ref.exact_centre(p, s, w)
                assert same_bits(got.record[g, 3:7], exact.mean) and got.sum_weights[g] == exact.sum_w, g
            elif self.centre == "given":
                bound = ref.centre_bound(p, s, w)
                off = np.abs(got.record[g, 3:7].astype(ref.LD) - bound.mean).astype(np.float64) / bound.mean_bound
                off_w = float(abs(ref.LD(got.sum_weights[g]) - bound.sum_w)) / bound.sum_w_bound
                for name, value in (("pbar", off[:2].max()), ("sbar", off[2:].max()), ("sum_w", off_w)):
                    RATIOS[name] = max(RATIOS[name], float(value))
                assert off.max() <= 1 and off_w <= 1, (g, off, off_w)
            assert same_bits(got.energy[g], want.energy), (g, np.argwhere(got.energy[g] != want.energy)[:5])
            assert same_bits(got.radius[g], want.radius), (g, got.radius[g], want.radius)
        return got, wants


def print_ratios():
    print("deviation / bound so far: pbar %.3g, sbar %.3g, sum w %.3g" % (RATIOS["pbar"], RATIOS["sbar"], RATIOS["sum_w"]))


# ---- rays on radii ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", (False, True))
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_rays_on_radii_on_dyadic_frames(shape, follow):
    """Two groups on the 2^-8 grid (2500 rays of mixed weights, 700 of weight 1 of which 300 have exact roots), three
    dyadic shifts; the radii are rays' distances, the doubles beside them and 0, with rays at distance 0."""
    p, s, w = ref.dyadic_rays(2500, 51)
    p[:40], s[:40] = 0.0, 0.0
    exact, root = ref.pythagorean_rays(300, 52)
    p1, s1, w1 = ref.dyadic_rays(400, 53, unit_weights=True)
    p1[:25], s1[:25] = 0.0, 0.0
    p = np.concatenate([p, exact, p1])
    s = np.concatenate([s, np.zeros_like(exact), s1])
    w = np.concatenate([w, np.ones(300), w1])
    ids = np.concatenate([np.arange(2500), 4000 + np.arange(700)])
    case = Case(ref.plane_frame(p, s, w, ids), shape=shape, follow_centroid=follow, focus=(-0.5, 0.0, 0.25),
                rays_per_source=4000, n_groups=2, **ORIGIN)
    radii = case.radii_on_rays(60, zero=True)
    got, wants = case.check(radii, (0.01, 0.1, 0.5, 0.9, 1.0))
    for want in wants:
        assert (want.on > 0).sum() >= 20   # (the arm: rays whose distance is a radius, bit for bit)
    if not follow:
        assert wants[0].on[1, 0] >= 40 and wants[1].on[1, 0] >= 25 and radii[0] == 0.0   # (rays at 0, radius 0)
        if shape == "circle":   # (roots that are exact: the rays lie on their radius whatever sqrt's last bit is)
            assert np.array_equal(case.distances(1)[1, :300], root)


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_a_radius_shared_by_5000_rays_across_slices_and_chunks(shape):
    """6145 rays of weight 1: 5000 at (+-3, +-3) -- the same distance in every shape -- among 1145 on the grid."""
    n, tied = 6145, 5000
    p, s, w = ref.dyadic_rays(n, 61, unit_weights=True)
    s[:] = 0.0
    where = np.sort(np.random.default_rng(62).choice(n, tied, replace=False))
    p[where] = 3.0 * np.random.default_rng(63).choice([-1.0, 1.0], (tied, 2))
    case = Case(ref.plane_frame(p, s, w), shape=shape, follow_centroid=False, **ORIGIN)
    d = case.distances(0)[0]
    shared = d[where[0]]
    assert np.all(d[where] == shared) and (d == shared).sum() >= tied
    bounds = ref.slice_bounds(n)
    assert ref.slices(n) == 4 and ref.chunks(n) == 2 and all(np.any((where >= lo) & (where < hi)) for lo, hi in bounds)
    assert np.any(where < ref.MTF_CHUNK) and np.any(where >= ref.MTF_CHUNK)
    radii = np.unique(np.concatenate([case.radii_on_rays(8), [np.nextafter(shared, 0.0), shared, np.nextafter(shared, 9.0)]]))
    got, (want,) = case.check(radii, SIXTEENTHS)
    at = int(np.flatnonzero(radii == shared)[0])
    assert want.on[0, at] >= tied and (got.radius[0, 0] == shared).sum() >= 8   # (thresholds inside the tie)
    assert int(want.bins[0, at]) >= tied * (want.W // n) and want.W % n == 0   # (the tie's weight in one bin, in integers)


# ---- thresholds on cumulative sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_thresholds_on_cumulative_sums(shape):
    """4800 rays of weight 1 with distinct distances; phi = k / 16 puts T_k on a cumulative sum, phi one ulp beside it
    does not; a tiny phi asks for one unit of weight."""
    n = 4800
    p, s, w = ref.dyadic_rays(n, 41, unit_weights=True)
    case = Case(ref.plane_frame(p, s, w), shape=shape, follow_centroid=False, focus=(0.25,), **ORIGIN)
    d = np.sort(case.distances(0)[0])
    for fractions in (SIXTEENTHS, tuple(np.nextafter(SIXTEENTHS[:-1], 0.0)) + (5e-324,),
                      tuple(np.nextafter(SIXTEENTHS[:-1], 1.0)) + (1e-30,)):
        got, (want,) = case.check(None, fractions)
        unit = want.W // n
        count = [-(-t // unit) for t in want.T]   # (the rays the threshold needs)
        assert want.W == n * unit and np.array_equal(got.radius[0, 0], d[np.array(count) - 1])
        if fractions is SIXTEENTHS:   # (the arm: every threshold is a cumulative sum, and the next ray is another one)
            assert want.T == [k * (n // 16) * unit for k in range(1, 17)]
            assert np.all(d[np.array(count[:-1])] >= got.radius[0, 0, :-1])
        elif fractions[-1] == 5e-324:
            assert count[:-1] == [k * (n // 16) for k in range(1, 16)] and want.T[-1] == 1
            assert all(t % unit for t in want.T[:-1])   # (below the sum: the same ray, but not by equality)
        else:
            assert count[:-1] == [k * (n // 16) + 1 for k in range(1, 16)] and want.T[-1] == 1
            # (phi W > 0 for every phi > 0 and W >= 1: ceil gives 1 and the lower clamp has nothing left to do)
            assert got.radius[0, 0, -1] == d[0]


def test_the_upper_clamp_decides_where_the_total_rounds_up():
    """Seven rays of weight 1 + 2^-52: W = 7 2^58 + 448 lies between two doubles and rounds up, so ceil(1.0 * (double) W)
    is above W and the radius at phi = 1 is the farthest ray only because of the clamp."""
    w = np.full(7, np.nextafter(1.0, 2.0))
    p = np.stack([np.arange(1.0, 8.0), np.zeros(7)], 1)[[3, 6, 0, 5, 1, 4, 2]]
    case = Case(ref.plane_frame(p, np.zeros((7, 2)), w), centre="none", shape="slit_e2", follow_centroid=False, **ORIGIN)
    got, (want,) = case.check([1.0, 6.5, 7.0], (1.0, np.nextafter(1.0, 0.0), 6 / 7))
    assert want.W == 7 * 2 ** 58 + 448 and float(want.W) > want.W
    assert int(np.ceil(1.0 * float(want.W))) > want.W and want.T[0] == want.W   # (the arm: the clamp decides)
    assert got.radius[0, 0, 0] == 7.0 and got.energy[0, 0, 2] == 1.0


# ---- the integer weights ------------------------------------------------------------------------------------------------------
def weight_groups():
    """Per group its weights (distances ascend with the position, so the first rays show alone in the first energies)
    and what to call it."""
    out = []
    for top in (0.75, 1.0, 8.0, np.nextafter(8.0, 0.0), 2.0 ** -20, 5e-324 * 2 ** 20, 5e-324 * 3, 1e308, 2.0 ** 1023):
        n = 9
        e = int(np.frexp(top)[1])
        unit = np.ldexp(1.0, e - 62 + int(n).bit_length())   # (one quantum: w_max 2^-(61 - B) for f = 1/2)
        w = np.array([unit, unit / 2, 1.5 * unit, 0.0, 2.5 * unit, top, 0.0, top / 2, 3 * unit])
        out.append((w, "w_max %r" % top))
    return out


def test_floor_at_the_quantum_and_the_edges_of_the_weights():
    """w_max, one quantum of it, half of one (counts 0), one and a half (counts 1: floor, not round), zeros; w_max on a
    power of two and just below; subnormal and near the top of the doubles; a group with no weight between live ones."""
    groups = weight_groups()
    groups.insert(4, (np.zeros(9), "no weight"))
    per = 16
    w = np.concatenate([g[0] for g in groups])
    ids = np.concatenate([k * per + np.arange(len(g[0])) for k, g in enumerate(groups)])
    p = np.stack([np.tile(np.arange(1.0, 10.0), len(groups)), np.zeros(len(w))], 1)
    case = Case(ref.plane_frame(p, np.zeros_like(p), w, ids), centre="none", shape="slit_e2", follow_centroid=False,
                rays_per_source=per, n_groups=len(groups), **ORIGIN)
    got, wants = case.check(np.arange(1.0, 10.0), (5e-324, 0.5, 1.0))
    for k, ((weights, name), want) in enumerate(zip(groups, wants)):
        if name == "no weight":
            assert want.W == 0 and np.all(np.isnan(got.energy[k])) and np.all(np.isnan(got.radius[k]))
            continue
        subnormal_unit = weights[0] == 0.0 or weights[1] == 0.0   # (a quantum below the doubles: nothing to floor)
        if not subnormal_unit:   # (the arm: the counts the issue names)
            assert want.q[:5].tolist() == [1, 0, 1, 0, 2] and want.q[8] == 3, name
            assert got.energy[k, 0, 0] == 1.0 / float(want.W) and got.energy[k, 0, 2] == 2.0 / float(want.W), name
            assert got.radius[k, 0, 0] == 1.0
        assert 2 ** 57 <= int(want.q[5]) < 2 ** 58 and want.W < 2 ** 62, name   # (B = 4: 2^(61 - B) <= q_max < 2^(62 - B))
    assert ref.weight_shift(groups[-1][0]) < -900 and ref.weight_shift(groups[6][0]) > 1000
    assert np.all(np.isfinite(got.energy[[3, 5]]))   # (the neighbours of the group without weight)


def test_ceil_decides_where_the_threshold_is_no_integer():
    """phi (double) W is a double, and at or above 2^53 every double is an integer: ceil rounds nothing up unless phi W
    is small.  Rays of one, one and two quanta lie nearest (cumulative q of 1, 2 and 4): phi = 1.5 / W asks for 2 units
    and phi = 2.5 / W for 3, where a floor would ask for 1 and 2 -- both cumulative sums, so another ray would answer."""
    top = 0.75
    unit = np.ldexp(1.0, 0 - 62 + 3)   # (w_max = 0.75 2^0 and B = bit_length(5) = 3: one quantum)
    w = np.array([unit, 1.25 * unit, 2.75 * unit, top, top / 4])
    q, total = ref.integer_weights(w)
    assert q[:3].tolist() == [1, 1, 2]
    fractions = (1.5 / float(total), 2.5 / float(total), 4.0 / float(total))
    products = [phi * float(total) for phi in fractions]
    assert [int(np.floor(v)) for v in products[:2]] == [1, 2] and [int(np.ceil(v)) for v in products] == [2, 3, 4]   # (the arm)
    p = np.stack([[1.0, -2.0, 3.0, 4.0, -5.0], np.zeros(5)], 1)
    case = Case(ref.plane_frame(p, np.zeros_like(p), w), centre="none", shape="slit_e2", follow_centroid=False, **ORIGIN)
    got, (want,) = case.check([1.0, 2.0, 3.0], fractions)
    assert want.T == [2, 3, 4] and list(got.radius[0, 0]) == [2.0, 3.0, 3.0]


@pytest.mark.parametrize("count", (255, 256, 4095, 4096, 65_535, 65_536))
def test_the_largest_total_and_the_count_that_sets_the_shift(count):
    """``count`` rays of weight w_max = 0.999 and one of one and a half quanta at the smallest distance: it counts 1 with
    B = bit_length(count + 1) and would count 0 or 3 with another B.  Beside them rows that are left out (a NaN end
    point, a negative weight: they do not count towards B) and, in a second group, a zero-weight ray that does.  A third
    group holds ``count`` rays that all weigh w_max: the largest W the rule allows at that count."""
    top = 0.999
    m = count   # (rays used in group 0: count - 1 of w_max and the small one)
    unit = np.ldexp(1.0, 0 - 62 + int(m).bit_length())
    rng = np.random.default_rng(count)
    frames = []
    for g, extra in enumerate(("left out", "zero weight")):
        w = np.full(m, top)
        w[0] = 1.5 * unit
        d = np.concatenate([[0.5], 1.0 + rng.permutation(m - 1) / 2.0 ** 10])
        if extra == "zero weight":
            w, d = np.append(w, 0.0), np.append(d, 0.25)
        p = np.stack([d * rng.choice([-1.0, 1.0], len(d)), np.zeros(len(d))], 1)
        rows = ref.plane_frame(p, np.zeros_like(p), w, g * 100_000 + np.arange(len(d)))
        if extra == "left out":
            bad = ref.plane_frame(np.zeros((2, 2)), np.zeros((2, 2)), [top, -1.0], g * 100_000 + 90_000 + np.arange(2))
            bad[0, 10] = np.nan
            rows = np.concatenate([rows[:m // 2], bad, rows[m // 2:]])
        frames.append(rows)
    d = 1.0 + rng.permutation(m) / 2.0 ** 10
    p = np.stack([d * rng.choice([-1.0, 1.0], m), np.zeros(m)], 1)
    frames.append(ref.plane_frame(p, np.zeros_like(p), np.full(m, top), 200_000 + np.arange(m)))
    case = Case(np.concatenate(frames), centre="none", shape="slit_e2", follow_centroid=False, rays_per_source=100_000,
                n_groups=3, **ORIGIN)
    radii = np.concatenate([[0.25, 0.5], 1.0 + np.arange(0, m, max(1, m // 16)) / 2.0 ** 10])
    got, wants = case.check(radii, (5e-324, 0.5, 1.0))
    assert list(got.n_rays) == [m, m + 1, m] and list(got.n_missed) == [2, 0, 0]
    full, bits = int(np.floor(np.ldexp(top, 62 - int(m).bit_length()))), int(m).bit_length()
    assert wants[0].q[0] == 1 and wants[0].W == (m - 1) * full + 1 < 2 ** 62 and wants[0].W >= 2 ** 60
    assert got.radius[0, 0, 0] == 0.5 and got.energy[0, 0, 1] == 1.0 / float(wants[0].W)
    # all weights w_max: W = count q_max, within one q_max of the 2^62 the rule keeps it under at 2^k - 1 rays
    assert wants[2].W == m * full < 2 ** 62 and wants[2].W >= 2 ** 60 and np.all(wants[2].q == full)
    assert got.energy[2, 0, -1] == float(wants[2].bins[0].sum()) / float(wants[2].W) and got.radius[2, 0, 2] == d.max()
    # the zero-weight ray is a ray used: at 2^k - 1 it moves B, and the small ray then counts 0
    other = int(m + 1).bit_length()
    assert wants[1].q[0] == (0 if other > bits else 1) and (other > bits) == (count in (255, 4095, 65_535))
    assert got.radius[1, 0, 0] == (1.0 if other > bits else 0.5)


# ---- the curve's plane tiles ----------------------------------------------------------------------------------------------------
CURVE = ((4095, 1, [1]), (4095, 2, [1, 1]), (4095, 3, [1, 1, 1]), (4096, 1, [1]), (4096, 2, [1, 1]), (4096, 3, [1, 1, 1]),
         (2048, 3, [2, 1]), (2049, 2, [1, 1]), (1365, 4, [3, 1]), (1366, 4, [2, 2]), (16, 256, [256]),
         (17, 256, [240, 16]), (1, 256, [256]))


@pytest.mark.parametrize("n_radii,n_focus,tiles", CURVE)
def test_every_bin_of_the_curve_tiles(n_radii, n_focus, tiles):
    """Half-widths on the 2^-10 grid (on the 2^-2 grid from 17 radii down) under 700 + 500 rays on the 2^-8 grid with
    slopes of at most 2^-7: at quarter shifts, and at 256 integer shifts, the rays stay on those grids and many lie on a
    radius exactly.  Every bin of every plane is compared."""
    assert ref.plane_tiles(n_focus, n_radii) == tiles and all(k * n_radii <= ref.ENERGY_WINDOW for k in tiles)
    p, s, w = ref.dyadic_rays(1200, 71)
    s = np.random.default_rng(72).integers(-2, 3, (1200, 2)) / ref.GRID
    ids = np.concatenate([np.arange(700), 1000 + np.arange(500)])
    focus = tuple(np.arange(n_focus) - n_focus // 2.0) if n_focus > 4 else (0.25, -0.5, 0.0, 1.0)[:n_focus]
    case = Case(ref.plane_frame(p, s, w, ids), shape="square", follow_centroid=False, focus=focus, rays_per_source=1000,
                n_groups=2, **ORIGIN)
    step = 4.0 / n_radii if n_radii > 17 else 0.25
    radii = np.round(np.arange(1, n_radii + 1) * step * 1024) / 1024 if n_radii > 1 else np.array([2.0])
    radii = np.unique(radii)
    if len(radii) < n_radii:   # (4095 steps of 4 / 4095 collide on the grid: take the grid itself)
        radii = np.arange(1, n_radii + 1) / 1024
    assert len(radii) == n_radii
    got, wants = case.check(radii, None)
    for want in wants:
        assert want.on.sum() >= 16 and np.count_nonzero(want.bins) >= min(n_radii, 300)   # (rays on radii; bins in use)
        assert np.all(want.bins.any(axis=1))   # (every plane of every tile, the ragged one too, holds weight)


# ---- the fraction tiles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fractions", (1, 4, 5, 8, 9, 16))
def test_the_fraction_tiles(n_fractions):
    want_tiles = {1: [(0, 1)], 4: [(0, 4)], 5: [(0, 4), (4, 1)], 8: [(0, 4), (4, 4)], 9: [(0, 4), (4, 4), (8, 1)],
                  16: [(0, 4), (4, 4), (8, 4), (12, 4)]}
    assert ref.fraction_tiles(n_fractions) == want_tiles[n_fractions]
    p, s, w = ref.dyadic_rays(1500, 81)
    ids = np.concatenate([np.arange(600), 1000 + np.arange(500), 2000 + np.arange(400)])
    case = Case(ref.plane_frame(p, s, w, ids), shape="circle", follow_centroid=True, focus=(-0.25, 0.0, 0.5),
                rays_per_source=1000, n_groups=3, **ORIGIN)
    fractions = tuple((np.arange(n_fractions) + 0.5) / n_fractions)   # (distinct: a swapped window shows)
    got, wants = case.check(None, fractions)
    for g in range(3):
        for f in range(3):
            assert len(np.unique(got.radius[g, f])) == n_fractions, (g, f)


# ---- the digit levels of the select -------------------------------------------------------------------------------------------------
def slit_case(values, focus=(0.0,), s=None):
    p = np.stack([values, np.zeros(len(values))], 1)
    s = np.zeros_like(p) if s is None else s
    return Case(ref.plane_frame(p, s, np.ones(len(p))), centre="none", shape="slit_e2", follow_centroid=False, focus=focus,
                **ORIGIN)


@pytest.mark.parametrize("bit", (0, 9, 10, 19, 20, 29, 30, 40, 41, 51, 52, 62))
def test_keys_that_differ_in_one_bit(bit):
    """Six rays at two distances whose bit images differ in bit ``bit`` alone: phi = 1/2 asks for the lower one by
    equality (T = 3 W / 6), the next double above 1/2 for the upper."""
    base = 0x3FF0000000000000 if bit < 52 else 0x0010000000000000 if bit == 62 else 0x3FE0000000000000
    base &= ~(1 << bit)
    low, high = ref.from_bits([base])[0], ref.from_bits([base | (1 << bit)])[0]
    assert np.isfinite(high) and low < high and int(ref.bits([high])[0] ^ ref.bits([low])[0]) == 1 << bit
    case = slit_case(np.array([high, -low, low, -high, high, low]))
    fractions = (0.5, np.nextafter(0.5, 1.0), 1 / 6, 1.0)
    got, (want,) = case.check([low, high], fractions)
    assert list(got.radius[0, 0]) == [low, high, low, high] and list(got.energy[0, 0]) == [0.5, 1.0]
    for need in want.T:   # (the arm: the pass that holds the bit chooses, and no other does)
        path = ref.digit_path(want.keys[0].tolist(), want.q.tolist(), need)
        assert ref.deciding_passes(path) == [ref.pass_of_bit(bit)], (bit, path)


def test_adjacent_doubles_subnormals_and_infinity():
    fractions = SIXTEENTHS[1::2] + SIXTEENTHS[:1] + (np.nextafter(0.5, 1.0), 5e-324)   # (eighths first)
    # 2048 adjacent doubles from 1: the keys share 42 bits and more, the last two passes choose
    k = np.random.default_rng(91).permutation(2048)
    case = slit_case((1.0 + k * 2.0 ** -52) * np.where(k % 2, -1.0, 1.0))
    got, (want,) = case.check(1.0 + np.array([0, 1, 1023, 1024, 2046, 2047]) * 2.0 ** -52, fractions)
    assert list(got.radius[0, 0, :8]) == [1.0 + (256 * j - 1) * 2.0 ** -52 for j in range(1, 9)]
    assert list(got.radius[0, 0, 8:]) == [1.0 + 127 * 2.0 ** -52, 1.0 + 1024 * 2.0 ** -52, 1.0]
    paths = [ref.digit_path(want.keys[0].tolist(), want.q.tolist(), need) for need in want.T]
    assert all(ref.deciding_passes(path) == [4, 5] for path in paths)
    # subnormal distances k 5e-324, k = 1 .. 3000: the first four digits are zero
    k = np.random.default_rng(92).permutation(3000) + 1
    case = slit_case(k * 5e-324 * np.where(k % 2, -1.0, 1.0))
    got, (want,) = case.check(np.array([1, 2, 1024, 1025, 3000]) * 5e-324, fractions)
    assert got.radius[0, 0, 7] == 3000 * 5e-324 and got.radius[0, 0, 3] == 1500 * 5e-324 and got.radius[0, 0, -1] == 5e-324
    paths = [ref.digit_path(want.keys[0].tolist(), want.q.tolist(), need) for need in want.T]
    assert all(ref.deciding_passes(path) == [4, 5] for path in paths) and int(want.keys.max()) == 3000
    # +inf among finite ones: at the far plane two rays overflow
    values = np.array([1.0, -2.0, 3.0, 0.5, -0.25, 4.0])
    s = np.zeros((6, 2))
    s[[1, 4], 0] = 1e200
    case = slit_case(values, focus=(0.0, 1e200), s=s)
    got, (want,) = case.check([0.5, 4.0, 1e308], (0.5, 4 / 6, 5 / 6, 1.0))
    assert (want.keys[1] == ref.INF_BITS).sum() == 2 and np.all(np.isfinite(got.radius[0, 0]))
    assert list(got.radius[0, 1]) == [3.0, 4.0, np.inf, np.inf] and got.energy[0, 1, 2] == 4 / 6


# ---- slices and chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", (False, True))
def test_group_sizes_at_the_slice_and_chunk_edges(follow):
    """Rays used per group of 2047, 2048, 2049, 4095, 4096, 4097 and 8193 and a group without rays, every group with
    rows that are left out, rows of another surface among them."""
    sizes = (2047, 2048, 2049, 0, 4095, 4096, 4097, 8193)
    assert [ref.slices(n) for n in sizes] == [1, 1, 2, 1, 2, 2, 3, 5]
    assert [ref.chunks(n) for n in sizes] == [1, 1, 1, 0, 1, 1, 2, 3]
    per = 10_000
    p, s, w = ref.dyadic_rays(sum(sizes), 101)
    ids = np.concatenate([g * per + np.arange(n) for g, n in enumerate(sizes)])
    rows = ref.plane_frame(p, s, w, ids)
    bad = ref.plane_frame(np.zeros((14, 2)), np.zeros((14, 2)), np.tile([1.0, -1.0], 7),
                          np.repeat([g * per + 9000 for g in range(8) if sizes[g]], 2) + np.tile([0, 1], 7))
    bad[::2, 11] = np.nan
    other = ref.plane_frame(*ref.dyadic_rays(3000, 102), ids=np.arange(3000) * 20, surface=6.0)
    frame = np.concatenate([rows, bad, other])
    frame = frame[np.random.default_rng(103).permutation(len(frame))]
    case = Case(frame, shape="circle", follow_centroid=follow, focus=(0.0, -0.75), rays_per_source=per, n_groups=len(sizes),
                **ORIGIN)
    got, wants = case.check(case.radii_on_rays(40, zero=True), (0.05, 0.5, 0.8, 0.9, 1.0))
    assert list(got.n_rays) == list(sizes) and list(got.n_missed) == [2, 2, 2, 0, 2, 2, 2, 2]
    assert all((want.on > 0).sum() >= 3 for want in wants if want.W)


@pytest.mark.parametrize("count", (524_288, 524_289))
def test_both_sides_of_the_cap_of_256_slices(count):
    assert ref.slices(count) == 256 and ref.slice_rays(count) == (2048 if count == 524_288 else 2049)
    assert ref.slices(count - 2048) == (255 if count == 524_288 else 256)   # (the cap itself: the first count to meet it)
    p, s, w = ref.dyadic_rays(count, 111, unit_weights=True)
    case = Case(ref.plane_frame(p, s, w), shape="square", follow_centroid=True, focus=(0.5,), **ORIGIN)
    got, (want,) = case.check(case.radii_on_rays(3), (0.25, 0.5, 0.9, 1.0))
    assert got.n_rays[0] == count and (want.on > 0).sum() >= 3 and want.W == count * (want.W // count)


def test_300_groups_with_empty_ones_and_rows_of_another_surface():
    """300 groups of 0 to 45 rays: more groups than one workgroup of k_energy_record holds, a group change every few
    rows of a chunk, groups without rays, rows of another surface between them."""
    n_groups, per = 300, 64
    sizes = [0 if g % 7 == 3 else 1 + (g * 37) % 45 for g in range(n_groups)]
    assert n_groups > ref.BLOCK and sizes.count(0) == 43 and sum(sizes) < 2 * ref.MTF_CHUNK
    p, s, w = ref.dyadic_rays(sum(sizes), 121)
    ids = np.concatenate([g * per + np.arange(n) for g, n in enumerate(sizes)])
    other = ref.plane_frame(*ref.dyadic_rays(2000, 122), ids=np.arange(2000) * 9, surface=6.0)
    frame = np.concatenate([ref.plane_frame(p, s, w, ids), other])
    frame = frame[np.random.default_rng(123).permutation(len(frame))]
    case = Case(frame, shape="circle", follow_centroid=True, focus=(0.0, 0.25), rays_per_source=per, n_groups=n_groups,
                **ORIGIN)
    got, wants = case.check(case.radii_on_rays(2), (0.5, 0.9, 1.0))
    assert list(got.n_rays) == sizes and np.all(np.isnan(got.radius[3::7])) and np.all(np.isfinite(got.radius[0::7]))


# ---- the cap of the digit windows -----------------------------------------------------------------------------------------------------
def test_exactly_16384_digit_windows():
    n_groups, n_focus, n_fractions = 64, 16, 16
    assert ref.digit_windows(n_groups, n_focus, n_fractions) == 16_384 and ref.within_caps(n_groups, n_focus, 0, n_fractions)
    assert not ref.within_caps(n_groups + 1, n_focus, 0, n_fractions)   # (refused: tests/test_host_energy_sums.py)
    per = 64
    sizes = [20 + (g * 13) % 40 for g in range(n_groups)]
    p, s, w = ref.dyadic_rays(sum(sizes), 131)
    ids = np.concatenate([g * per + np.arange(n) for g, n in enumerate(sizes)])
    case = Case(ref.plane_frame(p, s, w, ids), shape="square", follow_centroid=True, focus=tuple(np.arange(16) / 8.0 - 1.0),
                rays_per_source=per, n_groups=n_groups, **ORIGIN)
    got, wants = case.check(None, SIXTEENTHS)
    assert np.all(np.isfinite(got.radius)) and got.radius.shape == (64, 16, 16)


# ---- frames on no grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
@pytest.mark.parametrize("reference", ("centroid", "given"))
def test_frames_on_no_grid_from_the_devices_own_centre(reference, shape):
    """The synthetic frame of the MTF's tests (a tilted axis, two groups, rows left out) and a random plane frame of
    9000 rays: C_g, pbar and sbar are read from the record (and held to their bound), the radii are placed on rays and
    one ulp beside them, and every energy and radius is then equal bit for bit."""
    frame, axis = helpers.mtf_synthetic_frame()
    given = np.array([[0.01, -0.02, 0.03], [0.012, -0.021, 0.029]])
    options = dict(axis=axis, rays_per_source=6000, n_groups=2, shape=shape, focus=(-0.05, 0.0, 0.02),
                   reference="centroid" if reference == "centroid" else given)
    case = Case(frame, surface=5.0, centre="given", **options)
    got, wants = case.check(case.radii_on_rays(40), (0.05, 0.5, 0.8, 0.95, 1.0))
    assert np.all(got.n_rays > 1000) and got.n_missed.sum() == 5 and all((want.on > 0).sum() >= 20 for want in wants)
    rng = np.random.default_rng(141)
    n = 9000
    frame = ref.plane_frame(rng.normal(0, 0.01, (n, 2)), rng.normal(0, 0.05, (n, 2)), 0.5 + rng.random(n))
    frame[:, 9] = rng.normal(0, 1e-3, n)   # (end points off the plane: the staging's own arithmetic takes part)
    options = dict(shape=shape, focus=(-0.1, 0.0, 0.2), reference="centroid" if reference == "centroid" else given[0])
    case = Case(frame, centre="given", **options)
    got, wants = case.check(case.radii_on_rays(40), (0.05, 0.5, 0.8, 0.95, 1.0))
    assert ref.chunks(n) == 3 and (wants[0].on > 0).sum() >= 20
    # and measured from C_g itself
    case = Case(frame, centre="given", **dict(options, follow_centroid=False))
    case.check(case.radii_on_rays(40), (0.05, 0.5, 0.8, 0.95, 1.0))
    print_ratios()
    assert max(RATIOS.values()) > 0   # (the bound was exercised: the sums do round on these frames)
