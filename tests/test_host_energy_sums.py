"""The integer restatement of the enclosed energy (tests/energy_sums_reference.py) on the CPU: its constants and rules
against the headers' text, its partition rules against hand-counted values at every edge the GPU module visits, the
integers against tests/energy_reference.py where that one is valid and against a brute-force loop in Python ints and
fractions (ties and +inf included), the digit path against the sorted selection, and the refusals of the exact form."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import energy_reference as old
import energy_sums_reference as ref


# ---- the constants and the restated lines -------------------------------------------------------------------------------
def test_constants_and_rules_are_the_headers():
    found = ref.sums.header_constants(ref.HOST_RULES)
    for key, name in ref.HEADER_NAMES.items():
        assert found[key] == getattr(ref, name), (key, found[key], getattr(ref, name))
    for name, lines in ref.HOST_RULES.items():
        text = open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", name)).read()
        for line in lines:
            assert line in text, (name, line)
    assert sum(ref.ENERGY_WIDTH) == 63 and len(ref.ENERGY_WIDTH) == ref.ENERGY_PASSES
    assert all(low == sum(ref.ENERGY_WIDTH[k + 1:]) for k, low in enumerate(ref.ENERGY_LOW))
    assert max(ref.ENERGY_WIDTH) == 11 and 1 << 11 == ref.ENERGY_DIGITS
    device = open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", "prt_device.hpp")).read()
    assert "#define PRT_BLOCK 256" in device and ref.BLOCK == 256
    makefile = open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract=off" in makefile   # (what lets numpy's separate operations stand for the kernel's)


def test_partition_rules_at_hand_counted_edges():
    # slices: 2048 rays a slice at least, 256 slices at most; per = ceil(count / slices)
    want = {0: (1, 0), 1: (1, 1), 2047: (1, 2047), 2048: (1, 2048), 2049: (2, 1025), 4095: (2, 2048), 4096: (2, 2048),
            4097: (3, 1366), 6145: (4, 1537), 8193: (5, 1639), 524_288: (256, 2048), 524_289: (256, 2049),
            1_000_000: (256, 3907)}
    for count, (n, per) in want.items():
        assert (ref.slices(count), ref.slice_rays(count)) == (n, per), count
        bounds = ref.slice_bounds(count)
        assert sum(max(hi - lo, 0) for lo, hi in bounds) == count and len(bounds) == n
        assert all(b[0] == a[0] + per for a, b in zip(bounds, bounds[1:]))
    assert ref.slice_bounds(4097) == [(0, 1366), (1366, 2732), (2732, 4097)]
    assert ref.slice_bounds(524_289)[-1] == (255 * 2049, 524_289) and 524_289 - 255 * 2049 == 1794
    # chunks of 4096 and the depth of the centroid sums
    assert [ref.chunks(n) for n in (0, 1, 4095, 4096, 4097, 8193, 524_289)] == [0, 1, 1, 1, 2, 3, 129]
    assert ref.centre_depth(4096) == 16 + 8 + 1 and ref.centre_depth(8193) == 16 + 8 + 3
    # the curve's window of 4096 (plane, radius) tallies
    tiles = {(1, 4095): [1], (2, 4095): [1, 1], (3, 4096): [1, 1, 1], (3, 2048): [2, 1], (2, 2049): [1, 1],
             (4, 1365): [3, 1], (4, 1366): [2, 2], (256, 16): [256], (256, 17): [240, 16], (256, 1): [256],
             (41, 130): [31, 10], (5, 0): [1] * 5}
    for (n_focus, n_radii), planes in tiles.items():
        assert ref.plane_tiles(n_focus, n_radii) == planes, (n_focus, n_radii)
        assert all(k * max(n_radii, 1) <= ref.ENERGY_WINDOW for k in planes)
    assert ref.planes_per_tile(256, 16) * 16 == ref.ENERGY_WINDOW   # (one full window)
    # fraction tiles of 4
    assert ref.fraction_tiles(1) == [(0, 1)] and ref.fraction_tiles(4) == [(0, 4)]
    assert ref.fraction_tiles(5) == [(0, 4), (4, 1)] and ref.fraction_tiles(8) == [(0, 4), (4, 4)]
    assert ref.fraction_tiles(9) == [(0, 4), (4, 4), (8, 1)] and ref.fraction_tiles(16) == [(k, 4) for k in (0, 4, 8, 12)]
    # the caps: 256 MiB of bins, 256 MiB of 16 KiB digit windows = 16 384 of them
    assert ref.digit_windows(64, 16, 16) == 16_384 == ref.ENERGY_SLAB_BYTES // (ref.ENERGY_DIGITS * 8)
    assert ref.within_caps(64, 16, 0, 16) and not ref.within_caps(65, 16, 0, 16)
    assert not ref.within_caps(64, 17, 0, 16)
    assert ref.within_caps(32, 256, 4096, 0) and not ref.within_caps(33, 256, 4096, 0)
    # the digit that holds a bit of the key
    assert [ref.pass_of_bit(b) for b in (0, 9, 10, 19, 20, 29, 30, 40, 41, 51, 52, 62)] == [5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]


def test_the_library_refuses_one_digit_window_past_the_cap():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_energy_workspace_bytes(1000, 64, 0, 16, 16) > 0
    assert lib.prt_frame_energy_workspace_bytes(1000, 65, 0, 16, 16) == -1
    assert lib.prt_frame_energy_workspace_bytes(1000, 64, 0, 16, 17) == -1
    buf = np.zeros(65 * 10)
    p = buf.ctypes.data
    phi, planes = np.linspace(0.05, 0.8, 16), np.zeros(17)
    for n_groups, n_focus in ((65, 16), (64, 17)):
        assert not ref.within_caps(n_groups, n_focus, 0, 16)
        rc = lib.prt_frame_energy(0, p, 4, 4, 1.0, float("nan"), 1.0, n_groups, None, ref.DEFAULT_AXES.ctypes.data, 1, 0,
                                  1, None, 0, phi.ctypes.data, 16, planes.ctypes.data, n_focus, None, p, p, p, None)
        assert rc == -1 and "16 KiB above the 256 MiB slab cap" in lib.prt_last_error().decode()


# ---- the integer weights ------------------------------------------------------------------------------------------------
def test_integer_weights_floor_quantum_and_the_power_of_two_edges():
    # w_max, one quantum, half a quantum, one and a half, zero: B = bit_length(5) = 3, the quantum is w_max 2^-(61 - B)
    top = 0.75
    unit = top * 2.0 ** -(61 - 3) / 0.75 * 0.5   # (w_max = 0.75 2^0: 2^(E - 1) 2^-(61 - B) = 2^-59)
    assert unit == 2.0 ** -59
    q, total = ref.integer_weights([top, unit, unit / 2, 1.5 * unit, 0.0])
    assert q.tolist() == [3 * 2 ** 57, 1, 0, 1, 0] and total == 3 * 2 ** 57 + 2
    # w_max on a power of two, and just below it: frexp(2^k) = 0.5 2^(k + 1)
    for k in (-3, 0, 7):
        q, _ = ref.integer_weights([2.0 ** k, 2.0 ** k])
        assert q.tolist() == [2 ** 59, 2 ** 59]   # (B = 2: q_max = 2^(61 - B))
        q, _ = ref.integer_weights([np.nextafter(2.0 ** k, 0.0), 2.0 ** (k - 1)])
        assert q.tolist() == [2 ** 60 - 2 ** 7, 2 ** 59]
    # subnormal and huge weights: the shift is far outside +-1023 and still a power of two
    q, _ = ref.integer_weights([5e-324, 0.0, 5e-324])
    assert q.tolist() == [2 ** 59, 0, 2 ** 59] and ref.weight_shift([5e-324, 0.0, 5e-324]) == 62 + 1073 - 2
    q, _ = ref.integer_weights([1e308, 0.5e308, 1.0])
    assert ref.weight_shift([1e308, 1.0, 1.0]) < -900 and q[0] == 2 * q[1] and q[2] == 0
    # the largest W the rule allows: 2^k - 1 and 2^k rays of weight w_max
    for m in (255, 256, 4095, 4096, 65_535, 65_536):
        q, total = ref.integer_weights(np.full(m, 0.999))
        bits = m.bit_length()
        assert int(q[0]) >> (61 - bits) == 1 and total == m * int(q[0]) < 2 ** 62
        assert total >= 2 ** 61 * m // 2 ** bits
    assert ref.integer_weights([])[1] == 0 and ref.integer_weights(np.zeros(3))[0].tolist() == [0, 0, 0]
    # the same integers as the float restatement's
    rng = np.random.default_rng(3)
    for n in (1, 64, 4097):
        w = 50 + 50 * rng.random(n)
        assert np.array_equal(ref.integer_weights(w)[0], old.integer_weights(w))


# ---- against the float restatement where it is valid ----------------------------------------------------------------------
def test_against_the_float_restatement_where_its_margin_is_positive():
    rng = np.random.default_rng(17)
    n = 3000
    p, s, w = rng.normal(0, 0.01, (n, 2)), rng.normal(0, 0.05, (n, 2)), 0.5 + rng.random(n)
    focus, fractions = (-0.1, 0.0, 0.2), (0.05, 0.3, 0.5, 0.8, 0.9, 1.0)
    for shape in ref.SHAPES:
        for follow in (False, True):
            mean = None
            if follow:   # (the float restatement's own centre, passed as the given form)
                mean = np.concatenate([(w @ p) / w.sum(), (w @ s) / w.sum()])
            found = np.concatenate([old.distances(p, s, d, old.plane_centre(p, s, w, d, follow), shape) for d in focus])
            radii = old.clear_radii(found, 9)
            energy, radius, margin = old.enclosed(p, s, w, radii, fractions, focus, shape, follow)
            assert margin > 0
            got = ref.enclosed(p, s, w, radii, fractions, focus, shape, follow, mean=mean)
            assert np.array_equal(got.energy, energy) and np.array_equal(got.radius, radius), (shape, follow)
            assert got.on.sum() == 0 and int(got.bins.sum(1)[0]) <= got.W


# ---- against a brute-force loop ---------------------------------------------------------------------------------------------
def brute_force(p, s, w, radii, fractions, focus, shape, mean):
    """The definitions with loops over rays, Python ints and fractions; d itself is the fp64 value (an input here)."""
    n = len(w)
    positive = [Fraction(v) for v in w if v > 0]
    energy = [[math.nan] * len(radii) for _ in focus]
    radius = [[math.nan] * len(fractions) for _ in focus]
    if not positive:
        return energy, radius, 0
    top = max(positive)
    e = 0
    while top >= Fraction(2) ** e:
        e += 1
    while top < Fraction(2) ** (e - 1):
        e -= 1   # (top = f 2^e with 0.5 <= f < 1)
    scale = Fraction(2) ** (62 - e - n.bit_length())
    q = [int(Fraction(v) * scale // 1) for v in w]
    total = sum(q)
    for f, delta in enumerate(focus):
        d = ref.distances(p, s, delta, ref.plane_centre(mean, delta, mean is not None), shape).tolist()
        exact = [None if math.isinf(v) else Fraction(v) for v in d]   # (None: +inf, beyond every radius, last)
        for j, edge in enumerate(radii):
            inside = sum(q[r] for r in range(n) if exact[r] is not None and exact[r] <= Fraction(edge))
            energy[f][j] = float(inside) / float(total)
        for k, phi in enumerate(fractions):
            need = min(max(math.ceil(Fraction(float(phi) * float(total))), 1), total)
            best = None
            for r in range(n):   # the smallest own distance whose cumulative weight reaches the threshold
                if exact[r] is None:
                    reach = total
                else:
                    reach = sum(q[t] for t in range(n) if exact[t] is not None and exact[t] <= exact[r])
                if reach >= need and (best is None or (exact[r] is not None and (exact[best] is None or exact[r] < exact[best]))):
                    best = r
            radius[f][k] = d[best]
    return energy, radius, total


def test_against_brute_force_with_ties_and_infinity():
    rng = np.random.default_rng(23)
    cases = []
    p, s, w = ref.dyadic_rays(40, 5)
    cases.append((p, s, w, (-0.5, 0.0, 0.25)))
    p, s, w = ref.dyadic_rays(33, 6, unit_weights=True, reach=1)
    p[10:25] = p[10]   # (a tie of fifteen rays)
    s[10:25] = s[10]
    cases.append((p, s, w, (0.0, 2.0)))
    p = rng.normal(0, 1, (17, 2))
    s = np.zeros((17, 2))
    s[3] = [1e200, 0.0]   # (+inf at the far plane for the circle)
    cases.append((p, s, 0.25 + rng.random(17), (0.0, 1e200)))
    cases.append((np.zeros((5, 2)), np.zeros((5, 2)), np.zeros(5), (0.0,)))   # (no weight: NaN)
    for p, s, w, focus in cases:
        for shape in ref.SHAPES:
            for follow in (False, True):
                mean = None
                if follow and w.sum() > 0:
                    mean = np.concatenate([(w @ p) / w.sum(), (w @ s) / w.sum()])
                every = np.concatenate([ref.distances(p, s, d, ref.plane_centre(mean, d, mean is not None), shape)
                                        for d in focus])
                finite = np.unique(every[np.isfinite(every)])
                picks = finite[:: max(1, len(finite) // 5)]
                radii = np.unique(np.concatenate([picks, np.nextafter(picks, np.inf), np.nextafter(picks[picks > 0], 0.0),
                                                  [0.0, 1e308]]))
                fractions = [k / 8 for k in range(1, 9)] + [1e-30, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)]
                got = ref.enclosed(p, s, w, radii, fractions, focus, shape, mean is not None, mean=mean)
                energy, radius, total = brute_force(p, s, w, radii, fractions, focus, shape, mean)
                assert got.W == total
                assert np.array_equal(ref.bits(got.energy), ref.bits(energy)), (shape, follow)
                assert np.array_equal(ref.bits(got.radius), ref.bits(radius)), (shape, follow)
                if total:
                    assert got.on.sum() > 0   # (radii do lie on rays)


def test_rays_on_radii_and_thresholds_on_cumulative_sums_are_counted():
    """4800 rays of weight 1 on the grid at shift 0.25, radii on rays, phi = k / 16: W is exact in a double, every T_k
    is a cumulative sum, and energies and radii are the counted ones for all four shapes."""
    n = 4800
    p, s, w = ref.dyadic_rays(n, 41, unit_weights=True)
    delta = 0.25
    fractions = [k / 16 for k in range(1, 17)]
    for shape in ref.SHAPES:
        d = np.sort(ref.distances(p, s, delta, np.zeros(2), shape))
        radii = np.unique(d[:: n // 16])
        got = ref.enclosed(p, s, w, radii, fractions, (delta,), shape, follow_centroid=False)
        unit = got.W // n
        assert got.W == n * unit and float(got.W) == got.W and got.T == [k * n // 16 * unit for k in range(1, 17)]
        assert np.array_equal(got.energy[0], np.searchsorted(d, radii, side="right") / n)
        assert np.array_equal(got.radius[0], d[[k * n // 16 - 1 for k in range(1, 17)]])
        assert np.all(got.on[0] >= 1)
        # and with the plane's own centre, from integers
        got = ref.enclosed(p, s, w, radii, fractions, (delta,), shape, follow_centroid=True)
        centre = got.mean[:2] + delta * got.mean[2:]
        d = np.sort(ref.distances(p, s, delta, centre, shape))
        assert np.array_equal(got.radius[0], d[[k * n // 16 - 1 for k in range(1, 17)]])


# ---- the digit path ---------------------------------------------------------------------------------------------------------
def test_the_digit_path_reassembles_to_the_radius():
    p, s, w = ref.dyadic_rays(500, 8)
    p[100:300] = p[100]
    s[100:300] = s[100]
    fractions = [0.01, 0.2, 0.5, np.nextafter(0.5, 1.0), 0.9, 1.0]
    for shape in ref.SHAPES:
        got = ref.enclosed(p, s, w, (), fractions, (0.0, 0.5), shape, follow_centroid=False)
        for f in range(2):
            for k, need in enumerate(got.T):
                path = ref.digit_path(got.keys[f].tolist(), got.q.tolist(), need)
                assert path[-1][0] == int(ref.bits(got.radius[f])[k]), (shape, f, k)
                assert all(path[j][0] == path[-1][0] >> ref.ENERGY_LOW[j] for j in range(6))
                assert 1 <= path[-1][1] and all(a[1] >= b[1] for a, b in zip(path, path[1:]))
    # keys that differ in one bit: the pass that holds the bit is the only one that chooses
    for bit in (0, 9, 10, 19, 20, 29, 30, 40, 41, 51, 52, 62):
        low = 0x3FF0000000000000 if bit < 52 else 0x0010000000000000 if bit == 62 else 0x3FE0000000000000
        low &= ~(1 << bit)
        keys = [low, low | (1 << bit)] * 3
        for need, want in ((3, low), (4, low | (1 << bit))):
            path = ref.digit_path(keys, [1] * 6, need)
            assert path[-1][0] == want and ref.deciding_passes(path) == [ref.pass_of_bit(bit)]
    # +inf among finite ones is a key like any other, the largest
    keys = [int(k) for k in ref.bits([1.0, np.inf, 2.0])]
    assert ref.digit_path(keys, [1, 1, 1], 3)[-1][0] == ref.INF_BITS


# ---- the centre of a plane --------------------------------------------------------------------------------------------------
def test_the_exact_centre_and_its_refusals():
    p, s, w = ref.dyadic_rays(5000, 9)
    centre = ref.exact_centre(p, s, w)
    wide = ref.centre_bound(p, s, w)
    assert centre.sum_w == w.sum() and np.all(np.abs(centre.mean - wide.mean.astype(float)) <= wide.mean_bound)
    # one correctly rounded division: the same in any order of the rays
    order = np.random.default_rng(1).permutation(len(w))
    assert np.array_equal(ref.exact_centre(p[order], s[order], w[order]).mean, centre.mean)
    assert np.array_equal(centre.mean, [math.fsum(w * p[:, 0]) / w.sum(), math.fsum(w * p[:, 1]) / w.sum(),
                                        math.fsum(w * s[:, 0]) / w.sum(), math.fsum(w * s[:, 1]) / w.sum()])
    with pytest.raises(ValueError, match="p: not a multiple"):
        ref.exact_centre(p + 2.0 ** -9, s, w)
    with pytest.raises(ValueError, match="w: not a multiple"):
        ref.exact_centre(p, s, w + 1 / 16)
    with pytest.raises(ValueError):
        ref.exact_centre(p * 2.0 ** 30, s, w)   # (beyond 2^30 grid units a value)
    big = np.full((2 ** 19, 2), 2.0 ** 21 - 1)
    with pytest.raises(ref.NotExact):
        ref.exact_centre(big, np.zeros_like(big), np.full(len(big), 7.875))   # (sum |w p| >= 2^53 units of 2^-11)
    # the bound grows with the depth and is of the order of u
    small = ref.centre_bound(p[:100], s[:100], w[:100])
    assert small.depth == 25 and wide.depth == 26 and 0 < small.sum_w_bound < 30 * ref.U * float(small.sum_w)


def test_staging_restates_the_plane_frame_exactly():
    p, s, w = ref.dyadic_rays(300, 12)
    frame = ref.plane_frame(p, s, w)
    frame[5, 10] = np.nan
    frame[6, 1] = -1.0
    (gp, gs, gw, used, missed), = ref.stage(frame, 4.0, np.zeros((1, 3)))
    keep = np.ones(300, dtype=bool)
    keep[5:7] = False
    assert used == 298 and missed == 2
    assert np.array_equal(gp, p[keep]) and np.array_equal(gs, s[keep]) and np.array_equal(gw, w[keep])
    # the same rays kept, the same s and w as the float restatement's staging on a general frame (p: another order)
    rng = np.random.default_rng(2)
    general = ref.plane_frame(rng.normal(0, 1, (50, 2)), rng.normal(0, 0.1, (50, 2)), rng.random(50))
    general[:, 9] = rng.normal(0, 1e-3, 50)
    theirs = old.stage(general, 4.0, reference=np.array([[0.1, -0.2, 0.3]]))[0]
    ours = ref.stage(general, 4.0, np.array([[0.1, -0.2, 0.3]]))[0]
    assert np.array_equal(ours[1], theirs[1]) and np.array_equal(ours[2], theirs[2]) and ours[0].shape == theirs[0].shape


def test_pythagorean_points_have_exact_roots():
    p, root = ref.pythagorean_rays(400, 4)
    d = ref.distances(p, np.zeros_like(p), 0.0, np.zeros(2), "circle")
    assert np.array_equal(d, root) and len(np.unique(root)) > 50
