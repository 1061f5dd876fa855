"""prt_frame_reduce, prt_frame_mean_square and prt_frame_stats at the edges of their partition, against
tests/frame_sums_reference.py: on dyadic frames, whose sums are exact in any order, bit for bit against numpy integers
(no tolerance); on random frames every statistic within the bound derived there.

The edges: one row to several waves of kFrameRowsPerWave; both sides of the switch to the slot path (64 copies of the
output, k_frame_fold) for one, two and three groups; group changes inside a slice, at a wave boundary, 64 groups in a
slice, revisited groups, ids outside the groups, empty groups; every filter; an offset view with ld > n_rows and a
frame that has to be made contiguous.  The other arm of the slot switch, n_groups > kFrameSlotGroups = 2048 with 256
waves a group, needs more than 5 * 10^8 rows (60 GB of frame) and is not reached here."""
import numpy as np
import pytest

import frame_sums_reference as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX
WAVE = ref.FRAME_ROWS_PER_WAVE  # prt_frame.hpp: kFrameRowsPerWave
FILTERS = ((None, None), (3.0, None), (None, 1.0), (4.0, 2.0))
_CACHE = {}
RATIOS = {}


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)).to("cuda:0"))


def labelled(frame, seed, generations=3):
    """Surfaces 3 / 4 at random -- but surface 9 over a stretch of more than two waves, where the filters select nothing
    --, generations in equal blocks, ids ascending from 0 inside each."""
    rng = np.random.default_rng(seed)
    n = len(frame)
    frame[:, IX["surface"]] = rng.choice([3.0, 4.0], n)
    if n > 8 * WAVE:
        frame[3 * WAVE - 5:5 * WAVE + 70, IX["surface"]] = 9.0
    block = -(-n // generations)
    frame[:, IX["generation"]] = np.arange(n) // block
    frame[:, IX["id"]] = np.arange(n) % block
    return frame, block


def big_dyadic(n_rows, n_groups):
    key = ("dyadic", n_rows)
    if key not in _CACHE:
        frame, block = labelled(ref.dyadic_frame(n_rows, n_rows % 1000), n_rows % 999)
        _CACHE[key] = (frame, device_frame(frame), block)
    frame, device, block = _CACHE[key]
    return frame, device, -(-block // n_groups)


def check_exact(frame, device, rays_per_source, n_groups, filters=FILTERS, pivot_seeds=(None, 5)):
    for k, (surface, generation) in enumerate(filters):
        for seed in pivot_seeds:
            pivots = None if seed is None else ref.dyadic_pivots(n_groups, seed + k)
            want = ref.integer_reduce(frame, surface, generation, rays_per_source, n_groups, pivots)
            got = device._reduce_pass(surface, generation, rays_per_source, n_groups,
                                      None if pivots is None else torch.from_numpy(pivots).to("cuda:0"))
            assert np.array_equal(got.cpu().numpy(), want), (len(frame), surface, generation, seed)
        for quantity, about in (("y1", 0.25), ("axis_intercept", -0.75)):
            count, mean, mean_square = ref.mean_square_table(
                ref.integer_mean_square(frame, quantity, about, surface, generation, rays_per_source, n_groups))
            got = device.mean_square(quantity, about=about, surface=surface, generation=generation,
                                     rays_per_source=rays_per_source, n_groups=n_groups)
            if rays_per_source:
                assert np.array_equal(got["count"].to_numpy(), count)
                assert np.array_equal(got["mean"].to_numpy(), mean, equal_nan=True)
                assert np.array_equal(got["mean_square"].to_numpy(), mean_square, equal_nan=True)
            else:
                assert np.array_equal([got], mean_square, equal_nan=True)


# ---- row counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, 4 * WAVE + 1])
def test_sums_are_exact_at_every_row_count(n_rows):
    frame, block = labelled(ref.dyadic_frame(n_rows, n_rows), n_rows + 1)
    device = device_frame(frame)
    check_exact(frame, device, 7, -(-block // 7))        # (7: no power of two; a few hundred groups at the largest)
    check_exact(frame, device, None, 1)
    whole = ref.integer_reduce(frame)
    assert whole[0, 0] == n_rows and np.array_equal(device._reduce_pass(None, None, None, 1, None).cpu().numpy(), whole)
    # values that select nothing at all
    assert not device._reduce_pass(8.0, None, None, 1, None).any() and not device._reduce_pass(None, 7.0, 7, 3, None).any()


# ---- both sides of the slot switch --------------------------------------------------------------------------------------------
SWITCH = [(ref.slot_switch_rows(1) - 1, 1), (ref.slot_switch_rows(1), 1), (ref.slot_switch_rows(2) - 1, 2),
          (ref.slot_switch_rows(2), 2), (ref.slot_switch_rows(3) + 100 * WAVE + 37, 3)]


@pytest.mark.parametrize("n_rows,n_groups", SWITCH)
def test_sums_are_exact_on_both_sides_of_the_slot_switch(n_rows, n_groups):
    frame, device, rays_per_source = big_dyadic(n_rows, n_groups)
    on_slots = n_rows >= ref.slot_switch_rows(n_groups)
    assert ref.frame_slots(n_rows, n_groups) == (ref.FRAME_SLOTS if on_slots else 1)
    assert n_groups < 3 or (on_slots and n_rows % WAVE)
    check_exact(frame, device, rays_per_source if n_groups > 1 else None, n_groups,
                filters=((None, None), (3.0, 2.0)), pivot_seeds=(None,))
    check_exact(frame, device, rays_per_source, n_groups, filters=((3.0, None), (None, 1.0)), pivot_seeds=(5,))
    want = ref.integer_reduce(frame, None, None, rays_per_source, n_groups)
    assert want[:, 0].sum() == n_rows and (want[:, 0] > 0).all()


# ---- group changes --------------------------------------------------------------------------------------------------------------
def test_sums_are_exact_across_group_changes():
    n = 2 * WAVE + 500
    rng = np.random.default_rng(8)
    base, _ = labelled(ref.dyadic_frame(n, 21), 22)
    row = np.arange(n)
    cases = {
        # a change inside the second slice (row 100), one exactly at the wave boundary (row 1024)
        "inside a slice and at a wave boundary": (np.where(row < 100, 0, np.where(row < WAVE, 1, 2)) * 1000 + row % 1000,
                                                  1000, 4),
        "64 groups in a slice": (row, 1, n),
        "rays_per_source that is no power of two": (row, 3, -(-n // 3)),
        # ids below 0 and at or above n_groups * rays_per_source are not counted; groups 1, 3 and 5 have no rows
        "ids outside the groups, empty groups": (np.where(row % 5 == 0, -1 - row, np.where(row % 7 == 0, 6 * 500 + row,
                                                                                        (row % 3) * 2 * 500 + row % 500)), 500, 6),
        # not ascending: a group is met again after its sums were flushed, within a slice and across slices
        "revisited groups": (rng.integers(0, 5 * 40, n), 40, 5),
        "revisited in runs": ((row // 96) % 3 * 100, 100, 3),
    }
    for name, (ids, rays_per_source, n_groups) in cases.items():
        frame = base.copy()
        frame[:, IX["id"]] = ids
        want = ref.integer_reduce(frame, None, None, rays_per_source, n_groups)
        if name.startswith("ids outside"):
            assert not want[1::2, 0].any() and want[::2, 0].all() and want[:, 0].sum() < n - n // 5
        check_exact(frame, device_frame(frame), rays_per_source, n_groups)


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_an_offset_view_and_a_frame_that_is_not_contiguous():
    from pyrayt_amd.frame import DeviceFrame

    n = 5 * WAVE + 11
    frame, block = labelled(ref.dyadic_frame(n, 31), 32)
    rows = torch.from_numpy(np.ascontiguousarray(frame.T)).to("cuda:0")
    a, b = 37, n - 3 * WAVE - 5  # (a > 0: the base pointer is offset; ld = n > b - a)
    view = DeviceFrame(rows[:, a:b])
    assert view.rows.stride(0) == n > len(view) and view.rows.stride(1) == 1 and view.rows.data_ptr() != rows.data_ptr()
    assert view._contiguous_rows().data_ptr() == view.rows.data_ptr()   # (read in place)
    check_exact(frame[a:b], view, 7, -(-block // 7))
    # a transposed block and a strided selection: the .contiguous() route
    for device, want in ((DeviceFrame(torch.from_numpy(frame).to("cuda:0").T), frame),
                         (DeviceFrame(rows[:, 1::2]), frame[1::2])):
        assert device.rows.stride(1) != 1
        made = device._contiguous_rows()
        assert made.stride(1) == 1 and made.data_ptr() != device.rows.data_ptr()
        check_exact(want, device, 7, -(-block // 7), filters=((None, None), (4.0, 2.0)))
        stats = device.group_stats(rays_per_source=7, n_groups=2)   # (prt_frame_stats takes the same route)
        assert np.array_equal(stats["count"].to_numpy(), ref.integer_reduce(want, None, None, 7, 2)[:, 0])


# ---- the statistics, which are not exact: every one within its derived bound ---------------------------------------------------------
def note(name, deviation, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, deviation / bound, np.where(deviation > 0, np.inf, 0.0))
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(np.nanmax(ratio)))
    print(f"deviation / bound, {name}: {float(np.nanmax(ratio)):.3g} (largest so far {RATIOS[name]:.3g})")
    return ratio


STATS = ("count", "y", "z", "rms_radius", "focus", "focus_std", "wavelength", "intensity")


@pytest.mark.parametrize("n_rows,n_groups,centre,width", [
    (ref.slot_switch_rows(1) - 1, 1, (0.3, -0.2), 1.0), (ref.slot_switch_rows(1), 1, (0.3, -0.2), 1.0),
    (ref.slot_switch_rows(2) - 1, 2, (0.3, -0.2), 1.0), (ref.slot_switch_rows(2), 2, (0.3, -0.2), 1.0),
    (ref.slot_switch_rows(2), 2, (1e3, -1e3), 1e-6), (ref.slot_switch_rows(3) + 100 * WAVE + 37, 3, (0.3, -0.2), 1.0)])
def test_statistics_stay_inside_the_derived_bound(n_rows, n_groups, centre, width):
    frame, rays_per_source = ref.random_frame(n_rows, n_groups, 17 + n_groups, centre, width)
    device = device_frame(frame)
    want = ref.stats_reference(frame, None, None, rays_per_source, n_groups)
    bound = ref.stats_bound(want, ref.reduce_depth(want.group, n_groups, ref.frame_slots(n_rows, n_groups)))
    got = device.group_stats(rays_per_source=rays_per_source, n_groups=n_groups)[list(STATS)].to_numpy(dtype=np.float64)
    assert np.array_equal(got[:, 0], want.stats[:, 0].astype(np.float64))
    deviation = np.abs(got - want.stats).astype(np.float64)
    for k, name in enumerate(STATS[1:], 1):
        ratio = note(f"group_stats {name}", deviation[:, k], bound[:, k])
        assert np.all(ratio <= 1.0), (name, deviation[:, k], bound[:, k])
    # the coma metric's shape: mean square of sin(y_tilt) - c, grouped and over the whole frame
    want, bound = ref.mean_square_reference(frame, "y_tilt", 0.17, "sin", None, None, rays_per_source, n_groups)
    got = device.mean_square("y_tilt", about=0.17, transform="sin", rays_per_source=rays_per_source, n_groups=n_groups)
    assert np.array_equal(got["count"].to_numpy(), want[:, 0].astype(np.int64))
    for k, name in ((1, "mean"), (2, "mean_square")):
        ratio = note(f"mean_square sin {name}", np.abs(got[name].to_numpy() - want[:, k]).astype(np.float64), bound[:, k])
        assert np.all(ratio <= 1.0), (name, got[name].to_numpy(), want[:, k], bound[:, k])
    want, bound = ref.mean_square_reference(frame, "y_tilt", 0.17, "sin")
    got = device.mean_square("y_tilt", about=0.17, transform="sin")
    assert note("mean_square sin mean_square", np.abs(np.array([got]) - want[:, 2]).astype(np.float64), bound[:, 2]) <= 1.0
