"""The frame histograms on the device (DeviceFrame.histogram / histogram2d) where the host's plan changes arm, against
exact integers: the last row count at which two 16-bit tallies share a word (every workgroup counts 64 512 rows into one
half-word) and the first at which they do not, the window flushed by atomics and by the slab that
k_frame_histogram_fold adds up, with packed and with whole words, an odd last window, one pass and a ragged pass of the
grid-stride loop, and weight sums that are representable in every order, compared on bit images.  plan()
(tests/histogram_partitions.py, held to the source by tests/test_host_histogram_partitions.py) restates
prt_frame_histogram's choices from the CU count the library reads; every case asserts the arm it is named for before
it calls the device.  The large frames are built on the device and their counts are known in closed form.  No case is sampled or filtered by its result."""
import numpy as np
import pytest

from histogram_partitions import BLOCK, FOLD_CHUNKS, MAX_PER_CU, arm_rows, last_packed_rows, plan, slab_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
IX = {name: k for k, name in enumerate(COLUMNS)}


def cus():
    return max(1, torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def block():
    """One (15, 64 * 1024 * cus) block of zeros on the device (2 GB at 256 CUs): the large frames are views of it with
    one column filled."""
    rows = torch.zeros((15, 64 * BLOCK * cus()), dtype=torch.float64, device="cuda:0")
    yield rows
    del rows
    torch.cuda.empty_cache()


def view(block, n_rows, column, values):
    from pyrayt_amd.frame import DeviceFrame

    rows = block[:, :n_rows]
    rows[IX[column]] = values
    return DeviceFrame(rows)


def ramp(n_rows, period, offset=0.5):
    """offset + (row number mod period), on the device."""
    return torch.arange(n_rows, device="cuda:0", dtype=torch.float64).remainder_(period).add_(offset)


def spread_counts(n_rows, bins):
    """Rows dealt to the bins in turn."""
    return np.full(bins, n_rows // bins, dtype=np.float64) + (np.arange(bins) < n_rows % bins)


def from_host(frame):
    from pyrayt_amd.frame import DeviceFrame

    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the half-word bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ("last packed", "first unpacked", "a full half-word"))
@pytest.mark.parametrize("bins", (2, 65536))
def test_a_workgroup_counts_64512_rows_into_one_half_word(block, bins, size):
    """63 * 1024 rows a CU is the last packed size: every workgroup counts 64 512 rows, and with all of them in one bin
    a half-word holds 64 512 of its 65 535.  One row more and the tallies are whole words; at 64 * 1024 rows a CU a
    workgroup counts the 65 536 rows that a half-word would turn into 0.  Two bins flush by atomics; 65 536 bins are
    one packed window (two unpacked ones) on the slab side, where k_frame_histogram_fold adds one half-word of 64 512
    (one word of up to 65 536) per workgroup."""
    n = dict([("last packed", last_packed_rows(cus())), ("first unpacked", last_packed_rows(cus()) + 1),
              ("a full half-word", 64 * BLOCK * cus())])[size]
    p = plan(n, bins, cus())
    if size == "last packed":
        assert p.packed and p.grid == cus() and p.per_cu == 1 and p.share_rows == 64512 < 65536 and n == 64512 * p.grid
        assert p.window == bins and p.windows == 1
    else:
        assert not p.packed and p.window == min(bins, 32768) and p.windows == bins // p.window
        assert p.grid == cus() * p.per_cu and p.per_cu == (2 if bins == 2 else 1)
        assert p.share_rows == 65536 // p.per_cu and (size == "first unpacked" or n == p.share_rows * p.grid)
    assert p.slab == (bins == 65536) and (p.ratio >= 2 or p.ratio <= 0.5)
    low = 0 if bins == 2 else 40_000          # an even bin, the odd one beside it in the same word, and the last bin
    for name, values in (("even", low + 0.5), ("odd", low + 1.5), ("last", bins - 0.5), ("alternating", None)):
        want = np.zeros(bins)
        if values is None:
            values = ramp(n, 2, low + 0.5)
            want[low], want[low + 1] = (n + 1) // 2, n // 2
        else:
            want[int(values)] = n
        hist, edges = view(block, n, "y1", values).histogram("y1", bins=bins, range=(0, bins))
        assert np.array_equal(edges, np.arange(bins + 1.0))
        assert np.array_equal(hist, want), (name, np.flatnonzero(hist != want)[:8], hist[hist != want][:8])


# ---- the flush arms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["packed, atomic", "packed, slab", "packed, slab, last window of one bin", "unpacked, atomic",
                                 "unpacked, slab"])
def test_the_flush_arms_by_name(block, arm):
    """Rows dealt to the bins in turn: every bin holds n // bins rows or one more.  65 537 bins leave a last window of
    one bin, half a word: its slab is one word a workgroup and the fold adds its low half alone.  (The fold's guard
    `2 * w + 1 < window` is not what this pins: the kernel drops every bin at or past the window, so the high half of
    that word is 0 and the guard has nothing to decide.)"""
    n, bins = arm_rows(arm, cus())
    p = plan(n, bins, cus())
    print(arm, n, bins, p)
    assert p.packed == arm.startswith("packed") and p.slab == ("slab" in arm)
    assert p.ratio >= 2 if p.slab else p.ratio <= 0.5
    if "last window of one bin" in arm:
        assert p.window == 65536 and p.windows == 2 and bins - p.window == 1
    if arm == "unpacked, slab":
        assert p.window == 32768 and p.windows == 2
    hist, _ = view(block, n, "y1", ramp(n, bins)).histogram("y1", bins=bins, range=(0, bins))
    want = spread_counts(n, bins)
    assert want.sum() == n and np.array_equal(hist, want), (np.flatnonzero(hist != want)[:8], hist[hist != want][:8])


def test_a_fold_over_a_grid_that_is_no_multiple_of_eight(block):
    """k_frame_histogram_fold adds the slabs in eight chunks of ceil(grid / 8) workgroups, the last ones short or empty
    when the grid is no multiple of 8.  The grid of a slab flush is the CU count (a smaller grid has at most 1024 rows a
    workgroup, which never reaches the slab: asserted), so the ragged chunks are entered where the CU count is no
    multiple of 8.  Where it is one -- the whole MI355X has 256 -- no row count reaches them through the library: the
    case then runs whole chunks only, and the ragged arm of the fold stays unexecuted there (a gap)."""
    count = cus()
    for blocks in range(1, count):
        for bins in (2, 64, 1024, 4096, 16384, 32768, 65536, 65537, 1 << 20):
            for n in ((blocks - 1) * BLOCK + 1, blocks * BLOCK):
                assert plan(n, bins, count).grid == blocks and not plan(n, bins, count).slab
    n, bins = slab_rows(count, 65536), 65536
    p = plan(n, bins, count)
    assert p.slab and p.packed and p.grid == count
    per = -(-p.grid // FOLD_CHUNKS)
    print("grid", p.grid, "workgroups a chunk", per, "ragged" if p.grid % FOLD_CHUNKS else "whole")
    assert (per * FOLD_CHUNKS > p.grid) == (count % FOLD_CHUNKS != 0)
    hist, _ = view(block, n, "y1", ramp(n, 3, 65533 + 0.5)).histogram("y1", bins=bins, range=(0, bins))
    want = np.zeros(bins)
    want[65533:] = spread_counts(n, 3)
    assert np.array_equal(hist, want)


# ---- one pass and a ragged pass of the grid-stride loop ---------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
def test_row_counts_beside_a_pass_of_the_grid(block, weighted):
    """1, 1023, 1024 and 1025 rows (one workgroup, ragged, whole, and a second one with one row), and one row fewer
    and one more than 1024 * grid: the last workgroup one row short, and a second pass of one row."""
    count = cus()
    full = count * (MAX_PER_CU if weighted else 1)
    assert plan(BLOCK * full + 1, 7, count, weighted).grid == full and plan(BLOCK * full, 7, count, weighted).grid == full
    try:
        rows_beside_a_pass(block, weighted, count, full)
    finally:
        block[IX["intensity"]] = 0.0   # (the shared block goes back as it came, whatever a case found)


def rows_beside_a_pass(block, weighted, count, full):
    for n, grid in ((1, 1), (1023, 1), (1024, 1), (1025, 2), (BLOCK * full - 1, full), (BLOCK * full + 1, full)):
        if grid > full:
            continue
        p = plan(n, 7, count, weighted)
        assert p.grid == grid and p.share_rows == (2048 if n == BLOCK * full + 1 else 1024) and not p.slab
        frame = view(block, n, "y1", ramp(n, 7))
        if not weighted:
            hist, _ = frame.histogram("y1", bins=7, range=(0, 7))
            assert np.array_equal(hist, spread_counts(n, 7)), n
        else:  # weights -2 .. 2 by row number mod 5: integers, exact
            frame.rows[IX["intensity"]] = ramp(n, 5, -2.0)
            hist, _ = frame.histogram("y1", bins=7, range=(0, 7), weights="intensity")
            i = np.arange(n)
            want = np.bincount(i % 7, weights=i % 5 - 2.0, minlength=7)
            assert np.array_equal(hist, want), n


# ---- weights, bit for bit ---------------------------------------------------------------------------------------------------
N_DYADIC = 200_000


def dyadic_frame():
    """Weights k / 32 with k from -127 to 127 (every partial sum of 200 000 of them is a double, so any order of adding
    gives the same one), y1 and z1 scattered over [0, 1), ids in three groups."""
    i = np.arange(N_DYADIC)
    frame = np.zeros((N_DYADIC, 15))
    frame[:, IX["id"]] = i
    frame[:, IX["intensity"]] = ((i * 37) % 255 - 127) / 32.0
    frame[:, IX["y1"]] = ((i * 7919) % 1_000_003) / 1_000_003.0
    frame[:, IX["z1"]] = ((i * 104_729) % 999_983) / 999_983.0
    return frame


def test_dyadic_weight_sums_are_the_same_bits_as_numpy():
    frame = dyadic_frame()
    w = frame[:, IX["intensity"]]
    assert w.min() == -127 / 32 and w.max() == 127 / 32 and np.all(w * 32 == np.round(w * 32)) and np.abs(w).sum() * 32 < 2 ** 53
    device = from_host(frame)
    for bins, windows, last in ((10_921, 1, 10_921), (10_922, 1, 10_922), (10_923, 2, 1)):
        p = plan(N_DYADIC, bins, cus(), weighted=True)
        assert p.window == min(bins, 10_922) and p.windows == windows and bins - (windows - 1) * p.window == last
        assert not p.slab and not p.packed
        hist, edges = device.histogram("y1", bins=bins, range=(0, 1), weights="intensity")
        want, want_edges = np.histogram(frame[:, IX["y1"]], bins=bins, range=(0, 1), weights=w)
        assert np.array_equal(edges, want_edges) and np.array_equal(bits(hist), bits(want)), bins
        assert (want < 0).sum() > 1000 and (want > 0).sum() > 1000
    # 3 x 150 x 150: seven windows of 10 922 bins, two of which straddle a group boundary
    rays_per_source, shape = 66_667, (3, 150, 150)
    p = plan(N_DYADIC, 3 * 150 * 150, cus(), weighted=True)
    assert p.window == 10_922 and p.windows == 7 and 22_500 % p.window != 0 and 45_000 % p.window != 0
    hist, xe, ye = device.histogram2d("y1", "z1", bins=150, range=((0, 1), (0, 1)), weights="intensity",
                                      rays_per_source=rays_per_source, n_groups=3)
    assert hist.shape == shape
    for g in range(3):
        m = frame[:, IX["id"]] // rays_per_source == g
        want, _, _ = np.histogram2d(frame[m, IX["y1"]], frame[m, IX["z1"]], bins=150, range=((0, 1), (0, 1)), weights=w[m])
        assert m.sum() > 60_000 and np.array_equal(bits(hist[g]), bits(want)), g


@pytest.mark.parametrize("bins", (10, 10_923))
def test_weights_that_are_not_finite_stay_in_their_bins(bins):
    """One NaN, one +inf and one -inf weight in three different bins: those bins hold what numpy puts there, every
    other bin is exact, and the counts do not see the weights."""
    frame = dyadic_frame()
    y, w = frame[:, IX["y1"]], frame[:, IX["intensity"]]
    rows = (11, 50, 90)
    w[list(rows)] = (np.nan, np.inf, -np.inf)
    where = [int(np.floor(y[r] * bins)) for r in rows]
    assert len(set(where)) == 3
    device = from_host(frame)
    with np.errstate(invalid="ignore"):
        want, _ = np.histogram(y, bins=bins, range=(0, 1), weights=w)
    assert np.isnan(want[where[0]]) and want[where[1]] == np.inf and want[where[2]] == -np.inf
    assert np.isfinite(np.delete(want, where)).all()
    hist, _ = device.histogram("y1", bins=bins, range=(0, 1), weights="intensity")
    assert np.array_equal(np.isnan(hist), np.isnan(want)) and np.isnan(hist).sum() == 1
    assert np.array_equal(bits(hist[~np.isnan(want)]), bits(want[~np.isnan(want)]))
    counts, _ = device.histogram("y1", bins=bins, range=(0, 1))
    assert np.array_equal(counts, np.histogram(y, bins=bins, range=(0, 1))[0]) and counts.sum() == N_DYADIC
