"""prt_frame_launch_index and prt_frame_ray_aberrations at the edges of their partition, against
tests/aberration_sums_reference.py: on dyadic frames, whose sums are exact in any order, bit for bit against integers (no
tolerance); where the arithmetic rounds -- the centroid, rho from the extent, the normal equations above one term,
frames on no grid -- within the bounds derived there (no fixed tolerance anywhere: deviation / bound <= 1).

The edges: one row and one ragged slice; a bucket on both sides of an LDS tile (kAbBlock) and of a chunk (kMtfChunk), alone
and among rows of another surface; a group folded over zone buckets of several chunks; the wave boundary, a group change
on it and inside a slice; 64 buckets in one slice; the scan with two waves a thread and a ragged last wave (524 289
rows); the wave cap (2 097 153 rows); the count cap that cuts the waves (65 536 buckets).  Every case first asserts, with
the partition rules restated in the reference module, that it reaches the arm it is named for.  No case is sampled or
filtered by its result: the only rows left out are those the definitions leave out, and they are counted."""
import numpy as np
import pytest

import aberration_sums_reference as ab
import frame_sums_reference as ref
from test_gpu_frame_partitions import note

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX
SCAN_ROWS = ab.MTF_SCAN_BLOCK * ab.WF_ROWS_PER_WAVE + 1      # 524 289: the smallest frame with two waves a scan thread
CAP_ROWS = ab.WF_MAX_WAVES * ab.WF_ROWS_PER_WAVE + 1         # 2 097 153: the smallest frame above the wave cap
COUNT_ROWS, COUNT_GROUPS, COUNT_ZONES = 200_000, 64, 1024    # 65 536 buckets: the count cap allows 128 waves
_CACHE = {}


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist()
    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)).to("cuda:0"), counts)


def sized_frame(n_rows, n_rays, seed, id0=0, selected_ids=None, n_other=0, shuffle_launch=False, launched=None):
    """A dyadic frame of n_rows rows: launch rows for the ids id0 .. id0 + n_rays - 1 (``launched``: a mask of those that
    have one), the selected generation (surface 5.0: ``selected_ids``, default all ids ascending, with ``n_other`` rows of
    surface 6.0 spread among them) and an intermediate generation that fills the frame up to n_rows."""
    rng = np.random.default_rng(seed + 1)
    ids = id0 + np.arange(n_rays)
    selected = ids if selected_ids is None else np.asarray(selected_ids)
    last = np.concatenate([selected, id0 + n_rays + np.arange(n_other)])
    other = np.zeros(len(last), dtype=bool)
    other[len(selected):] = True
    if n_other:
        place = np.sort(rng.choice(len(last), n_other, replace=False))
        mask = np.zeros(len(last), dtype=bool)
        mask[place] = True
        merged = np.zeros(len(last), dtype=last.dtype)
        merged[mask], merged[~mask] = last[other], last[~other]
        last, other = merged, mask
    launch = ids if launched is None else ids[launched]
    if shuffle_launch:
        launch = rng.permutation(launch)
    n_middle = n_rows - len(launch) - len(last)
    assert n_middle >= 1
    frame = ab.dyadic_aberration_frame(launch, id0 + np.arange(n_middle) % n_rays, last, seed)
    assert len(frame) == n_rows
    frame[np.flatnonzero(frame[:, 0] == 2)[other], IX["surface"]] = 6.0
    return frame


def cached(name, build):
    """(frame, DeviceFrame, the dictionary join), built once."""
    if name not in _CACHE:
        frame = build()
        _CACHE[name] = (frame, device_frame(frame), ab.join(frame))
    return _CACHE[name]


def run(device, terms, surface=None, generation=None, pupil="position", origin=(0.0, 0.0, 0.0), reference="centroid",
        axes=None, pupil_radius=None, zones=64, weights=None, rays_per_source=None, n_groups=None):
    frame_axes = {} if axes is None else dict(axis=axes[0:3], basis=(axes[3:6], axes[6:9]))
    return device.ray_aberrations(surface, pupil=pupil, launch_origin=origin, reference=reference,
                                  pupil_radius=pupil_radius, zernike=terms, zones=zones, weights=weights,
                                  generation=generation, rays_per_source=rays_per_source, n_groups=n_groups, **frame_axes)


def check_exact(frame, device, index=None, **options):
    """Everything the pass reports at one term, bit for bit against the integers."""
    options = dict(dict(surface=5.0, reference=(0.25, 0.5, -0.5), pupil_radius=4.0), **options)
    want = ab.integer_aberrations(frame, index=index, **options)
    got = run(device, 1, **options)
    assert np.array_equal(got.rows.cpu().numpy(), want.rows)   # (compacted in row order, over all the groups)
    assert np.array_equal(got.n_rays, want.n_rays) and np.array_equal(got.n_missed, want.n_missed)
    assert np.array_equal(got.chief_row, want.chief) and np.array_equal(got.n_longitudinal, want.n_la)
    assert np.array_equal(got.pupil_radius, np.full(len(want.n_rays), options["pupil_radius"]))
    assert np.array_equal(got.centre, want.centre, equal_nan=True)
    assert np.array_equal(got.record[:, 8:16], want.sums), np.flatnonzero((got.record[:, 8:16] != want.sums).any(1))
    assert np.array_equal(got.normal, want.normal)
    assert got.zones.shape == want.zones.shape and np.array_equal(got.zones, want.zones)
    assert np.array_equal(got.rays.cpu().numpy(), want.rays, equal_nan=True)
    return got, want


def ratio_of(name, got, want, bound):
    ratio = note(name, np.abs(np.asarray(got) - want).astype(np.float64), np.asarray(bound))
    assert np.all(ratio <= 1.0), (name, float(np.nanmax(ratio)), np.unravel_index(np.nanargmax(ratio), ratio.shape))


def check_bounded(name, frame, device, terms, index=None, fit=True, **options):
    """The pass within the derived bounds of the longdouble reference; the counts and the zone populations exactly."""
    options = dict(dict(surface=5.0), **options)
    got = run(device, terms, **options)
    want = ab.bounded_aberrations(frame, got.centre, got.pupil_radius, terms=terms, index=index, fit=fit, **options)
    assert np.array_equal(got.rows.cpu().numpy(), want.rows)
    assert np.array_equal(got.n_rays, want.n_rays) and np.array_equal(got.n_missed, want.n_missed)
    assert np.array_equal(got.chief_row, want.chief) and np.array_equal(got.n_longitudinal, want.n_la)
    full = want.n_rays > 0
    assert full.any()
    if options.get("reference", "centroid") == "centroid":
        assert np.all(np.isnan(got.centre[~full]))
    ratio_of(f"{name} centre", got.centre[full], want.centre_ref[full], want.centre_bound[full])
    ratio_of(f"{name} rho", got.pupil_radius[full], want.rho_ref[full], want.rho_bound[full])
    rays = got.rays.cpu().numpy()
    assert np.array_equal(np.isnan(rays), np.isnan(want.rays.astype(np.float64)))   # (la without an intercept: NaN)
    fin = ~np.isnan(rays[:, 6])
    for what, columns in (("p", slice(0, 2)), ("eps", slice(2, 4)), ("s", slice(4, 6))):
        ratio_of(f"{name} {what}", rays[:, columns], want.rays[:, columns], want.rays_bound[:, columns])
    ratio_of(f"{name} la", rays[fin, 6], want.rays[fin, 6], want.rays_bound[fin, 6])
    ratio_of(f"{name} sums", got.record[:, 8:16], want.sums, want.sums_bound)
    if options.get("zones", 64):
        assert np.array_equal(got.zones[:, :, [0, 5]], want.zones[:, :, [0, 5]].astype(np.float64))
        ratio_of(f"{name} zones", got.zones, want.zones, want.zones_bound)
    ratio_of(f"{name} normal", got.normal, want.normal, want.normal_bound)
    if fit:
        assert want.coef
        for g, coef in want.coef.items():
            assert got.rank[g] == terms
            ratio_of(f"{name} coefficients", got.coefficients[g], coef, np.tile(want.coef_bound[g][:, None], (1, terms)))
            assert want.coef_bound[g].max() < 2.0 ** -20 * np.abs(coef).max()   # (the bound says something: twenty bits)
    return got, want


# ---- one row, one ragged slice, the LDS tile, the chunk ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_one_row_and_one_ragged_slice(n):
    frame = sized_frame(3 * n, n, n)
    assert ab.ab_waves(len(frame), 1, 64) == 1 and ab.ab_per_wave(len(frame), 1, 64) == -(-3 * n // 64) * 64
    device = device_frame(frame)
    _, want = check_exact(frame, device)
    assert want.n_rays[0] == n
    check_exact(frame, device, generation=2, surface=None, weights="intensity", reference="chief", zones=3, pupil="direction")


@pytest.mark.parametrize("n", [ab.AB_BLOCK - 1, ab.AB_BLOCK, ab.AB_BLOCK + 1])
def test_a_bucket_on_both_sides_of_an_lds_tile(n):
    assert ab.ab_tiles(n) == (2 if n > ab.AB_BLOCK else 1) and ab.ab_chunks(n) == 1
    frame = sized_frame(3 * n, n, n)
    device = device_frame(frame)
    _, want = check_exact(frame, device, zones=0, weights="intensity")
    assert want.buckets.tolist() == [[n]]   # (every ray is used, in the one bucket)


@pytest.mark.parametrize("n_other", [0, 4196])
@pytest.mark.parametrize("n", [ab.MTF_CHUNK - 1, ab.MTF_CHUNK, ab.MTF_CHUNK + 1, 2 * ab.MTF_CHUNK + 1])
def test_a_bucket_on_both_sides_of_a_chunk(n, n_other):
    assert ab.ab_chunks(n) == {4095: 1, 4096: 1, 4097: 2, 8193: 3}[n] and ab.ab_tiles(n) == (1 if n % ab.MTF_CHUNK == 1 else 16)
    frame = sized_frame(3 * n + n_other, n, n, n_other=n_other)
    assert (frame[:, IX["surface"]] == 6.0).sum() == n_other and ab.ab_waves(len(frame), 1, 0) >= 12
    device = device_frame(frame)
    _, want = check_exact(frame, device, zones=0, weights="intensity")
    assert want.buckets.tolist() == [[n]]   # (every ray is used, in the one bucket)
    check_exact(frame, device, zones=0, reference="chief")


def test_a_group_folded_over_zone_buckets_of_several_chunks():
    counts = (200, ab.MTF_CHUNK + 1, 100)
    n = sum(counts)
    frame = sized_frame(3 * n, n, 21)
    rng = np.random.default_rng(21)
    zone = rng.permutation(np.repeat(np.arange(3), counts))
    # rho = 2, three zones: |h| < 2/3, < 4/3, the rest -- h = (y0, z0) of the launch rows
    y = np.where(zone == 0, rng.integers(-128, 129, n), np.where(zone == 1, rng.integers(192, 321, n), rng.integers(384, 511, n)))
    frame[:n, IX["y0"]], frame[:n, IX["z0"]] = y / ab.GRID, np.where(zone == 0, rng.integers(-64, 65, n), 0) / ab.GRID
    device = device_frame(frame)
    for options in (dict(), dict(weights="intensity", reference="chief")):
        _, want = check_exact(frame, device, zones=3, pupil_radius=2.0, **options)
        assert want.buckets.tolist() == [list(counts)] and ab.ab_chunks(want.buckets).tolist() == [[1, 2, 1]]
    assert np.array_equal(want.zone, zone)


# ---- the wave boundary -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [ab.WF_ROWS_PER_WAVE - 1, ab.WF_ROWS_PER_WAVE, ab.WF_ROWS_PER_WAVE + 1])
def test_a_frame_on_both_sides_of_one_wave(n_rows):
    n = n_rows // 3
    frame = sized_frame(n_rows, n, n_rows)
    assert ab.ab_waves(n_rows, 2, 64) == (2 if n_rows > ab.WF_ROWS_PER_WAVE else 1)
    assert ab.ab_per_wave(n_rows, 2, 64) == (576 if n_rows > ab.WF_ROWS_PER_WAVE else 1024)
    device = device_frame(frame)
    assert frame[-1, IX["surface"]] == 5.0   # (the frame's last row is selected)
    _, want = check_exact(frame, device, rays_per_source=171, n_groups=2, weights="intensity")
    assert want.n_rays.tolist() == [171, n - 171]
    check_exact(frame, device, zones=0)


def test_group_changes_on_a_wave_boundary_and_inside_a_slice():
    n_rows, n = 4096, 1400
    frame = sized_frame(n_rows, n, 31)
    per_wave = ab.ab_per_wave(n_rows, 4, 5)
    start = n_rows - n                                   # the selected generation's first row
    on_boundary = 3 * per_wave - start                   # the ray whose row opens the fourth wave
    assert ab.ab_waves(n_rows, 4, 5) == 4 and per_wave == 1024 and 0 < on_boundary < n
    assert (start + on_boundary) % per_wave == 0 and (start + 2 * on_boundary) % 64 != 0
    device = device_frame(frame)
    _, want = check_exact(frame, device, rays_per_source=on_boundary, n_groups=4, zones=5, weights="intensity")
    assert want.n_rays.tolist() == [on_boundary] * 3 + [n - 3 * on_boundary]
    _, fewer = check_exact(frame, device, rays_per_source=on_boundary, n_groups=2, zones=5, reference="chief")
    assert fewer.n_rays.tolist() == [on_boundary] * 2 and len(fewer.rows) == 2 * on_boundary   # (ids past the groups are absent)


def test_sixty_four_buckets_in_one_slice():
    n_rows, n = 3 * 1024, 1000
    frame = sized_frame(n_rows, n, 41)
    start = n_rows - n
    first = -start % 64 + 128                            # a ray whose row opens a slice
    assert (start + first) % 64 == 0 and ab.ab_waves(n_rows, 1, 64) == 3
    rays = first + np.arange(64)
    frame[rays, IX["y0"]], frame[rays, IX["z0"]] = (8 * np.arange(64) + 4) / ab.GRID, 0.0   # |p| = (k + 1/2) / 64 at rho = 2
    device = device_frame(frame)
    _, want = check_exact(frame, device, zones=64, pupil_radius=2.0, weights="intensity")
    assert np.array_equal(want.rows[first:first + 64], start + rays) and np.array_equal(want.zone[first:first + 64], np.arange(64))
    assert np.all(want.buckets >= 1)


# ---- the large frames ---------------------------------------------------------------------------------------------------------
def test_the_scan_with_two_waves_a_thread_and_a_ragged_last_wave():
    n = SCAN_ROWS // 3
    frame, device, index = cached("scan", lambda: sized_frame(SCAN_ROWS, n, 51))
    assert ab.ab_waves(SCAN_ROWS, 1, 0) == 513 and ab.ab_all_waves(SCAN_ROWS, 1, 0) == 516
    assert ab.ab_scan_per(SCAN_ROWS, 5, 7) == 2 and ab.ab_scan_per(SCAN_ROWS - 1, 5, 7) == 1
    assert ab.ab_per_wave(SCAN_ROWS, 5, 7) == ab.WF_ROWS_PER_WAVE and SCAN_ROWS % ab.WF_ROWS_PER_WAVE == 1
    assert frame[-1, IX["surface"]] == 5.0               # (the last wave holds one row, and it is selected)
    _, want = check_exact(frame, device, index, zones=0)
    assert want.n_rays[0] == n and ab.ab_chunks(n) == 43
    rays_per_source = 37_001                             # no power of two; the groups' edges fall inside waves
    _, want = check_exact(frame, device, index, rays_per_source=rays_per_source, n_groups=5, zones=7, weights="intensity",
                          reference="chief", pupil="direction", pupil_radius=2.0)
    assert want.n_rays.tolist() == [rays_per_source] * 4 + [n - 4 * rays_per_source]
    assert all((SCAN_ROWS - n + k * rays_per_source) % ab.WF_ROWS_PER_WAVE for k in range(1, 5))


def cap_frame():
    n = CAP_ROWS // 3
    launched = np.ones(n, dtype=bool)
    launched[::1013] = False                             # rays that were never launched
    frame = sized_frame(CAP_ROWS, n, 61, id0=100_000, shuffle_launch=True, launched=launched)
    return frame


def test_the_join_above_the_wave_cap():
    frame, device, index = cached("cap", cap_frame)
    ids = frame[frame[:, 0] == 0, IX["id"]]
    assert len(frame) == CAP_ROWS and ids.min() >= 100_000 and np.any(np.diff(ids) < 0) and (index < 0).sum() > 1000
    assert np.array_equal(device.launch_index().cpu().numpy(), index)


def test_the_wave_cap():
    frame, device, index = cached("cap", cap_frame)
    n = CAP_ROWS // 3
    per_wave = ab.ab_per_wave(CAP_ROWS, 3, 9)
    assert ab.ab_waves(CAP_ROWS, 3, 9) == ab.WF_MAX_WAVES and per_wave == 1088 > ab.WF_ROWS_PER_WAVE
    assert ab.ab_per_wave(CAP_ROWS - 1, 3, 9) == ab.WF_ROWS_PER_WAVE and ab.ab_scan_per(CAP_ROWS, 3, 9) == 4
    _, want = check_exact(frame, device, index, zones=0, weights="intensity")
    missed = len(range(0, n, 1013))
    assert want.n_missed[0] >= missed and want.n_rays[0] + want.n_missed[0] == n
    # ids from 100 000 in groups of 250 000: the fourth group's ids are at or above n_groups * rays_per_source
    _, want = check_exact(frame, device, index, rays_per_source=250_000, n_groups=3, zones=9, reference="chief")
    assert (want.n_rays + want.n_missed).tolist() == [150_000, 250_000, 250_000] and want.n_missed.sum() > 500


def count_frame():
    n = COUNT_ROWS // 3
    return sized_frame(COUNT_ROWS, n, 71)


def test_the_count_cap_cuts_the_waves():
    frame, device, index = cached("count", count_frame)
    n = COUNT_ROWS // 3
    rays_per_source = -(-n // COUNT_GROUPS)
    assert ab.ab_buckets(COUNT_GROUPS, COUNT_ZONES) * 8 * 128 == ab.AB_COUNT_BYTES
    assert ab.ab_waves(COUNT_ROWS, COUNT_GROUPS, COUNT_ZONES) == 128 < ab.ab_waves(COUNT_ROWS, 1, 0) == 196
    assert ab.ab_per_wave(COUNT_ROWS, COUNT_GROUPS, COUNT_ZONES) == 1600 and ab.ab_bucket_scan_per(COUNT_GROUPS, COUNT_ZONES) == 128
    assert rays_per_source & (rays_per_source - 1) and rays_per_source * (COUNT_GROUPS - 1) < n
    _, want = check_exact(frame, device, index, rays_per_source=rays_per_source, n_groups=COUNT_GROUPS, zones=COUNT_ZONES,
                          weights="intensity")
    assert np.all(want.n_rays > 0) and (want.buckets == 0).any() and (want.buckets > 1).any()
    # the same frame without the cap: 196 waves
    check_exact(frame, device, index, rays_per_source=rays_per_source, n_groups=COUNT_GROUPS, zones=2)


# ---- content edges, inside a frame of several waves and chunks ---------------------------------------------------------------------
EDGE_RAYS = 2 * ab.MTF_CHUNK + 300


def edge_frame(tie_rows=(), left_out=0, shuffled=False, id0=0):
    """Eight waves, three chunks a group at most.  Launch points off the origin but for the rays of ``tie_rows`` (rows of
    the frame, inside the selected generation); the first ``left_out`` of those rows have a NaN end point."""
    n = EDGE_RAYS
    n_rows = 3 * n
    rng = np.random.default_rng(81)
    selected = id0 + (rng.permutation(n) if shuffled else np.arange(n))
    launched = np.ones(n, dtype=bool)
    launched[[50, 5000, 8000]] = False
    frame = sized_frame(n_rows, n, 82, id0=id0, selected_ids=selected, launched=launched, shuffle_launch=True)
    launch = np.flatnonzero(frame[:, 0] == 0)
    origin = (frame[launch, IX["y0"]] == 0) & (frame[launch, IX["z0"]] == 0)
    frame[launch[origin], IX["y0"]] = 1 / ab.GRID
    index = ab.join(frame)
    for k, row in enumerate(tie_rows):
        assert frame[row, IX["surface"]] == 5.0 and index[row] >= 0
        frame[index[row], IX["y0"]], frame[index[row], IX["z0"]] = 0.0, 0.0
        if k < left_out:
            frame[row, IX["z1"]] = np.nan
    last = np.flatnonzero(frame[:, 0] == 2)
    frame[last[100], IX["intensity"]], frame[last[4200], IX["intensity"]] = -1.0, np.nan
    frame[last[200:264], IX["y_tilt"]] = 0.0            # (a whole slice without an axis intercept: the rays still count)
    return frame


def tie_rows():
    n_rows = 3 * EDGE_RAYS
    per_wave = ab.ab_per_wave(n_rows, 1, 4)
    boundary = (2 * EDGE_RAYS // per_wave + 3) * per_wave
    assert ab.ab_waves(n_rows, 1, 4) > 20 and 2 * EDGE_RAYS < boundary - 1 and boundary + 6000 < n_rows
    return boundary - 1, boundary, boundary + 6000     # the last row of a wave, the first of the next, a much later one


@pytest.mark.parametrize("left_out", [0, 1, 2])
def test_the_smallest_row_of_a_tie_is_the_chief_ray(left_out):
    rows = tie_rows()
    frame = edge_frame(rows, left_out)
    device = device_frame(frame)
    for options in (dict(zones=4), dict(zones=0, weights="intensity", rays_per_source=3 * EDGE_RAYS, n_groups=2)):
        got, want = check_exact(frame, device, reference="chief", **options)
        assert got.chief_row[0] == rows[left_out] and want.n_missed[0] == 3 + left_out + (2 if "weights" in options else 0)
        assert np.array_equal(got.centre[0], frame[rows[left_out], 9:12])
        assert ab.ab_chunks(want.buckets).sum() >= 3


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("options", [
    dict(weights="intensity", zones=6),
    dict(pupil="direction", reference="chief", pupil_radius=2.0),
    dict(weights="intensity", pupil="direction", reference=(1.0, -0.5, 0.125), origin=(0.0, 0.5, -0.25), zones=0),
    dict(origin=(0.0, 0.5, -0.25), reference="chief", zones=1)])
def test_content_edges_in_groups(options, shuffled):
    frame = edge_frame(shuffled=shuffled, id0=100_000)
    # 3001 is no power of two; ids start in the middle of group 33, group 34 (ids 102 034 ..) is emptied, 36 holds the tail
    rays_per_source, n_groups = 3001, 37
    frame[(frame[:, 0] == 2) & (frame[:, IX["id"]] // rays_per_source == 34), IX["surface"]] = 6.0
    device = device_frame(frame)
    got, want = check_exact(frame, device, rays_per_source=rays_per_source, n_groups=n_groups, **options)
    assert np.all(want.n_rays[:33] == 0) and want.n_rays[34] == 0 and np.all(want.n_rays[[33, 35, 36]] > 0)
    assert np.all(got.chief_row[want.n_rays == 0] == -1) and want.n_missed.sum() >= 2
    assert np.isnan(got.rays.cpu().numpy()[:, 6]).sum() >= 60
    per_wave = ab.ab_per_wave(len(frame), n_groups, options.get("zones", 64))
    if not shuffled:   # (the groups' edges fall inside waves)
        edges = 2 * EDGE_RAYS + np.array([35, 36]) * rays_per_source - 100_000
        assert np.all(edges % per_wave != 0) and np.all((edges > 2 * EDGE_RAYS) & (edges < len(frame)))
    fewer, _ = check_exact(frame, device, rays_per_source=rays_per_source, n_groups=35, **options)
    assert fewer.n_rays.sum() == want.n_rays[33]       # (ids at or above n_groups * rays_per_source are absent)


# ---- what rounds: within the derived bounds ---------------------------------------------------------------------------------------
def test_the_centroid_and_the_extent_on_a_dyadic_frame():
    frame = edge_frame((), 0, shuffled=True)
    device = device_frame(frame)
    # (without zones: on a grid many rays lie on a zone's edge exactly, where the running bound cannot decide the zone)
    check_bounded("dyadic centroid", frame, device, 1, fit=False, weights="intensity", zones=0)
    check_bounded("dyadic centroid", frame, device, 6, fit=False, rays_per_source=3001, n_groups=3, pupil="direction", zones=0)


BOUNDED_RAYS = 3 * ab.MTF_CHUNK + 1


@pytest.mark.parametrize("terms,options", [
    (21, dict(weights="intensity", zones=0, origin=(0.0, 0.3, -0.2))),
    (36, dict(weights="intensity", zones=0, origin=(0.0, 0.3, -0.2), reference="chief")),
    (36, dict(zones=16, rays_per_source=5000, n_groups=3, origin=(-5.0, 0.3, -0.2), reference=(8.0, 0.0, 0.0),
              pupil_radius=2.5)),
    (21, dict(pupil="direction", weights="wavelength", zones=64, axes="tilted"))])
def test_a_random_frame_within_the_bounds(terms, options):
    frame, device, index = cached("random", lambda: ab.random_aberration_frame(BOUNDED_RAYS, 91, n_other=4196, id0=100_000))
    options = dict(options)
    if options.get("rays_per_source"):
        frame, device, index = cached("random0", lambda: ab.random_aberration_frame(BOUNDED_RAYS, 92, n_other=4196))
    if options.get("axes") == "tilted":
        c, s = np.cos(0.3), np.sin(0.3)   # (e1, e2 turned about the axis: the cone of launch directions stays centred)
        options["axes"] = np.array([1.0, 0.0, 0.0, 0.0, c, s, 0.0, -s, c])
    assert ab.ab_waves(len(frame), 1, 0) > 30
    _, want = check_bounded("random", frame, device, terms, index=index, **options)
    assert want.n_rays.sum() == BOUNDED_RAYS and int(ab.ab_chunks(want.buckets).sum()) >= (4 if not options["zones"] else 3)
    if not options["zones"]:
        assert want.buckets.tolist() == [[BOUNDED_RAYS]] and ab.ab_tiles(BOUNDED_RAYS) == 1   # (a last chunk of one ray)
