"""prt_frame_optical_path and prt_frame_wavefront on the large-frame paths, against the longdouble reference and the
derived bounds of tests/frame_sums_reference.py (no fixed tolerance: every comparison is a bound from there).

The paths: a k_frame_zernike workgroup whose share is longer than one LDS tile (140 000 selected rows); the offset scan
with several waves a thread and a ragged last wave (700 001 rows); the cap of kWfMaxWaves waves, above which a wave's
run is no longer kWfRowsPerWave rows (2 250 000 rows); the slab cap that cuts the waves for many groups (4096 groups).
In each: the compacted rows are in the frame's row order over all groups, n_rays + n_missed is the selected count per
group, rows of groups past n_groups are absent.  And prt_frame_ray_aberrations, whose row passes share kWfMaxWaves:
the same rays give the same bits inside the 2 250 000-row frame."""
from types import SimpleNamespace

import numpy as np
import pytest

import frame_sums_reference as ref
from test_gpu_frame_partitions import note

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX
# the sizes follow from the constants of prt_wavefront.hpp, restated in frame_sums_reference.py
DENSE_RAYS = 140_000                                    # > kWfMaxZBlocks * kWfZBlock = 131 072 selected rows
SCAN_ROWS = 700_001                                     # > kWfRefBlock * kWfRowsPerWave = 524 288 rows: per = 2
CAP_ROWS = 2_250_000                                    # > kWfMaxWaves * kWfRowsPerWave = 2 097 152 rows
assert DENSE_RAYS > ref.WF_MAX_ZBLOCKS * ref.WF_ZBLOCK and SCAN_ROWS > ref.WF_REF_BLOCK * ref.WF_ROWS_PER_WAVE
assert CAP_ROWS > ref.WF_MAX_WAVES * ref.WF_ROWS_PER_WAVE and CAP_ROWS % 3 == 0
MANY_GROUPS, MANY_RPS, MANY_RAYS = 4096, 24, 100_008    # 2 * MANY_RAYS is a multiple of MANY_RPS
_CACHE = {}


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist()
    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)).to("cuda:0"), counts)


def cached(name, build):
    """(frame, DeviceFrame, the device's optical path on the host), built once."""
    if name not in _CACHE:
        frame = build()
        device = device_frame(frame)
        _CACHE[name] = (frame, device, device.optical_path().cpu().numpy())
    return _CACHE[name]


def sparse_places(n_rows, per_wave, seed):
    """About 6000 rows of the last generation: at the first and the last row of several waves' runs, in the last wave
    (the frame's last row among them), at random elsewhere -- and none in a stretch of twelve consecutive waves."""
    rng = np.random.default_rng(seed)
    start = 2 * -(-n_rows // 3)
    waves = -(-n_rows // per_wave)
    first_wave = start // per_wave + 1
    edges = [k * per_wave + d for k in (first_wave, first_wave + 1, first_wave + 40, waves - 2, waves - 1) for d in (-1, 0)]
    tail = [n_rows - 1, n_rows - 2, (waves - 1) * per_wave + 5]
    gap = ((first_wave + 60) * per_wave, (first_wave + 72) * per_wave)
    anywhere = rng.choice(np.arange(start, n_rows), 6000, replace=False)
    places = np.unique(np.concatenate([edges, tail, anywhere]))
    places = places[(places < gap[0]) | (places >= gap[1])]
    assert places.min() >= start and places.max() == n_rows - 1 and gap[1] < n_rows
    return places, gap


def sparse(n_rows):
    per_wave = ref.wf_per_wave(n_rows, 1)
    places, _ = sparse_places(n_rows, per_wave, n_rows % 97)
    return ref.sparse_frame(-(-n_rows // 3), places)[:n_rows]


def many_groups_frame():
    frame = ref.slab_frame(MANY_RAYS, 7, ids=np.arange(MANY_RAYS))
    last = frame[:, 0] == 2
    frame[last & (frame[:, IX["id"]] // MANY_RPS == 1000), IX["surface"]] = 6.0   # (group 1000 has no rows)
    return frame


def check(name, frame, device, opl, terms=15, weights=None, rays_per_source=None, n_groups=1, fit_groups=None):
    n_rows = len(frame)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = device.wavefront(5.0, zernike=terms, weights=weights, rays_per_source=rays_per_source, n_groups=n_groups)
    group = ref.selection(frame, 5.0, None, rays_per_source, n_groups)
    waves = -(-ref.wf_waves(n_rows, n_groups) // 4) * 4
    sphere = ref.sphere_bound(frame, group, n_groups, ref.wf_per_wave(n_rows, n_groups), waves)
    # n_rays + n_missed is the selected count per group; rows of groups past n_groups are absent
    assert np.array_equal(got.n_rays + got.n_missed, sphere.count)
    assert len(got.opd) == sphere.count.sum() == (group >= 0).sum()
    full = sphere.count > 0
    assert np.all(np.isnan(got.reference[~full])) and np.all(got.n_rays[~full] == 0)
    # pass 1: the reference sphere
    ratio = note(f"{name} reference point", np.abs(got.reference[full] - sphere.p[full]).astype(np.float64), sphere.p_bound[full])
    assert np.all(ratio <= 1.0)
    ratio = note(f"{name} radius", np.abs(got.radius[full] - sphere.radius[full]).astype(np.float64), sphere.r_bound[full])
    assert np.all(ratio <= 1.0)
    # pass 2 and the sums, from the device's sphere and optical paths
    want = ref.wavefront_reference(frame, opl, group, n_groups, got.reference, got.radius, terms, weights, n_rows, cus,
                                   fit_groups)
    assert np.array_equal(got.n_rays, want.n_rays) and np.array_equal(got.n_missed, want.n_missed)
    opd, pupil = got.opd.cpu().numpy(), got.pupil.cpu().numpy()
    # (the rows in the frame's row order over all groups: the reference's rows are, and every row is compared)
    assert np.array_equal(np.isnan(opd), ~want.hit) and np.array_equal(np.isnan(pupil), ~np.stack([want.hit] * 2, 1))
    hit = want.hit
    ratio = note(f"{name} opd", np.abs(opd[hit] - want.opd[hit]).astype(np.float64), want.opd_bound[hit])
    assert np.all(ratio <= 1.0), (ratio.max(), np.argmax(ratio))
    ratio = note(f"{name} pupil", np.abs(pupil[hit] - want.pupil[hit]).astype(np.float64), want.pupil_bound[hit])
    assert np.all(ratio <= 1.0), (ratio.max(), np.argmax(ratio))
    ratio = note(f"{name} normal", np.abs(got.normal - want.sums).astype(np.float64), want.sums_bound)
    assert np.all(ratio <= 1.0), (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    seen = want.n_rays > 0
    ratio = note(f"{name} rms", np.abs(got.rms[seen] - want.rms[seen]).astype(np.float64), want.rms_bound[seen])
    assert np.all(ratio <= 1.0), ratio.max()
    ratio = note(f"{name} pv", np.abs(got.pv[seen] - want.pv[seen]).astype(np.float64), want.pv_bound[seen])
    assert np.all(ratio <= 1.0), ratio.max()
    assert want.coef
    for g, coef in want.coef.items():
        assert got.rank[g] == terms
        ratio = note(f"{name} zernike", np.abs(got.zernike[g] - coef).astype(np.float64), np.full(terms, want.coef_bound[g]))
        assert np.all(ratio <= 1.0), (g, ratio.max(), want.condition[g])
        assert want.coef_bound[g] < 1e-9 * np.abs(coef).max()   # (the bound says something)
    return got, want


def check_optical_path(name, frame, opl):
    want, bound = ref.opl_reference(frame)
    ratio = note(f"{name} optical path", np.abs(opl - want).astype(np.float64), bound)
    assert np.all(ratio <= 1.0), (ratio.max(), np.argmax(ratio))


# ---- a workgroup's share of the Zernike sums longer than one tile ---------------------------------------------------------------
@pytest.mark.parametrize("terms,weights", [(15, None), (36, "intensity")])
def test_dense_selection_beyond_one_tile_a_workgroup(terms, weights):
    frame, device, opl = cached("dense", lambda: ref.slab_frame(DENSE_RAYS))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ref.wf_zshare(DENSE_RAYS, ref.wf_zblocks(len(frame), 1, terms, cus)) > ref.WF_ZBLOCK
    if weights is None:
        check_optical_path("dense", frame, opl)
    got, _ = check("dense", frame, device, opl, terms=terms, weights=weights)
    assert got.n_rays[0] == DENSE_RAYS


# ---- the scan with several waves a thread ---------------------------------------------------------------------------------------
def test_sparse_selection_scanned_two_waves_a_thread():
    frame, device, opl = cached("scan", lambda: sparse(SCAN_ROWS))
    assert len(frame) == SCAN_ROWS and ref.wf_scan_per(SCAN_ROWS, 1) == 2 and ref.wf_per_wave(SCAN_ROWS, 1) == ref.WF_ROWS_PER_WAVE
    assert SCAN_ROWS % ref.WF_ROWS_PER_WAVE and frame[-1, IX["surface"]] == 5.0   # (a ragged last wave, its last row selected)
    check_optical_path("scan", frame, opl)
    got, want = check("scan", frame, device, opl, weights="intensity")
    places, gap = sparse_places(SCAN_ROWS, ref.WF_ROWS_PER_WAVE, SCAN_ROWS % 97)
    assert np.array_equal(want.rows, places) and not np.any((places >= gap[0]) & (places < gap[1]))
    check("scan", frame, device, opl, rays_per_source=100_000, n_groups=2)      # (the third group's rows are absent)


# ---- the wave cap -----------------------------------------------------------------------------------------------------------------
def test_sparse_selection_above_the_wave_cap():
    frame, device, opl = cached("cap", lambda: sparse(CAP_ROWS))
    per_wave = ref.wf_per_wave(CAP_ROWS, 1)
    assert ref.wf_waves(CAP_ROWS, 1) == ref.WF_MAX_WAVES and per_wave > ref.WF_ROWS_PER_WAVE and per_wave % 64 == 0
    selected = np.flatnonzero(frame[:, IX["surface"]] == 5.0)
    edges = selected[(selected % per_wave == 0) | (selected % per_wave == per_wave - 1)]
    assert len(edges) >= 8 and len(selected) < 6100
    check_optical_path("cap", frame, opl)   # (the whole 2.25M-row frame)
    check("cap", frame, device, opl, weights="intensity")
    # three groups whose boundaries fall inside a wave; then two, so that the third group's rows are absent
    rays_per_source = CAP_ROWS // 9
    assert (2 * CAP_ROWS // 3 + rays_per_source) % per_wave and (2 * CAP_ROWS // 3 + 2 * rays_per_source) % per_wave
    got, _ = check("cap", frame, device, opl, terms=21, rays_per_source=rays_per_source, n_groups=3)
    assert np.all(got.n_rays > 1000)
    fewer, _ = check("cap", frame, device, opl, rays_per_source=rays_per_source, n_groups=2)
    assert np.array_equal(fewer.n_rays, got.n_rays[:2])


# ---- the slab cap for many groups -----------------------------------------------------------------------------------------------------
def test_many_groups_cut_the_waves():
    frame, device, opl = cached("many", many_groups_frame)
    n_rows = len(frame)
    per_wave = ref.wf_per_wave(n_rows, MANY_GROUPS)
    assert ref.wf_waves(n_rows, MANY_GROUPS) == ref.WF_SLAB_BYTES // (MANY_GROUPS * ref.WF_LOC * 8) < ref.wf_waves(n_rows, 1)
    assert per_wave > ref.WF_ROWS_PER_WAVE
    start = 2 * MANY_RAYS
    boundaries = np.arange(-(-start // per_wave) * per_wave, start + MANY_GROUPS * MANY_RPS, per_wave)
    straddling = sorted({int((b - start) // MANY_RPS) for b in boundaries if (b - start) % MANY_RPS})
    sample = sorted({0, MANY_GROUPS - 1, 1000, *straddling})
    assert 40 < len(straddling) and len(sample) <= 64 and MANY_RAYS > MANY_GROUPS * MANY_RPS
    got, want = check("many groups", frame, device, opl, terms=6, weights="intensity", rays_per_source=MANY_RPS,
                      n_groups=MANY_GROUPS, fit_groups=sample)
    assert got.n_rays[1000] == 0 and got.n_missed[1000] == 0 and np.isnan(got.rms[1000])
    assert sorted(want.coef) == [g for g in sample if g != 1000]
    assert np.all(np.delete(got.n_rays + got.n_missed, 1000) == MANY_RPS)


# ---- ray aberrations: the same rays inside a frame above the wave cap ---------------------------------------------------------------
def test_ray_aberrations_do_not_depend_on_the_rows_around():
    import test_gpu_ray_aberrations as aberrations

    frame, device, _ = cached("cap", lambda: sparse(CAP_ROWS))
    ids = frame[frame[:, IX["surface"]] == 5.0, IX["id"]]
    inside = np.flatnonzero(np.isin(frame[:, IX["id"]], ids))    # (the selected rays' rows of all three generations)
    thin = device_frame(frame[inside])
    assert 3000 < len(ids) and len(inside) == 3 * len(ids)
    for options in (dict(), dict(rays_per_source=CAP_ROWS // 9, weights="intensity", reference="chief", zones=9)):
        small, big = thin.ray_aberrations(5.0, **options), device.ray_aberrations(5.0, **options)
        # row numbers are the only thing that may differ: the big frame's are taken back to the thin frame's
        where = torch.from_numpy(inside).to("cuda:0")
        rows = torch.searchsorted(where, big.rows)
        assert torch.equal(where[rows], big.rows)
        record = big.record.copy()
        chief = record[:, 7] >= 0
        record[chief, 7] = np.searchsorted(inside, record[chief, 7].astype(np.int64))
        mapped = SimpleNamespace(record=record, normal=big.normal, zones=big.zones, coefficients=big.coefficients,
                                 rank=big.rank, rows=rows, rays=big.rays)
        aberrations.same(small, mapped)
        assert small.record[:, 4].sum() == len(ids)
