"""tests/aberration_sums_reference.py on the host: its copies of the headers' constants and partition rules, the integer
reference against the float64 restatement of tests/test_gpu_ray_aberrations.py on small dyadic frames (exact there), a
float64 emulation of the chunk / tile / fold order inside the derived bounds -- and outside them once the last chunk is
dropped."""
import os

import numpy as np
import pytest

import aberration_sums_reference as ab
import frame_sums_reference as ref

IX = ref.IX


# ---- the copies of the headers ----------------------------------------------------------------------------------------
def test_the_named_constants_are_the_headers():
    found = ab.header_constants()
    for key, name in ab.HEADER_NAMES.items():
        assert found[key] == getattr(ab, name), key
    for name, lines in ab.HOST_RULES.items():
        text = open(os.path.join(ab.ROOT, "pyrayt_amd", "csrc", name)).read()
        for line in lines:
            assert line in text, (name, line)
    assert f"#define PRT_BLOCK {ab.BLOCK}" in open(os.path.join(ab.ROOT, "pyrayt_amd", "csrc", "prt_device.hpp")).read()
    assert ab.MTF_CHUNK % ab.AB_BLOCK == 0 and ab.AB_BLOCK == 2 ** 8   # (what stage_depth counts: 16 + 8)
    assert ab.stage_depth(3) == 16 + 8 + 3 and ab.normal_depth(4096, 3) == 4099


def test_the_partition_rules_give_the_sizes_the_tests_are_built_on():
    waves, per_wave, all_waves, per = ab.ab_waves, ab.ab_per_wave, ab.ab_all_waves, ab.ab_scan_per
    for n in (1, 63, 64, 65, 1023, 1024):
        assert waves(n, 1, 0) == 1 and per_wave(n, 1, 0) == -(-n // 64) * 64 and per(n, 1, 0) == 1
    assert waves(1025, 1, 0) == 2 and per_wave(1025, 1, 0) == 576
    # scan per = 2, a ragged last wave
    n = ab.MTF_SCAN_BLOCK * ab.WF_ROWS_PER_WAVE + 1
    assert n == 524_289 and waves(n, 1, 0) == 513 and all_waves(n, 1, 0) == 516 and per(n, 1, 0) == 2
    assert per_wave(n, 1, 0) == 1024 and n % 1024 == 1 and per(n - 1, 1, 0) == 1
    # the wave cap
    n = ab.WF_MAX_WAVES * ab.WF_ROWS_PER_WAVE + 1
    assert n == 2_097_153 and waves(n, 1, 0) == 2048 and per_wave(n, 1, 0) == 1088 and per(n, 1, 0) == 4
    assert per_wave(n - 1, 1, 0) == 1024
    # the count cap cuts the waves
    assert ab.ab_buckets(64, 1024) == 65_536 and waves(200_000, 64, 1024) == 128 and waves(200_000, 1, 0) == 196
    assert per_wave(200_000, 64, 1024) == 1600 and ab.ab_bucket_scan_per(64, 1024) == 128
    # chunks and tiles
    assert [int(ab.ab_chunks(n)) for n in (0, 1, 4095, 4096, 4097, 8192, 8193)] == [0, 1, 1, 1, 2, 2, 3]
    assert [ab.ab_tiles(n) for n in (1, 255, 256, 257, 4095, 4096, 4097, 8193)] == [1, 1, 1, 2, 16, 16, 1, 1]


# ---- integers against the float64 restatement -------------------------------------------------------------------------------
def small_dyadic(n, seed):
    rng = np.random.default_rng(seed)
    ids = 100 + np.arange(n)
    frame = ab.dyadic_aberration_frame(ids[rng.random(n) < 0.9], ids, np.r_[ids, 100 + n + np.arange(5)], seed)
    last = np.flatnonzero(frame[:, 0] == 2)
    frame[last[::7], IX["surface"]] = 6.0
    if n >= 70:
        frame[last[3], IX["y1"]] = np.nan
        frame[last[4], IX["intensity"]] = -1.0
        frame[last[5], IX["intensity"]] = np.nan
    return frame


@pytest.mark.parametrize("n", [1, 70, 700, 5000])
@pytest.mark.parametrize("options", [
    dict(), dict(weights="intensity", reference="chief", zones=7), dict(pupil="direction", zones=0, pupil_radius=0.5),
    dict(weights="intensity", rays_per_source=300, n_groups=3, reference=(0.5, -0.25, 1.0), origin=(0.0, 0.5, -0.125),
         zones=1024, pupil_radius=4.0)])
def test_the_integer_reference_is_the_float64_restatement_on_dyadic_frames(n, options):
    import test_gpu_ray_aberrations as base

    frame = small_dyadic(n, n)
    options = dict(dict(surface=5.0, pupil_radius=2.0, reference=(0.25, 0.5, -0.5), zones=64), **options)
    n_groups = options.get("n_groups", 1)
    got = ab.integer_aberrations(frame, **options)
    wants = base.aberration_reference(frame, terms=1, **options)
    assert np.array_equal(got.rows, np.sort(np.concatenate([want["rows"] for want in wants])))
    assert np.array_equal(ab.join(frame), base.join_reference(frame))
    for g, want in enumerate(wants):
        assert got.n_rays[g] == want["n_rays"] and got.n_missed[g] == want["n_missed"]
        if not want["n_rays"]:
            assert got.chief[g] == -1
            continue
        mine = got.rays[got.group == g]
        assert got.chief[g] == want["chief"] and got.n_la[g] == want["n_la"]
        assert np.array_equal(got.centre[g], want["centre"])
        assert np.array_equal(mine[:, 0:2], want["p"]) and np.array_equal(mine[:, 2:4], want["eps"])
        assert np.array_equal(mine[:, 4:6], want["s"]) and np.array_equal(mine[:, 6], want["la"], equal_nan=True)
        assert np.array_equal(got.sums[g], want["sums"]) and np.array_equal(got.normal[g], want["normal"])
        assert np.array_equal(got.zones[g], want["zones"][:options["zones"]])
        assert got.buckets[g].sum() == want["n_rays"]
    assert got.n_missed.sum() >= (2 if n >= 70 else 0) and len(wants) == n_groups


def test_the_precondition_fails_loudly():
    frame = small_dyadic(500, 3)
    last = np.flatnonzero(frame[:, 0] == 2)
    off = frame.copy()
    off[last[10], IX["z1"]] = 0.3
    with pytest.raises(ValueError, match="multiple"):
        ab.integer_aberrations(off, surface=5.0)
    with pytest.raises(ValueError, match="power of two"):
        ab.integer_aberrations(frame, surface=5.0, pupil_radius=3.0)
    big = frame.copy()
    big[last, IX["intensity"]] = 2.0 ** 29     # an integer weight, but 400 terms w |eps|^2 of 2^48 units pass 2^53
    with pytest.raises(ref.NotExact, match="2\\^53"):
        ab.integer_aberrations(big, surface=5.0, weights="intensity")


# ---- the emulated partition inside the bound, and outside it without its last chunk -------------------------------------------
def emulate(frame, terms, drop_last_chunk=False, **options):
    """The pass in float64 on the emulated partition: centre, rho, the eight sums and the normal equations."""
    index = ab.join(frame)
    group = ref.selection(frame, options.get("surface"), None, None, 1)
    axes = ab.DEFAULT_AXES
    rows = np.flatnonzero(ab.used_rays(frame, index, group, "position", (0.0, 0.3, -0.2), axes, "intensity"))
    ray = ab.ray_chain(ab.Fp64, frame, rows, index[rows], "position", (0.0, 0.3, -0.2), axes, "intensity")
    bucket = np.zeros(len(rows), dtype=np.int64)
    wq = np.stack([ray.w.v] + [ray.w.v * ray.q[k].v for k in range(3)], 1)
    first = ab.emulate_chunk_sums(wq, bucket, 1)
    centre, rho = (first[1:4] / first[0])[None, :], np.array([ray.radius.v.max()])
    st = ab.stage_chain(ab.Fp64, ray, bucket, centre, rho, axes)
    sums = ab.emulate_chunk_sums(np.stack([t.v for t in st.terms], 1), bucket, 1, drop_last_chunk)
    z = ref.zernike_recurrence(terms, st.p1, st.p2)
    upper = np.triu_indices(terms)
    entries = [ray.w.v * z[i].v * z[j].v for i, j in zip(*upper)]
    entries += [ray.w.v * z[i].v * t.v for t in (st.e1, st.e2, ray.s1, ray.s2) for i in range(terms)]
    entries.append(ray.w.v * 1.0 * 1.0)
    per_ray = np.stack(entries, 1)
    chunks = [np.cumsum(per_ray[lo:lo + ab.MTF_CHUNK], axis=0)[-1] for lo in range(0, len(rows), ab.MTF_CHUNK)]
    normal = np.zeros(per_ray.shape[1])
    for chunk in (chunks[:-1] if drop_last_chunk else chunks):   # (each entry over a chunk's rays in series, then the fold)
        normal = normal + chunk
    return centre, rho, sums, normal


def test_the_emulated_partition_stays_inside_the_bound_and_a_dropped_chunk_does_not():
    n = 2 * ab.MTF_CHUNK + 1          # three chunks, the last of one ray
    frame = ab.random_aberration_frame(n, 11)
    options = dict(surface=5.0, origin=(0.0, 0.3, -0.2), weights="intensity", zones=0, terms=6)
    centre, rho, sums, normal = emulate(frame, 6, surface=5.0)
    want = ab.bounded_aberrations(frame, centre, rho, **options)
    assert want.n_rays[0] == n and int(ab.ab_chunks(n)) == 3 and ab.ab_tiles(n) == 1
    assert np.all(np.abs(centre - want.centre_ref) <= want.centre_bound) and np.all(want.centre_bound[0, 1:] > 0)
    assert np.all(np.abs(rho - want.rho_ref) <= want.rho_bound) and want.rho_bound[0] < 16 * ref.U * rho[0]
    deviation = np.abs(sums[0:8] - want.sums[0]).astype(np.float64)
    assert np.all(deviation <= want.sums_bound[0]), (deviation / want.sums_bound[0]).max()
    assert np.all(want.sums_bound[0] < ab.gamma(64) * np.abs(want.sums[0]).max())   # (about twice stage_depth(3) = 27)
    assert sums[8] == want.n_la[0] == n - len(range(0, n, 997))
    deviation = np.abs(normal - want.normal[0]).astype(np.float64)
    assert np.all(deviation <= want.normal_bound[0]), (deviation / want.normal_bound[0]).max()
    assert want.coef_bound[0].max() < 2.0 ** -20 * np.abs(want.coef[0]).max()   # (the bound says something: twenty bits)
    # one ray less in 8193: every sum with that ray's term leaves its bound
    _, _, short, short_normal = emulate(frame, 6, drop_last_chunk=True, surface=5.0)
    assert np.all(np.abs(short[0:8] - want.sums[0]).astype(np.float64)[[0, 5, 7]] > want.sums_bound[0][[0, 5, 7]])
    assert abs(short_normal[-1] - want.normal[0, -1]) > want.normal_bound[0, -1]
    assert abs(short_normal[0] - want.normal[0, 0]) > want.normal_bound[0, 0]


def test_the_running_bounds_hold_for_the_float64_chain():
    frame = ab.random_aberration_frame(3000, 5, n_other=300, id0=100_000)
    index = ab.join(frame)
    group = ref.selection(frame, 5.0, None, 34_000, 4)   # (ids from 100 000: groups 2 and 3)
    c, s = np.cos(0.3), np.sin(0.3)
    axes = np.array([c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0])
    for pupil in ("position", "direction"):
        rows = np.flatnonzero(ab.used_rays(frame, index, group, pupil, (0.0, 0.3, -0.2), axes, None))
        assert len(rows) == 3000 and set(group[rows]) == {2, 3}
        wide = ab.ray_chain(ab.Err, frame, rows, index[rows], pupil, (0.0, 0.3, -0.2), axes, None)
        narrow = ab.ray_chain(ab.Fp64, frame, rows, index[rows], pupil, (0.0, 0.3, -0.2), axes, None)
        centre, rho = np.tile((8.0, 0.05, -0.02), (4, 1)), np.full(4, 2.5)
        a, b = ab.stage_chain(ab.Err, wide, group[rows], centre, rho, axes), ab.stage_chain(ab.Fp64, narrow, group[rows], centre, rho, axes)
        for x, y in ((a.p1, b.p1), (a.e2, b.e2), (wide.s1, narrow.s1), (a.la, b.la), (a.terms[6], b.terms[6]), (a.terms[11], b.terms[11])):
            assert np.all(np.abs(y.v - x.v) <= x.e) and np.all(np.isfinite(x.e))
