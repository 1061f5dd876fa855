"""tests/frame_sums_reference.py on the host: its copies of the headers' constants and partition rules, the integer and
the longdouble reference of the frame sums against each other, a float64 emulation of the device's partition inside the
derived bounds, the 2^53 precondition, and the longdouble wavefront against the float64 restatement of
tests/test_gpu_wavefront.py."""
import os

import numpy as np
import pytest

import frame_sums_reference as ref

IX = ref.IX


def grouped_dyadic_frame(n_rows, seed, rays_per_source):
    frame = ref.dyadic_frame(n_rows, seed)
    rng = np.random.default_rng(seed + 1)
    frame[:, IX["id"]] = np.arange(n_rows)
    frame[:, IX["surface"]] = rng.choice([3.0, 4.0], n_rows)
    frame[:, IX["generation"]] = np.sort(rng.integers(0, 3, n_rows))
    return frame, -(-n_rows // rays_per_source)


# ---- the copies of the headers ----------------------------------------------------------------------------------------
def test_the_named_constants_are_the_headers():
    found = ref.header_constants()
    for key, name in ref.HEADER_NAMES.items():
        assert found[key] == getattr(ref, name), key
    for name, lines in ref.HOST_RULES.items():
        text = open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", name)).read()
        for line in lines:
            assert line in text, (name, line)
    device = open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", "prt_device.hpp")).read()
    assert f"#define PRT_BLOCK {ref.BLOCK}" in device
    assert "enum { WF_LOC = 8," in open(os.path.join(ref.ROOT, "pyrayt_amd", "csrc", "prt_wavefront.hpp")).read()


def test_the_partition_rules_give_the_sizes_the_tests_are_built_on():
    assert ref.slot_switch_rows(1) == 261_121 and ref.slot_switch_rows(2) == 523_265
    for groups in (1, 2, 3):
        n = ref.slot_switch_rows(groups)
        assert ref.frame_slots(n, groups) == ref.FRAME_SLOTS and ref.frame_slots(n - 1, groups) == 1
    assert ref.wf_scan_per(524_288, 1) == 1 and ref.wf_scan_per(700_001, 1) == 2
    assert ref.wf_per_wave(2_097_152, 1) == 1024 and ref.wf_per_wave(2_250_000, 1) == 1152
    assert ref.wf_waves(300_000, 4096) == 256 and ref.wf_per_wave(300_000, 4096) == 1216
    # a workgroup of k_frame_zernike holds more than one tile only above 512 x 256 selected rows
    assert ref.wf_zblocks(10 ** 6, 1, 15, 256) == ref.WF_MAX_ZBLOCKS
    assert ref.wf_zshare(131_072, ref.WF_MAX_ZBLOCKS) == ref.WF_ZBLOCK < ref.wf_zshare(131_073, ref.WF_MAX_ZBLOCKS)
    assert ref.wf_zshare(140_000, ref.wf_zblocks(420_000, 1, 15, 256)) == 2 * ref.WF_ZBLOCK


# ---- integers against longdouble ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 65, 1025, 4 * 1024 + 1, 70_000])
def test_integer_and_longdouble_sums_agree_on_dyadic_frames(n_rows):
    frame, n_groups = grouped_dyadic_frame(n_rows, n_rows, 700)
    pivots = ref.dyadic_pivots(n_groups, 9)
    for surface, generation in ((None, None), (3.0, None), (None, 1.0), (4.0, 2.0)):
        for p in (None, pivots):
            want = ref.integer_reduce(frame, surface, generation, 700, n_groups, p)
            got = ref.reduce_reference(frame, surface, generation, 700, n_groups, p)
            assert np.array_equal(want, got.astype(np.float64))
            group = ref.selection(frame, surface, generation, 700, n_groups)
            for slots in (1, 64):  # (exact sums: the emulated partition gives the same bits too)
                assert np.array_equal(want, ref.emulate_reduce(frame, group, n_groups, p, slots))
        for quantity, about in (("y1", 0.25), ("axis_intercept", -0.75), ("intensity", 0.0)):
            want = ref.integer_mean_square(frame, quantity, about, surface, generation, 700, n_groups)
            got, _ = ref.mean_square_reference(frame, quantity, about, None, surface, generation, 700, n_groups)
            count, mean, mean_square = ref.mean_square_table(want)
            assert np.array_equal(count, got[:, 0].astype(np.int64))
            assert np.array_equal(mean, got[:, 1].astype(np.float64), equal_nan=True)
            assert np.array_equal(mean_square, got[:, 2].astype(np.float64), equal_nan=True)
    assert int(ref.integer_reduce(frame, None, None, 700, n_groups)[:, 0].sum()) == n_rows
    ids = frame[:, IX["id"]].astype(np.int64)
    assert np.array_equal(ref.selection(frame, None, None, 700, n_groups), ids // 700)


def test_the_precondition_fails_loudly():
    frame = ref.dyadic_frame(40, 1)
    frame[:, IX["y1"]] = 2.0 ** 21          # on the grid, but 40 squares of 2^52 units pass 2^53
    with pytest.raises(ref.NotExact, match="2\\^53"):
        ref.integer_reduce(frame)
    with pytest.raises(ref.NotExact, match="2\\^53"):
        ref.integer_mean_square(frame, "y1")
    frame = ref.dyadic_frame(40, 1)
    frame[3, IX["z1"]] = 0.3                # not on the grid
    with pytest.raises(ValueError, match="multiple"):
        ref.integer_reduce(frame)
    frame = ref.dyadic_frame(40, 1)
    frame[3, IX["y_tilt"]] = 0.25
    with pytest.raises(ValueError, match="y_tilt"):
        ref.integer_reduce(frame)
    assert issubclass(ref.NotExact, AssertionError)


# ---- the emulated partition inside the bound ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups,below,centre,width", [(1, True, (0.3, -0.2), 1.0), (1, False, (0.3, -0.2), 1.0),
                                                         (2, True, (0.3, -0.2), 1.0), (2, False, (1e3, -1e3), 1e-6)])
def test_the_emulated_partition_stays_inside_the_bound(n_groups, below, centre, width):
    n_rows = ref.slot_switch_rows(n_groups) - (1 if below else 0)
    frame, rays_per_source = ref.random_frame(n_rows, n_groups, 17 + n_groups, centre, width)
    want = ref.stats_reference(frame, None, None, rays_per_source, n_groups)
    slots = ref.frame_slots(n_rows, n_groups)
    assert slots == (1 if below else ref.FRAME_SLOTS)
    bound = ref.stats_bound(want, ref.reduce_depth(want.group, n_groups, slots))
    got = ref.emulate_stats(frame, None, None, rays_per_source, n_groups)
    deviation = np.abs(got - want.stats).astype(np.float64)
    assert np.array_equal(got[:, 0], want.stats[:, 0].astype(np.float64))
    assert np.all(deviation <= bound), (deviation / np.maximum(bound, 1e-300)).max()
    assert np.all(bound[:, 1:] > 0) and np.all(bound[:, 1:4] < 1e-9 * max(abs(centre[0]), 1.0))
    if width < 1e-3:  # (what the pivots are for: the spot's radius to 1e-10 of itself, 1e9 radii from the origin)
        assert np.all(bound[:, 3] < 1e-10 * want.stats[:, 3].astype(np.float64))


def test_reduce_depth_counts_the_flushes():
    group = np.full(3 * 1024, -1)
    group[:1024] = 0                       # one run in wave 0
    group[1024:1024 + 64] = [0, 1] * 32    # a slice with both groups: one flush each
    group[2048:2048 + 128] = 1
    group[2048 + 128:2048 + 192] = 0
    group[2048 + 192:2048 + 256] = 1       # group 1 is met again after a flush
    assert list(ref.reduce_depth(group, 2, 1)) == [16 + 6 + 3, 16 + 6 + 3]
    assert list(ref.reduce_depth(group, 2, 64)) == [16 + 6 + 1 + 64, 16 + 6 + 2 + 64]


def test_mean_square_of_the_sine_inside_its_bound():
    frame, rays_per_source = ref.random_frame(70_001, 3, 4)
    want, bound = ref.mean_square_reference(frame, "y_tilt", 0.17, "sin", None, None, rays_per_source, 3)
    group = ref.selection(frame, None, None, rays_per_source, 3)
    for g in range(3):
        v = np.sin(frame[group == g, IX["y_tilt"]]) - 0.17
        assert abs(v.mean() - want[g, 1]) <= bound[g, 1] and abs((v * v).mean() - want[g, 2]) <= bound[g, 2]
        assert 0 < bound[g, 2] < 1e-12


# ---- the wavefront reference ----------------------------------------------------------------------------------------------------
def test_the_recurrence_is_the_closed_form_and_its_bound_holds_in_float64():
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.random(4000)), rng.random(4000) * 2 * np.pi
    r[:3] = 0.0, 1.0, 1e-9    # (underflow is not modelled: fp64 would lose rho^2 below 1e-154)
    x, y = r * np.cos(t), r * np.sin(t)
    z = ref.zernike_recurrence(36, ref.Err(x), ref.Err(y))
    closed = ref.zernike_closed_form(36, x, y)
    float64 = ref.zernike_recurrence(36, ref.Fp64(x), ref.Fp64(y))
    worst = 0.0
    for j in range(36):
        assert np.abs(z[j].v - closed[:, j]).max() < 1e-15, j
        assert np.all(z[j].e < 1e-12) and float64[j].v.dtype == np.float64
        assert np.all(np.abs(float64[j].v - z[j].v) <= z[j].e), j
        worst = max(worst, float((np.abs(float64[j].v - z[j].v) / np.maximum(z[j].e, 1e-300)).max()))
    assert worst > 1e-3  # (the running bound is no wild overestimate)


@pytest.mark.parametrize("options", [dict(), dict(weights="intensity", terms=36),
                                     dict(rays_per_source=3000, n_groups=7, weights="intensity")])
def test_the_longdouble_wavefront_is_the_float64_restatement(options):
    import test_gpu_wavefront as base

    frame = ref.slab_frame(5000)
    assert np.array_equal(frame, base.synthetic_frame())
    terms, n_groups = options.get("terms", 15), options.get("n_groups", 1)
    wants, opl64 = base.wavefront_reference(frame, 5.0, **options)
    opl, opl_bound = ref.opl_reference(frame)
    assert np.all(np.abs(opl64 - opl[frame[:, IX["surface"]] == 5.0]) <= 4 * opl_bound[frame[:, IX["surface"]] == 5.0])
    group = ref.selection(frame, 5.0, None, options.get("rays_per_source"), n_groups)
    sphere = ref.sphere_bound(frame, group, n_groups, ref.wf_per_wave(len(frame), n_groups),
                              ref.wf_waves(len(frame), n_groups))
    got = ref.wavefront_reference(frame, opl.astype(np.float64), group, n_groups, sphere.p.astype(np.float64),
                                  sphere.radius.astype(np.float64), terms, options.get("weights"), len(frame), 256)
    scale = float(np.abs(opl).max())
    assert got.opd_bound.max() < 1e-13 * scale and got.pupil_bound.max() < 1e-13
    for g, want in enumerate(wants):
        if want is None:
            assert sphere.count[g] == 0
            continue
        assert np.allclose(sphere.p[g].astype(np.float64), want["p"], rtol=1e-13, atol=0)
        assert got.n_rays[g] == want["n_rays"] and got.n_missed[g] == want["n_missed"]
        m = got.group == g
        np.testing.assert_allclose(got.opd[m].astype(np.float64), want["opd"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(got.pupil[m].astype(np.float64), want["pupil"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got.sums[g].astype(np.float64), want["sums"], rtol=0,
                                   atol=1e-11 * np.abs(want["sums"]).max())
        assert np.all(got.sums_bound[g] < 1e-11 * np.abs(want["sums"]).max())
        assert abs(float(got.rms[g]) - want["rms"]) <= 1e-9 * want["rms"] and abs(float(got.pv[g]) - want["pv"]) <= 1e-12 * scale
        np.testing.assert_allclose(got.coef[g].astype(np.float64), want["coef"], rtol=0, atol=1e-8 * np.abs(want["coef"]).max())
        assert got.coef_bound[g] < 1e-9 * np.abs(want["coef"]).max()
