"""The wave-level shortcut of the hit phase that skips arithmetic no lane needs: a bare plane leaf
computes its crossing first and its slabs only where some lane's crossing can win (scene option `no_plane_bound`
switches it off).  It may not change a bit of a row: every scene here is traced with it on and with it off and
compared as uint64, then against the oracles; the path counter says that it fires where config 2 is expected to
take it.  Small ray sets: a partial wave, one tile, four tiles with a partial last.  (The scenes also cover what the
"sphere left behind" experiment of the interval chains needed -- waves that mix rays approaching and leaving a lens --:
tools/experiments/sphere_left_behind.patch ran this file with its option as well.)"""
import numpy as np
import pytest

import helpers
import scenes
from oracle import c_oracle
from oracle import prt_oracle as orc
from pyrayt_amd import engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OFF = {"no_plane_bound": 1}
LIMIT = 10


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to("cuda:0")


def _config2(api, n):
    return scenes.config2(api, n)


def _plane_first(api, n):
    """the detector listed in front of the lens: the plane runs with best_t = inf and nothing may be skipped"""
    (lens, baffle), rays = scenes.config2(api, n)
    return [baffle, lens], rays


def _two_baffles(api, n):
    """two detectors in one place: equal t, the earlier component keeps the hit"""
    (lens, baffle), rays = scenes.config2(api, n)
    return [lens, baffle, api.components.baffle((1, 1)).move_x(1)], rays


def _small_baffle(api, n):
    """a detector smaller than the collimated beam (radius ~0.21): the slabs decide within a wave"""
    (lens, _), rays = scenes.config2(api, n)
    return [lens, api.components.baffle((0.2, 0.2)).move_x(1), api.components.baffle((2, 2)).move_x(3)], rays


def _config3(api, n):
    return scenes.config3(api, n)


def _mirror_behind(api, n):
    """a mirror behind the lens and every second ray started between the two: a wave holds rays that approach a
    sphere of the lens and rays that leave it, in every generation"""
    (lens, _), rays = scenes.config2(api, n)
    mirror = api.components.plane_mirror(0.2, aperture=(2.0, 2.0)).move_x(1.5)
    catcher = api.components.baffle((4, 4)).move_x(-4)
    rays[0, 1::2] = 0.6
    return [lens, mirror, catcher], rays


def _parallel_to_plane(api, n):
    """every third ray runs along y: parallel to the detector, some of them inside its plane (x = 1)"""
    parts, rays = scenes.config2(api, n)
    rays[4:7, ::3] = np.array([[0.0], [1.0], [0.0]])
    rays[0, ::6] = 1.0
    rays[1, ::6] = -0.3
    return parts, rays


def _zero_direction(api, n):
    parts, rays = scenes.config2(api, n)
    rays[4:7, ::4] = 0.0
    return parts, rays


def _short_direction(api, n):
    parts, rays = scenes.config2(api, n)
    rays[4:7, ::3] *= 1e-3
    return parts, rays


def _origin_w(api, n):
    parts, rays = scenes.config2(api, n)
    rays[3, ::5] = 2.0
    return parts, rays


CASES = {
    "config2_70": (_config2, 70), "config2_256": (_config2, 256), "config2_1000": (_config2, 1000),
    "plane_first": (_plane_first, 256), "two_baffles": (_two_baffles, 256), "small_baffle": (_small_baffle, 256),
    "config3": (_config3, 256), "mirror_behind": (_mirror_behind, 256), "parallel_to_plane": (_parallel_to_plane, 256),
    "zero_direction": (_zero_direction, 256), "short_direction": (_short_direction, 256), "origin_w": (_origin_w, 256),
}
_TRACED = {}


def traced(name):
    """(snapshot, rays, frame with the shortcut (R, 15), counts, frame without, counts): traced once per case,
    read-only, shared by the tests below"""
    if name not in _TRACED:
        from pyrayt_amd.g3d.objects import CountedObject
        from pyrayt_amd.scene import SceneSnapshot

        build, n = CASES[name]
        CountedObject.reset_ids()
        parts, rays = build(scenes.product_api(), n)
        snap = SceneSnapshot(parts)
        frames = []
        for options in (None, OFF):
            ds = engine.DeviceScene(snap, options=options)
            rows, counts = ds.trace(dev(rays), LIMIT)
            frame = rows.cpu().numpy().T.copy()
            frame.setflags(write=False)
            frames.append((frame, list(counts)))
            ds.close()
        rays.setflags(write=False)
        _TRACED[name] = (snap, rays, frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    return _TRACED[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_are_the_same_bits_with_and_without_the_shortcut(name):
    snap, rays, on, on_counts, off, off_counts = traced(name)
    print(name, "rows per generation:", on_counts)
    assert on_counts == off_counts
    assert on.shape == off.shape and on.shape[0] > 0
    assert np.array_equal(np.ascontiguousarray(on).view(np.uint64), np.ascontiguousarray(off).view(np.uint64)), \
        f"{name}: {int((np.ascontiguousarray(on).view(np.uint64) != np.ascontiguousarray(off).view(np.uint64)).sum())} elements differ"


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_match_the_oracles(name):
    """The comparison of test_gpu_parity.py::test_trace_matches_oracle: the C oracle's frame in every bit, the numpy
    oracle's to 1e-12."""
    snap, rays, on, on_counts, off, off_counts = traced(name)
    flat = helpers.flat_scene(snap)
    want, want_counts = orc.trace(flat, np.array(rays), LIMIT)
    assert on_counts == list(want_counts)
    exact, exact_counts = c_oracle.trace(flat, np.array(rays), LIMIT)
    assert on_counts == list(exact_counts)
    helpers.assert_frames_identical(on, exact, what=f"{name} against the C oracle")
    helpers.assert_close_to_reference(on, want, what=f"{name} against the numpy oracle")


@pytest.mark.skipif(bool(engine.DEFAULT_OPTIONS) or bool(engine.DEFAULT_TRACE_FLAGS), reason="the expected counts are those of the default path")
def test_the_shortcut_fires_where_config2_leaves_work_behind():
    """256 rays = 4 waves.  Generations 0 and 1 find the lens nearer than the detector in every lane: the plane leaf is
    not finished, 4 waves x 2 generations; generation 2 needs it.  With the option set nothing counts."""
    from pyrayt_amd.g3d.objects import CountedObject
    from pyrayt_amd.scene import SceneSnapshot

    CountedObject.reset_ids()
    parts, rays = scenes.config2(scenes.product_api(), 256)
    snap = SceneSnapshot(parts)
    for options, want in ((None, 8), (OFF, 0)):
        ds = engine.DeviceScene(snap, options=options)
        rows, counts = ds.trace(dev(rays), LIMIT, flags=engine.TRACE_COUNT_PATHS)
        tele = ds.telemetry()
        print(options, list(counts), tele["plane_leaves_not_finished"])
        assert [c for c in counts if c] == [256, 256, 256]
        assert tele["plane_leaves_not_finished"] == want, options
        helpers.assert_frames_identical(rows.cpu().numpy().T, traced("config2_256")[2], what=f"counted trace, {options}")
        ds.close()
