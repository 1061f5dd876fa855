"""The edges of the shared-reciprocal window (csrc/prt_math.hpp): prt_div3 divides three numerators by one refined
reciprocal only while every lane of the wave holds operands with 2^-380 <= |x| < 2^381, and falls back to the plain `/`
as a whole wave otherwise.  Both sides of that switch must give the same doubles, so operands are put on, just inside
and just outside the window here -- whole waves of them, waves that mix them lane by lane, and single lanes:

  (a) through ray directions scaled by 2^k (the tilt normalisation of the record row): scaling by a power of two is
      exact, so surfaces, positions and tilts are those of the unscaled rays bit for bit, and the frame is the C
      oracle's.  Only the high edge: from 2^-200 down every ray misses (the reference's absolute thresholds);
  (b) through the normals, low and high edge: the world-space normalisation of prt_world_normals (a surface scaled by
      2^k: the divisor is 2^-k in every lane, whole waves on one side of the window) and the object-space one of
      prt_primitive_normal (points scaled by 2^k lane by lane: the divisor is |p|, waves that mix);
  (c) zero numerators (v_div_fixup's case that can meet a divisor inside the window) on both paths.  An infinite or NaN
      numerator of a normalisation makes the divisor infinite or NaN as well, so it only ever meets the plain `/`.

Every k was checked on the CPU first: at k = 0, 200, 379..382, 400, 500 the numpy and the C oracle trace config2 to
the same frame (difference 0.0) with the counts of k = 0, and at every k of (b) the numpy oracle's normals are finite
unit vectors with the bits of the unscaled call; none had to be dropped.  (The C oracle has no entry point for normals:
their expectation is the numpy oracle and the invariance under the scale.)"""
import numpy as np
import pytest

import helpers
import scenes
from oracle import c_oracle
from oracle import prt_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LIMIT = 10
WAVE = 64


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to("cuda:0")


@pytest.fixture(scope="module")
def config2():
    """(snapshot, oracle scene, the first 256 rays) of the config2 scene at 1024 rays."""
    from pyrayt_amd.g3d.objects import CountedObject
    from pyrayt_amd.scene import SceneSnapshot

    CountedObject.reset_ids()
    parts, rays = scenes.SCENES["config2"](scenes.product_api(), 1024)
    snap = SceneSnapshot(parts)
    rays = np.ascontiguousarray(rays[:, :4 * WAVE])
    rays.setflags(write=False)
    return snap, helpers.flat_scene(snap), rays


def exponents(layout):
    """k of each of the 256 rays: waves of one k, waves that alternate two lane by lane, single lanes."""
    lanes = np.arange(WAVE)
    if layout == "edges":          # inside (380 is the last exponent of the window), outside, and a wave that falls back for half its lanes
        waves = [np.zeros(WAVE), np.full(WAVE, 380), np.full(WAVE, 381), np.where(lanes & 1, 381, 0)]
    elif layout == "one_lane":     # one lane far outside in an otherwise ordinary wave
        waves = [np.zeros(WAVE) for _ in range(4)]
        waves[1][37] = 500
    else:                          # "around": a direction's length is 1 to rounding, so 2^k |d| may sit one exponent lower
        waves = [np.full(WAVE, 379), np.full(WAVE, 382), np.where(lanes & 1, 381, 380), np.where(lanes % 3 == 0, 382, 0)]
    return np.concatenate(waves).astype(np.int64)


@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("layout", ["edges", "one_lane", "around"])
def test_directions_scaled_to_the_high_edge_of_the_window(config2, layout, flags):
    from pyrayt_amd.engine import DeviceScene

    snap, flat, plain = config2
    rays = plain.copy()
    rays[4:7] *= np.ldexp(1.0, exponents(layout))
    want, want_counts = c_oracle.trace(flat, rays, LIMIT)
    assert want_counts == [rays.shape[1]] * 3                      # nothing is lost to the scale: the counts of k = 0
    ds = DeviceScene(snap)
    rows, counts = ds.trace(dev(rays), LIMIT, flags=flags)
    got = rows.cpu().numpy().T
    unscaled, unscaled_counts = ds.trace(dev(plain), LIMIT, flags=flags)
    unscaled = unscaled.cpu().numpy().T
    ds.close()
    assert counts == want_counts == unscaled_counts
    helpers.assert_frames_identical(got, want, what=f"{layout} flags {flags} against the C oracle")
    # (no oracle needed for this one) a power of two changes no significand: same surfaces, positions and tilts
    helpers.assert_same_bits(got[:, 5:15], unscaled[:, 5:15], what=f"{layout} flags {flags} against the unscaled rays")


def test_zero_numerators_of_the_tilt_on_both_paths(config2):
    """Axis-parallel directions of length exactly 2^380 -- numerators +0 and -0 over a divisor on the last exponent of the
    window -- once in a wave that is otherwise inside the window (shared reciprocal) and once in a wave that a lane at
    2^382 sends to the plain division: their rows are there and are the C oracle's.  Beside them directions with an
    infinite, a NaN and only zero components: those rays hit nothing, in the oracle as on the device, so no infinite
    or NaN numerator reaches the tilt division."""
    from pyrayt_amd.engine import DeviceScene

    snap, flat, plain = config2
    rays = plain[:, :2 * WAVE].copy()
    axis_lanes = []
    for wave in (0, 1):
        at = wave * WAVE
        rays[4:7, at + 3] = (2.0 ** 380, 0.0, 0.0)
        rays[4:7, at + 19] = (2.0 ** 380, -0.0, 0.0)
        axis_lanes += [at + 3, at + 19]
        rays[4:7, at + 7] = (np.inf, 0.0, 0.0)
        rays[4:7, at + 11] = (1.0, np.inf, 0.0)
        rays[4:7, at + 13] = (1.0, np.nan, 0.0)
        rays[4:7, at + 17] = (0.0, 0.0, 0.0)
    rays[4:7, WAVE + 29] *= 2.0 ** 382
    want, want_counts = c_oracle.trace(flat, rays, LIMIT)
    for lane in axis_lanes:                                          # (not vacuous: the axis-parallel rays are recorded)
        first = want[(want[:, 4] == rays[12, lane]) & (want[:, 0] == 0)]
        assert first.shape[0] == 1 and np.array_equal(first[0, 12:15], (1.0, 0.0, 0.0)), lane
    ds = DeviceScene(snap)
    for flags in (0, 2):
        rows, counts = ds.trace(dev(rays), LIMIT, flags=flags)
        assert counts == want_counts, flags
        helpers.assert_frames_identical(rows.cpu().numpy().T, want, what=f"axis-parallel directions, flags {flags}")
    ds.close()


# ---------------------------------------------------------------------------------------------
# (b) the normals' normalisations
# ---------------------------------------------------------------------------------------------
NORMAL_EXPONENTS = (-400, -381, -380, -379, 379, 380, 381, 400)


def unit_surface(kind):
    """(oracle scene of one untransformed primitive, 128 points on it)."""
    fx = helpers.load("primitives.npz")
    scene = {k: np.array(v) for k, v in helpers.scene_of(fx, f"{kind}_identity__").items()}
    assert np.array_equal(scene["prim_minv"][0].reshape(4, 4), np.eye(4))
    rng = np.random.default_rng(2024)
    points = np.ones((4, 2 * WAVE))
    if kind == "sphere":
        direction = rng.normal(size=(3, 2 * WAVE))
        points[:3] = scene["prim_params"][0][0] * direction / np.linalg.norm(direction, axis=0)
        points[:3, 5] = (scene["prim_params"][0][0], 0.0, 0.0)                      # (zero numerators)
        points[:3, 9] = (0.0, -scene["prim_params"][0][0], -0.0)
    else:  # paraboloid x^2 + y^2 = 4 f z below its cap: normal along (x, y, -2 f)
        focus, height = scene["prim_params"][0][:2]
        reach = np.sqrt(4 * focus * height)
        points[:2] = rng.uniform(-0.6, 0.6, size=(2, 2 * WAVE)) * reach
        points[2] = (points[0] ** 2 + points[1] ** 2) / (4 * focus)
        points[:3, 5] = 0.0                                                        # (the vertex: normal (0, 0, -1))
    return scene, points


@pytest.fixture(scope="module")
def unscaled_normals():
    """Per kind: (scene, points, the device's normals, the numpy oracle's) of the unscaled surface, computed once."""
    out = {}
    for kind in ("sphere", "paraboloid"):
        scene, points = unit_surface(kind)
        ds = helpers.device_scene(scene)
        got = ds.world_normals(0, dev(points)).cpu().numpy()
        ds.close()
        want = prt_oracle.world_normals(scene, 0, points)
        helpers.assert_close_to_reference(got, want, what=f"{kind}: unscaled normals")
        for array in (points, got, want):
            array.setflags(write=False)
        out[kind] = (scene, points, got, want)
    return out


@pytest.mark.parametrize("k", NORMAL_EXPONENTS)
@pytest.mark.parametrize("kind", ["sphere", "paraboloid"])
def test_normals_of_a_surface_scaled_to_the_edges_of_the_window(unscaled_normals, kind, k):
    """The surface scaled uniformly by 2^k (its inverse transform by 2^-k) and the points with it: the object-space
    point is the unscaled one (and its normalisation in this entry point a plain `/`), the world-space normal has length
    2^-k before the div3 that normalises it -- in every lane, so each wave is wholly on one side of the window.  A unit
    vector does not change under a power-of-two scale of the scene: the bits of the unscaled call, which is inside."""
    scene, points, unscaled, _ = unscaled_normals[kind]
    scaled = {name: np.array(value) for name, value in scene.items()}
    scaled["prim_minv"][0] = np.diag([2.0 ** -k, 2.0 ** -k, 2.0 ** -k, 1.0]).reshape(-1)
    moved = points.copy()
    moved[:3] *= 2.0 ** k
    want = prt_oracle.world_normals(scaled, 0, moved)
    assert np.isfinite(want).all()
    ds = helpers.device_scene(scaled)
    got = ds.world_normals(0, dev(moved)).cpu().numpy()
    ds.close()
    helpers.assert_close_to_reference(got, want, what=f"{kind} scaled by 2^{k}")
    helpers.assert_same_bits(got, unscaled, what=f"{kind} scaled by 2^{k} against the unscaled surface")


def sphere_shape_and_points(unscaled_normals):
    from pyrayt_amd.g3d import shapes

    scene, points, _, _ = unscaled_normals["sphere"]
    return shapes.SphereShape(float(scene["prim_params"][0][0])), scene["prim_params"][0], points


@pytest.mark.parametrize("k", NORMAL_EXPONENTS)
def test_object_normals_at_points_scaled_lane_by_lane(unscaled_normals, k):
    """prt_primitive_normal (object_normal: its normalisation is a div3): a sphere's normal at p is p / |p| wherever p
    is, so points moved along their radius by 2^k put the divisor at 2^k -- in every lane of the first wave, in every
    other lane of the second, which falls back as a whole because of some of its lanes -- and leave the normal what it
    was, bit for bit."""
    shape, params, points = sphere_shape_and_points(unscaled_normals)
    lanes = np.arange(2 * WAVE)
    moved = points.copy()
    moved[:3] *= np.ldexp(1.0, np.where((lanes < WAVE) | (lanes & 1), k, 0))
    want = prt_oracle.object_normal(prt_oracle.SPHERE, params, moved)
    assert np.isfinite(want).all()
    unscaled = shape.normal(points)
    got = shape.normal(moved)
    helpers.assert_close_to_reference(got, want, what=f"points scaled by 2^{k}")
    helpers.assert_same_bits(got, unscaled, what=f"points scaled by 2^{k} against the unscaled points")


def test_zero_numerators_of_the_object_normal_on_both_paths(unscaled_normals):
    """Points on the axes of a sphere (numerators +0 and -0) among ordinary ones: the first wave is inside the window
    in every lane (shared reciprocal), the second holds the same points and one more at 2^382 times its radius, whose
    divisor is outside (plain division for the whole wave).  Lane for lane the two waves give the same doubles, and the
    axis points the exact unit vectors with the zeros' signs."""
    shape, params, points = sphere_shape_and_points(unscaled_normals)
    radius = float(params[0])
    wave = points[:, :WAVE].copy()
    wave[:3, 3] = (radius, 0.0, 0.0)
    wave[:3, 13] = (0.0, -radius, -0.0)
    wave[:3, 21] = (-0.0, 0.0, 32.0 * radius)
    moved = np.hstack((wave, wave))
    moved[:3, WAVE + 29] *= 2.0 ** 382
    want = prt_oracle.object_normal(prt_oracle.SPHERE, params, moved)
    got = shape.normal(moved)
    helpers.assert_close_to_reference(got, want, what="axis points")
    same = np.arange(WAVE) != 29
    helpers.assert_same_bits(got[:, :WAVE][:, same], got[:, WAVE:][:, same], what="shared reciprocal against the plain division")
    helpers.assert_same_bits(got[:, WAVE + 29], got[:, 29], what="the lane outside the window")
    exact = np.array([(1.0, 0.0, 0.0, 0.0), (0.0, -1.0, -0.0, 0.0), (-0.0, 0.0, 1.0, 0.0)]).T
    for at in (0, WAVE):
        helpers.assert_same_bits(got[:, [at + 3, at + 13, at + 21]], exact, what="axis points, zero signs included")


def test_world_normals_where_the_normal_is_not_finite(unscaled_normals):
    """What prt_world_normals writes where there is no normal: at the centre of a sphere (0 / 0) and at points with an
    infinite or a NaN coordinate all four components are NaN like the numpy oracle's -- the fourth too, which the
    reference zeroes before it normalises, so it is 0 / |n|.  (Every such wave takes the plain division: a NaN length
    is outside the window.)  Elsewhere the fourth component is 0."""
    scene, points, _, _ = unscaled_normals["sphere"]
    moved = points.copy()
    moved[:3, 3] = (0.0, 0.0, 0.0)
    moved[:3, 7] = (np.inf, 0.5, 0.0)
    moved[:3, 11] = (0.5, np.nan, 0.0)
    moved[:3, WAVE + 13] = (0.0, 0.0, -3.0)
    with np.errstate(all="ignore"):
        want = prt_oracle.world_normals(scene, 0, moved)
    assert np.isnan(want[:, [3, 7, 11]]).all() and np.isfinite(np.delete(want, [3, 7, 11], axis=1)).all()
    ds = helpers.device_scene(scene)
    got = ds.world_normals(0, dev(moved)).cpu().numpy()
    ds.close()
    helpers.assert_close_to_reference(got, want, what="points without a normal")
    assert np.array_equal(got[:, WAVE + 13], (0.0, 0.0, -1.0, 0.0))
