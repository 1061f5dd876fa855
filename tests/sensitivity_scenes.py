"""Scenes for the sensitivity tests, traced on the CPU by the C oracle: each gives the parts, the frame (R, 15), the
surface to look at and the Motion parameters.  Built through pyrayt_amd's own scene objects, so the snapshot the tests
hand to ``sensitivity`` is the one the scene compiler takes."""
from types import SimpleNamespace

import numpy as np

import helpers
import scenes
from oracle import c_oracle

_CACHE = {}


def trace(parts, rays, limit=10):
    from pyrayt_amd.scene import SceneSnapshot

    frame, counts = c_oracle.trace(helpers.flat_scene(SceneSnapshot(parts)), rays, limit)
    return frame, counts


def directed_rays(origins, directions, wavelength=0.633):
    origins, directions = np.atleast_2d(origins).astype(float), np.atleast_2d(directions).astype(float)
    rays = scenes.blank_rays(len(origins), wavelength)
    rays[0:3] = origins.T
    rays[4:7] = (directions / np.linalg.norm(directions, axis=1, keepdims=True)).T
    return rays


def _case(name, parts, rays, surface, motions, limit=10, **more):
    frame, counts = trace(parts, rays, limit)
    return SimpleNamespace(name=name, parts=parts, rays=rays, frame=frame, counts=counts, surface=surface,
                           motions=motions, limit=limit, **more)


def build(name, n=257):
    """The case ``name`` with n rays (cached: a frame is computed once and shared, never changed)."""
    key = (name, n)
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[name](n)
    return _CACHE[key]


def _api():
    from pyrayt_amd import Motion

    api = scenes.product_api()
    return api, api.cg, api.components, api.materials, Motion


def detector_shift(n):
    """A cone onto a detector plane that is translated: dx = d (n.v) / (n.d)."""
    api, cg, c, matl, Motion = _api()
    det = c.baffle((4, 4)).move_x(1.0).rotate_z(12)
    v = (0.3, 0.2, -0.1)
    return _case("detector_shift", [det], scenes.cone_rays(n, (-1.0, 0.05, 0.0), 20.0, 5), det, [Motion(det, translate=v)],
                 velocity=np.array(v))


def plane_slide(n):
    """A detector slid within its own plane, and turned about its own normal: dx = 0."""
    api, cg, c, matl, Motion = _api()
    det = c.baffle((4, 4)).move_x(1.0)
    motions = [Motion(det, translate=(0.0, 0.3, -0.2)), Motion(det, rotate=(0.5, 0.0, 0.0), pivot=(1.0, 0.2, 0.1))]
    return _case("plane_slide", [det], scenes.cone_rays(n, (-1.0, 0.0, 0.0), 20.0, 6), det, motions, invariant=True)


def sphere_spin(n):
    """A glass ball turned about its own centre, in front of a detector: dx = 0 on every row."""
    api, cg, c, matl, Motion = _api()
    ball = cg.Sphere(0.8, material=matl.glass["BK7"]).move(0.3, 0.1, -0.05)
    det = c.baffle((6, 6)).move_x(4.0)
    motions = [Motion(ball, rotate=(0.3, -0.7, 0.5))]  # (pivot: the ball's position, its centre)
    return _case("sphere_spin", [ball, det], scenes.cone_rays(n, (-2.0, 0.0, 0.0), 12.0, 7), det, motions, invariant=True)


def cylinder_spin(n):
    """A mirror cylinder turned about its own axis: dx = 0 on every row (wall and caps alike)."""
    api, cg, c, matl, Motion = _api()
    rod = cg.Cylinder(0.5, -1.5, 1.5, material=matl.mirror).rotate_x(90).move(0.0, 0.0, 0.2)
    det = c.baffle((12, 12)).move_x(-3.0)
    axis = np.asarray(rod.get_orientation(), dtype=float).reshape(-1)[:3]
    motions = [Motion(rod, rotate=tuple(0.8 * axis))]
    return _case("cylinder_spin", [rod, det], scenes.cone_rays(n, (-2.0, 0.1, 0.0), 8.0, 8), det, motions, invariant=True)


def flat_mirror(n):
    """A flat mirror turned about an axis in its plane through each ray's own hit point, one parameter a ray:
    dd' = 2 w x d'."""
    api, cg, c, matl, Motion = _api()
    n = min(n, 6)
    mirror = cg.XYPlane(6, 6, material=matl.mirror).rotate_y(-90).move_x(3).rotate_z(20)
    det = c.baffle((40, 40)).move_x(-6.0)
    rays = scenes.cone_rays(n, (0.0, 0.0, 0.0), 10.0, 9)
    frame, _ = trace([mirror, det], rays)
    hits = frame[frame[:, 0] == 0][:, 9:12]
    normal = np.asarray(mirror.get_orientation(), dtype=float).reshape(-1)[:3]
    axes = []
    for k in range(n):
        other = np.cross(normal, [0.3 + 0.1 * k, 1.0, -0.4])
        axes.append(0.7 * other / np.linalg.norm(other))
    motions = [Motion(mirror, rotate=tuple(axes[k]), pivot=tuple(hits[k])) for k in range(n)]
    return _case("flat_mirror", [mirror, det], rays, det, motions, axes=np.array(axes))


def config2(n):
    """The config-2 lens (a 6 degree cone from the focus, aperture 1) and its detector: lens decentre in y, lens tilt about
    z, detector shift in x."""
    api, cg, c, matl, Motion = _api()
    parts, rays = scenes.config2(api, n)
    lens, det = parts
    motions = [Motion(lens, translate=(0, 1, 0)), Motion(lens, rotate=(0, 0, 1)), Motion(det, translate=(1, 0, 0))]
    return _case("config2", parts, rays, det, motions)


def two_mirrors(n):
    """scene_two_mirrors' parts: two facing plane mirrors, a slightly tilted beam, ten generations; the far mirror is
    tilted and pushed, the near one tilted."""
    api, cg, c, matl, Motion = _api()
    parts, _ = scenes.two_mirrors(api, 4)
    first, second = parts
    rays = scenes.cone_rays(n, (0.0, 0.0, 0.0), 3.0, 11)
    motions = [Motion(first, rotate=(0, 0, 1)), Motion(first, translate=(1, 0, 0)), Motion(second, rotate=(0, 1, 0))]
    return _case("two_mirrors", parts, rays, first, motions, limit=6)


def stopped(n):
    """A stop that absorbs part of the beam in mid-path (rays end early, their id slots go stale), a lens, a detector."""
    api, cg, c, matl, Motion = _api()
    parts, rays = scenes.stopped_lens(api, n)
    stop, lens, det = parts
    motions = [Motion(lens, translate=(0, 0, 1)), Motion(lens, rotate=(0, 1, 0)), Motion(stop, translate=(1, 0, 0))]
    return _case("stopped", parts, rays, det, motions)


def prism(n):
    """An equilateral prism entered through one face at an angle that puts the next face in total internal reflection."""
    api, cg, c, matl, Motion = _api()
    glass = c.equilateral_prism(1, 1).move_x(0.25)
    det = c.baffle((30, 30)).rotate_y(90).move(0.25, 0, -4.0)
    rng = np.random.default_rng(12)
    origins = np.column_stack([np.full(n, -1.5), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.3, -0.1, n)])
    directions = np.column_stack([np.ones(n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n)])
    motions = [Motion(glass, rotate=(0, 1, 0)), Motion(glass, translate=(0, 0, 1)), Motion(glass, rotate=(1, 0, 0))]
    return _case("prism", [glass, det], directed_rays(origins, directions, 0.5), det, motions)


def scaled(n):
    """A part that is not rigid in the snapshot: a glass ball stretched to an ellipsoid."""
    api, cg, c, matl, Motion = _api()
    egg = cg.Sphere(0.7, material=matl.glass["BK7"]).scale(1.0, 1.6, 0.8).rotate_z(25).move(0.2, 0.1, 0.0)
    det = c.baffle((8, 8)).move_x(3.5)
    motions = [Motion(egg, translate=(0, 1, 0)), Motion(egg, rotate=(0, 0, 1)), Motion(egg, rotate=(0.2, 1, 0), pivot=(0, 0, 0))]
    return _case("scaled", [egg, det], scenes.cone_rays(n, (-2.0, 0.0, 0.0), 8.0, 13), det, motions)


def scaled_cylinder(n):
    """A mirror cylinder squeezed to an elliptic one (a non-rigid minv under the wall's Hessian), met on its wall."""
    api, cg, c, matl, Motion = _api()
    rod = cg.Cylinder(0.5, -1.5, 1.5, material=matl.mirror).scale(1.4, 0.7, 1.0).rotate_x(90).rotate_z(15).move(0.0, 0.0, 0.2)
    det = c.baffle((12, 12)).move_x(-3.0)
    motions = [Motion(rod, translate=(1, 0, 0)), Motion(rod, rotate=(0, 1, 0)), Motion(rod, rotate=(0.3, 0, 1), pivot=(0.5, 0, 0))]
    return _case("scaled_cylinder", [rod, det], scenes.cone_rays(n, (-2.0, 0.1, 0.0), 8.0, 14), det, motions)


def paraboloid(n):
    """A parabolic mirror (the paraboloid's wall: its own Hessian and gradient length) that sends a cone to a detector."""
    api, cg, c, matl, Motion = _api()
    dish = c.parabolic_mirror(3.0, 0.5, aperture=1.5)
    det = c.baffle((8, 8)).move_x(4.0)
    motions = [Motion(dish, translate=(0, 1, 0)), Motion(dish, rotate=(0, 0, 1)), Motion(dish, translate=(1, 0, 0))]
    return _case("paraboloid", [dish, det], scenes.cone_rays(n, (3.0, 0.1, 0.05), 8.0, 15) * np.array(
        [1, 1, 1, 1, -1, 1, 1, 1, 1, 1, 1, 1, 1])[:, None], det, motions)


_BUILDERS = {f.__name__: f for f in (scaled_cylinder, paraboloid, detector_shift, plane_slide, sphere_spin, cylinder_spin, flat_mirror, config2,
                                     two_mirrors, stopped, prism, scaled)}
CLOSED_FORMS = ("detector_shift", "plane_slide", "sphere_spin", "cylinder_spin", "flat_mirror")
SYSTEMS = ("config2", "two_mirrors", "stopped", "prism", "scaled", "scaled_cylinder", "paraboloid")
