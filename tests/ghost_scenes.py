"""The scenes of the ghost tests and their reference runs: the C oracle traces, tests/fresnel_reference.py gives the
transmittance, tests/ghost_reference.py spawns the children, round after round."""
import numpy as np

import fresnel_reference
import ghost_reference
import helpers
import scenes

HOUSING = 30.0


def api():
    import pyrayt_amd as pyrayt

    pyrayt.g3d.objects.CountedObject.reset_ids()  # (the same surface ids whenever a scene is built)
    return scenes.product_api()


def housed(parts, housing=True):
    from pyrayt_amd import ghosts

    return list(parts) + ([ghosts.housing(HOUSING)] if housing else [])


def lens(n, housing=True):
    """Config 2 -- a biconvex lens, a detector, a 6 degree cone of n rays -- inside the housing: (parts, rays, detector)."""
    parts, rays = scenes.config2(api(), n)
    return housed(parts, housing), rays, parts[-1]


def stopped_lens(n, housing=True):
    parts, rays = scenes.stopped_lens(api(), n)
    return housed(parts, housing), rays, parts[-1]


def prism(n_per_wavelength, wavelengths=(0.45, 0.55, 0.633, 0.7)):
    """An equilateral prism of a dispersive glass in the housing, a fan of rays per wavelength."""
    a = api()
    body = a.components.equilateral_prism(1, 1, material=a.materials.glass["SF2"]).move_x(0.25)
    det = a.components.baffle((3, 3)).move_x(3.0)
    blocks = []
    for k, wavelength in enumerate(wavelengths):
        rays = scenes.cone_rays(n_per_wavelength, (-1.5, 0.0, 0.0), 4.0, 40 + k, wavelength=wavelength)
        blocks.append(rays)
    rays = np.hstack(blocks)
    rays[12] = np.arange(rays.shape[1])
    return housed([body, det]), rays, det


def plate(thickness, theta, n=1.5, rays=1):
    """A plane-parallel plate of index n normal to x, a detector behind it, `rays` rays at theta to the normal in the
    xy plane (the same ray, at z apart), in the housing: (parts, rays, detector)."""
    a = api()
    half = (thickness / 2, 2.0, 2.0)
    slab = a.cg.Cuboid(tuple(-h for h in half), half, material=a.materials.BasicRefractor(n))
    det = a.components.baffle((8, 8)).move_x(3.0)
    set_ = scenes.blank_rays(rays)
    set_[0], set_[2] = -1.0, 0.01 * np.arange(rays)
    set_[4], set_[5] = np.cos(theta), np.sin(theta)
    return housed([slab, det]), set_, det


def flat(parts):
    from pyrayt_amd.scene import SceneSnapshot

    return helpers.flat_scene(SceneSnapshot(parts))


def refracting(parts):
    from pyrayt_amd import ghosts

    return ghosts.refracting_surfaces(parts)


def reference_orders(parts, rays, order, surfaces=None, rays_per_group=None, n_groups=1, limit=10, min_intensity=0.0,
                     ray_offset=1e-6, **fresnel_options):
    """The reference's rounds: a list, per order k = 0 .. of dict(ghosts (None at 0), frame, fresnel); an order without
    children ends it.  Children start unpolarised."""
    from oracle import c_oracle

    scene = flat(parts)
    surfaces = refracting(parts) if surfaces is None else surfaces
    frame, _ = c_oracle.trace(scene, rays, limit, ray_offset)
    out = [dict(ghosts=None, frame=frame, fresnel=fresnel_reference.fresnel(frame, **fresnel_options))]
    fresnel_options.pop("polarization", None)
    for _ in range(order):
        children = ghost_reference.ghosts(out[-1]["frame"], out[-1]["fresnel"]["transmittance"], surfaces,
                                          rays_per_group=rays_per_group, n_groups=n_groups, min_intensity=min_intensity,
                                          ray_offset=ray_offset)
        if not children["rays"].shape[1]:
            out.append(dict(ghosts=children, frame=np.zeros((0, 15)), fresnel=None))
            break
        frame, _ = c_oracle.trace(scene, children["rays"], limit, ray_offset)
        out.append(dict(ghosts=children, frame=frame, fresnel=fresnel_reference.fresnel(frame, **fresnel_options)))
        rays_per_group, n_groups = children["stride"], children["n_groups"]
    return out


def path(orders, order, group):
    """(surfaces, first reflection first; source) of a group of an order of reference_orders."""
    surfaces = []
    for k in range(order, 0, -1):
        group, surface = (int(v) for v in orders[k]["ghosts"]["keys"][group])
        surfaces.append(surface)
    return tuple(reversed(surfaces)), group
