"""Bend a singlet on its wavefront: examples/bend_lens.py's lens, driven by the wavefront error instead of the spot.

A biconvex lens of radii 2 and 2 focuses a collimated beam onto a detector.  The variables are the lens's two radii of
curvature, each with its vertex kept so that the thickness does not change.  Each iteration traces once and asks
``trace_sensitivity(..., wavefront=True)`` for the wavefront of that trace -- the OPD against a sphere about the spot's
centroid on the detector -- and for its change per parameter on that sphere, held fixed (``dfield``); ``step(damping,
merit="wavefront")`` is the damped Gauss-Newton step that minimises the variance of the OPD.  Together the two radii set
the power, which brings the focus onto the detector (Z4, defocus), and the bending, which takes spherical aberration
(Z11) to its least.  ``dzernike()`` says which radius makes how much of which term.

The detector's own place is no variable here: against a fixed sphere a detector that moves changes nothing (only the
landing point slides along the ray); its effect comes in through the sphere's centre, which each iteration takes anew.

Central differences would need 2 K = 4 more traces and wavefronts per iteration, each behind a scene update.

usage: python examples/bend_lens_wavefront.py [--rays N] [--iterations I] [--damping D]   (needs an AMD GPU and the built library)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def world_radius(sphere):
    """The radius the sphere has in the world: its own radius times the scale its transform has taken on."""
    scale = np.linalg.norm(np.asarray(sphere.get_world_transform(), dtype=float)[:3, 0])
    return float(sphere.primitive.params[0]) * scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--damping", type=float, default=1e-3)
    args = ap.parse_args()
    thickness = 0.25
    lens = pyrayt.components.biconvex_lens(2, 2, thickness, aperture=1)
    rings = [pyrayt.components.CircleOfRays(diameter=d).move_x(-1) for d in (0.15, 0.3, 0.45, 0.6)]
    detector = pyrayt.components.baffle((1, 1)).move_x(2.0)
    front, back = lens.surface_ids[0][1], lens.surface_ids[1][1]  # (then the aperture stock)
    tracer = pyrayt.RayTracer(rings, [lens, detector], rays_per_source=max(1, args.rays // len(rings)))
    for iteration in range(args.iterations + 1):
        variables = [pyrayt.Deformation.radius(front, keep=(-thickness / 2, 0, 0)),
                     pyrayt.Deformation.radius(back, keep=(thickness / 2, 0, 0))]
        found = tracer.trace_sensitivity(detector, variables, weights=None, wavefront=True)  # (one group: the four rings)
        wave, change = found.wavefront, found.dzernike()[0]
        # a trust region on top of the damping: no radius changes by more than a quarter of itself in one step
        step = np.clip(found.step(args.damping, merit="wavefront")[0], -0.5, 0.5)
        print(f"iteration {iteration}: r1 {world_radius(front):.6f}, r2 {world_radius(back):.6f}, rms OPD {wave.rms[0]:.3e}, "
              f"Z4 {wave.zernike[0, 3]:+.3e}, Z11 {wave.zernike[0, 10]:+.3e}; dZ4/dr {np.array2string(change[:, 3], precision=3)}, "
              f"dZ11/dr {np.array2string(change[:, 10], precision=3)}"
              + (f", step {np.array2string(step, precision=4)}" if iteration < args.iterations else ""))
        if iteration < args.iterations:
            variables[0].apply(float(step[0]))
            variables[1].apply(float(step[1]))


if __name__ == "__main__":
    main()
