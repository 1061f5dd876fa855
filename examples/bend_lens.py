"""Bend a singlet: the lens-design notebook's optimisation in miniature, with the sensitivities of one trace per iteration.

A biconvex lens of radii 2 and 2 focuses a collimated beam onto a detector.  The variables are the lens's two radii of
curvature, each with its vertex kept so that the thickness does not change, and the detector's place along the axis.
Each iteration traces once, asks ``trace_sensitivity`` for d(landing point)/d(parameter) of the three -- two
``Deformation.radius`` and a ``Motion`` -- and takes ``step(damping)``: the damped Gauss-Newton step that minimises the
mean square radius of the spot.  ``Deformation.apply`` and ``move_x`` carry the step out.  The spot shrinks as the lens
bends towards the shape of least spherical aberration and the detector follows the focus; bending and power are nearly
the same thing to the rays of one field point, which is what the damping is for.

A radius is measured in the sphere's own frame: after ``apply`` the sphere keeps its ``params`` and its transform carries
the change, so the radii printed are read off the transforms.

Central differences would need 2 K = 6 more traces per iteration, each behind a scene update, for the same gradient.

usage: python examples/bend_lens.py [--rays N] [--iterations I] [--damping D]   (needs an AMD GPU and the built library)"""
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
                     pyrayt.Deformation.radius(back, keep=(thickness / 2, 0, 0)),
                     pyrayt.Motion(detector, translate=(1, 0, 0))]
        found = tracer.trace_sensitivity(detector, variables, weights=None)  # (one group: the four rings together)
        # a trust region on top of the damping: no radius changes by more than a quarter of itself in one step
        step = np.clip(found.step(args.damping)[0], -0.5, 0.5)
        place = float(np.asarray(detector.get_position(), dtype=float).reshape(-1)[0])
        print(f"iteration {iteration}: r1 {world_radius(front):.6f}, r2 {world_radius(back):.6f}, detector at x = {place:.6f}, "
              f"rms spot radius {np.sqrt(found.mean_square[0]):.9f}"
              + (f", step {np.array2string(step, precision=4)}" if iteration < args.iterations else ""))
        if iteration < args.iterations:
            variables[0].apply(float(step[0]))
            variables[1].apply(float(step[1]))
            detector.move_x(float(step[2]))


if __name__ == "__main__":
    main()
