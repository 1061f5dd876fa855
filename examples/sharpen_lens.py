"""Sharpen a singlet: bend it for the MTF at one frequency, with the MTF sensitivities of one trace per iteration.

examples/bend_lens.py bends the same lens for the smallest RMS spot; a lens specification is more often written against
the contrast at a frequency.  The variables are the same three -- the two radii of curvature, each with its vertex kept,
and the detector's place along the axis.  Each iteration traces once, asks ``trace_mtf_gradient`` for
d(MTF)/d(parameter) at half, once and one and a half times ``--frequency`` cycles per unit, tangential and sagittal, and
takes ``step(damping)``: the damped Gauss-Newton step on the residuals ``1 - MTF``.  ``Deformation.apply`` and ``move_x``
carry it out.  The contrast rises as the detector finds the focus and the lens bends towards the shape of least spherical
aberration; the first step that lowers the mean MTF is taken back and the loop stops.

The MTF is not a sum of squares of the landing points: where it is low (a badly defocused start) its gradient says little
and the spot's is the better guide, and at its maximum the Jacobian of ``1 - MTF`` vanishes, so Gauss-Newton gains most of
what there is in two or three steps from a fair start and then has no more to say.  ``dmtf_dfocus`` comes with the
same pass: it is the detector's gradient a second time, from the through-focus derivative instead of a ``Motion``.

Central differences would need 2 K = 6 more traces and 6 more ``mtf()`` calls per iteration for the same gradient.

usage: python examples/sharpen_lens.py [--rays N] [--iterations I] [--damping D] [--frequency NU]
(needs an AMD GPU and the built library)"""
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
    ap.add_argument("--damping", type=float, default=1e-2)
    ap.add_argument("--frequency", type=float, default=20.0)
    args = ap.parse_args()
    thickness = 0.25
    lens = pyrayt.components.biconvex_lens(2, 2, thickness, aperture=1)
    rings = [pyrayt.components.CircleOfRays(diameter=d).move_x(-1) for d in (0.15, 0.3, 0.45, 0.6)]
    detector = pyrayt.components.baffle((1, 1)).move_x(1.95)
    front, back = lens.surface_ids[0][1], lens.surface_ids[1][1]  # (then the aperture stock)
    tracer = pyrayt.RayTracer(rings, [lens, detector], rays_per_source=max(1, args.rays // len(rings)))
    frequencies = [args.frequency / 2, args.frequency, 1.5 * args.frequency]
    damping, best, last, taken = args.damping, -1.0, None, None
    for iteration in range(args.iterations + 1):
        variables = [pyrayt.Deformation.radius(front, keep=(-thickness / 2, 0, 0)),
                     pyrayt.Deformation.radius(back, keep=(thickness / 2, 0, 0)),
                     pyrayt.Motion(detector, translate=(1, 0, 0))]
        # the centre follows the centroid: with a fixed centre the OTF is taken on the plane through that centre, and a
        # detector that slides along its normal would change nothing
        found = tracer.trace_mtf_gradient(detector, variables, frequencies, azimuths=(0.0, 90.0), reference="centroid",
                                          weights=None)
        merit = float(found.mtf[0, 0].mean())
        place = float(np.asarray(detector.get_position(), dtype=float).reshape(-1)[0])
        print(f"iteration {iteration}: r1 {world_radius(front):.6f}, r2 {world_radius(back):.6f}, detector at x = {place:.6f}, "
              f"MTF at {args.frequency:g} cycles: tangential {found.mtf[0, 0, 0, 1]:.6f}, sagittal {found.mtf[0, 0, 1, 1]:.6f}, "
              f"mean over {len(frequencies)} frequencies {merit:.6f}, d(MTF)/d(focus) {found.dmtf_dfocus[0, 0, 0, 1]:+.4f}")
        if merit < best and last is not None:
            # the step made it worse: take it back with the objects that made it (``apply`` is linear in its amount, so
            # the radii come back to second order in the step) and stop -- at the MTF's maximum the Jacobian of 1 - MTF
            # vanishes and Gauss-Newton has no more to say
            taken[0].apply(-last[0])
            taken[1].apply(-last[1])
            detector.move_x(-last[2])
            print(f"  lower than {best:.6f}: step taken back; r1 {world_radius(front):.6f}, r2 {world_radius(back):.6f}, "
                  f"detector at x = {place - last[2]:.6f}")
            break
        best = merit
        if iteration < args.iterations:
            # a trust region on top of the damping: no variable changes by more than 0.1 in one step
            last = [float(v) for v in np.clip(found.step(damping)[0], -0.1, 0.1)]
            print(f"  step {np.array2string(np.array(last), precision=4)}, damping {damping:g}")
            taken = variables
            variables[0].apply(last[0])
            variables[1].apply(last[1])
            detector.move_x(last[2])


if __name__ == "__main__":
    main()
