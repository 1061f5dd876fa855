"""Bring a decentred lens back with the sensitivities of one trace per iteration.

A biconvex lens collimates a point source onto a detector.  The lens is knocked off its axis in y and z.  Each iteration
traces once, asks ``trace_sensitivity`` for d(landing point)/d(parameter) of the two decentres and takes ``step()``: the
Gauss-Newton step that minimises the mean square radius of the beam about the point where the centred system puts it.
The collimated beam keeps its own radius about that point, so the iteration contracts linearly, by a factor of about
ten a step; four iterations bring the lens back to a few parts in 10^4 of where it started.

Central differences would need 2 K = 4 more traces per iteration for the same gradient, with a step size to choose and
its truncation and rounding noise; the count beside each iteration is what the same iterations cost that way.

A tilt of this lens is left out on purpose: the spot of a collimated beam behind a symmetric lens does not tell a tilt
from a decentre to first order, and the mean square radius about a fixed point is then no alignment merit (it falls
when the tilt defocuses the beam).  Aligning a tilt wants a merit that sees it, such as several field points.

usage: python examples/align_lens.py [--rays N]   (needs an AMD GPU and the built library)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=4)
    args = ap.parse_args()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    source = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-1.959)
    detector = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(source, [lens, detector], rays_per_source=args.rays)
    nominal = tracer.trace_device().group_stats(surface=detector.get_id())  # (where the centred system puts the spot)
    target = (1.0, float(nominal["y"][0]), float(nominal["z"][0]))
    # knock the lens off
    lens.move(0.0, 2e-3, -1e-3)
    traces = 0
    for iteration in range(args.iterations):
        motions = [pyrayt.Motion(lens, translate=(0, 1, 0)), pyrayt.Motion(lens, translate=(0, 0, 1))]
        found = tracer.trace_sensitivity(detector, motions, reference=target)
        traces += 1
        step = found.step()[0]
        position = np.asarray(lens.get_position(), dtype=float).reshape(-1)[1:3]
        print(f"iteration {iteration}: lens at y, z = {np.array2string(position, precision=3)}, rms radius about the "
              f"target {np.sqrt(found.mean_square[0]):.9f}, step {np.array2string(step, precision=3)}; {traces} trace(s) "
              f"so far, with central differences {traces * (1 + 2 * len(motions))}")
        lens.move(0.0, float(step[0]), float(step[1]))
    position = np.asarray(lens.get_position(), dtype=float).reshape(-1)[1:3]
    print(f"after {args.iterations} iterations the lens is at y, z = {np.array2string(position, precision=3)}")


if __name__ == "__main__":
    main()
