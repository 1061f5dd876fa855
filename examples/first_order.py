"""First-order properties of a singlet from ONE trace: focal length, distortion over the field and chromatic focal shift.

A biconvex BK7 lens stands before a detector near its focal plane.  Three collimated sources (rings of parallel rays) come
in at the field angles 0, 2 and 4 degrees.  The parameters are not parts of the system but the rays themselves:

  ``SourceMotion.of_source(i, rotate=(0, 0, 1))``   the field angle of source i, in radians: d(centroid)/d(angle) is the
                                                     effective focal length at that field point (an image at f tan(theta)
                                                     moves by f / cos(theta)^2: what departs from that is distortion),
  ``WavelengthChange()``                             the wavelength of every ray, in micrometres: d(centroid)/d(lambda) is
                                                     lateral colour, ``focus_gradient()`` the chromatic focal shift.

``trace_sensitivity`` pushes the tangents of all four through the trace it has just made.  Beside each figure stands the
central difference of two more traces with the source turned, or its wavelength shifted, by hand: 2 K = 8 re-traces.

usage: python examples/first_order.py [--rays N]   (needs an AMD GPU and the built library)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402

ANGLES = (0.0, 2.0, 4.0)


def best_focus(rows):
    """The shift along x that minimises the mean square radius about the centroid, rays continued as straight lines."""
    p = rows[:, 10:12]
    s = rows[:, 13:15] / rows[:, 12:13]
    pc, sc = p - p.mean(axis=0), s - s.mean(axis=0)
    return -np.sum(pc * sc) / np.sum(sc * sc)


def landing(tracer, det, n):
    """Per source: the centroid (y, z) on the detector and the best-focus shift, from a trace's host frame."""
    frame = tracer.trace_device().to_numpy()
    rows = frame[frame[:, 5] == det.get_id()]
    groups = [rows[(rows[:, 4] // n) == g] for g in range(len(ANGLES))]
    return np.array([g[:, 10:12].mean(axis=0) for g in groups]), np.array([best_focus(g) for g in groups])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000)
    args = ap.parse_args()
    n = args.rays
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1, material=pyrayt.materials.glass["BK7"])
    det = pyrayt.components.baffle((2, 2)).move_x(1.9)
    sources = [pyrayt.components.CircleOfRays(diameter=0.5, wavelength=0.55).move_x(-1.5).rotate_z(a) for a in ANGLES]
    tracer = pyrayt.RayTracer(sources, [lens, det], rays_per_source=n)
    fields = [pyrayt.SourceMotion.of_source(i, rotate=(0, 0, 1)) for i in range(len(ANGLES))]
    sens = tracer.trace_sensitivity(det, fields + [pyrayt.WavelengthChange()], weights=None, rays_per_source=True)
    colour = len(fields)
    chromatic = sens.focus_gradient()[:, colour]
    lateral = sens.centroid_gradient[:, colour, 1]

    # the same by hand: each source turned by +-h, then every wavelength shifted by +-h
    # (0.01 degrees and no less: a beam within 1e-5 of an axis is taken for parallel to it by the primitives' isclose tests)
    h_angle, h_colour = 1e-2, 1e-4
    by_hand_focal, by_hand_shift, by_hand_lateral = [], None, None
    for i, source in enumerate(sources):
        source.rotate_z(h_angle)
        plus = landing(tracer, det, n)[0][i, 0]
        source.rotate_z(-2 * h_angle)
        minus = landing(tracer, det, n)[0][i, 0]
        source.rotate_z(h_angle)
        by_hand_focal.append((plus - minus) / (2 * np.radians(h_angle)))
    for sign in (1, -1):
        for source in sources:
            source.wavelength = 0.55 + sign * h_colour
        centre, focus = landing(tracer, det, n)
        by_hand_shift = focus if sign == 1 else (by_hand_shift - focus) / (2 * h_colour)
        by_hand_lateral = centre[:, 0] if sign == 1 else (by_hand_lateral - centre[:, 0]) / (2 * h_colour)
    for source in sources:
        source.wavelength = 0.55

    on_axis = sens.effective_focal_length(0)[0]  # (source 0 is collimated along x: d(centroid)/d(angle) is f)
    print(f"{n} rays a source, one trace and K = {sens.n_parameters} tangents; by hand: {2 * sens.n_parameters} re-traces")
    print(f"effective focal length {on_axis:.8f} about the real rays, a ring of radius 0.25 (the paraxial thick-lens "
          f"formula at BK7's index for 0.55 um: {1 / ((1.5185 - 1) * (1 / 2 + 1 / 2 - (1.5185 - 1) * 0.25 / (1.5185 * 4))):.4f})")
    print("field   d(y)/d(angle)    by hand       f / cos^2      distortion   d(focus)/d(um)   by hand      d(y)/d(um)    by hand")
    for i, angle in enumerate(ANGLES):
        focal = sens.centroid_gradient[i, i, 1]
        law = on_axis / np.cos(np.radians(angle)) ** 2
        print(f"{angle:4.1f}  {focal:14.8f} {by_hand_focal[i]:14.8f} {law:14.8f} {100 * (focal / law - 1):11.4f} %"
              f" {chromatic[i]:14.8f} {by_hand_shift[i]:14.8f} {lateral[i]:13.8f} {by_hand_lateral[i]:13.8f}")


if __name__ == "__main__":
    main()
