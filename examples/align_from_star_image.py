"""Find a lens's decentre from a star image, with the PSF sensitivities of one trace per iteration.

examples/align_lens.py brings a decentred lens back by its spot; near the diffraction limit the spot says little and what
one has is a picture of a star.  Here a singlet images a point at twice its focal length.  The lens is decentred by a
small amount the loop is not told (``--decentre``: by default the image moves by about half a pixel, an eighth of the Airy
radius; an image moved by more than that radius is outside what a first-order step can see), ``psf()`` of that system is
kept as the "measurement", and the lens is put back.  Each iteration then traces the system as it is believed to be, asks
``psf_gradient()`` for
d(image)/d(decentre along y and z) on the measurement's own grid -- the reference sphere (its centre P and radius R) and the
pixels are those of the nominal system throughout, as a detector's are --, and takes ``step(damping, target=measured)``:
the Gauss-Newton step on ``measured - image`` over the pixels.  The lens of the model is moved by it; what has been moved
in all is the estimate of the decentre.

Central differences would need 2 K = 4 more traces, wavefronts and Huygens sums per iteration for the same gradient.

usage: python examples/align_from_star_image.py [--rays N] [--iterations I] [--damping D] [--decentre DY DZ] [--pixels N]
(needs an AMD GPU and the built library)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402

UNIT = 1000.0  # (world units are millimetres)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20_000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--damping", type=float, default=0.0)
    ap.add_argument("--decentre", type=float, nargs=2, default=[5e-4, -2.5e-4])
    ap.add_argument("--pixels", type=int, default=32)
    args = ap.parse_args()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    # twelve cones from one point fill the pupil (one cone is a ring of rays, whose image is J0^2: side lobes as bright
    # as the core's shoulder, and a least-squares fit of one such image to another has minima between them)
    cones = [pyrayt.components.ConeOfRays(cone_angle=float(a)).move_x(-4.08) for a in np.linspace(0.25, 3.0, 12)]
    detector = pyrayt.components.baffle((1, 1)).move_x(4.2)
    system = [lens, detector]
    tracer = pyrayt.RayTracer(cones, system, rays_per_source=max(1, args.rays // len(cones)))

    # the nominal system fixes the reference sphere and the pixel grid
    nominal = tracer.trace_device().psf(detector, world_unit_um=UNIT, pixels=args.pixels)
    sphere = dict(reference=nominal.wavefront.reference, radius=nominal.wavefront.radius)
    grid = dict(world_unit_um=UNIT, pixels=args.pixels, pixel_size=nominal.pixel_size)
    print(f"nominal: Strehl {nominal.strehl[0]:.4f}, f/{nominal.f_number[0]:.1f}, pixel {nominal.pixel_size[0]:.3e}")

    # the "measurement": the same system with the lens decentred, seen on the same grid
    dy, dz = args.decentre
    lens.move_y(dy).move_z(dz)
    measured = tracer.trace_device().psf(detector, **grid, **sphere)
    lens.move_y(-dy).move_z(-dz)
    print(f"measured (lens decentred by ({dy:+.3e}, {dz:+.3e})): Strehl {measured.strehl[0]:.4f}, "
          f"peak at ({measured.peak_uv[0, 0]:+.3e}, {measured.peak_uv[0, 1]:+.3e})")

    found = np.zeros(2)
    for iteration in range(args.iterations):
        variables = [pyrayt.Motion(lens, translate=(0, 1, 0)), pyrayt.Motion(lens, translate=(0, 0, 1))]
        frame = tracer.trace_device()
        wave = frame.wavefront(detector, weights="intensity", **sphere)
        sens = frame.sensitivity(detector, variables, system, wavefront=wave)
        gradient = sens.psf_gradient(**grid)
        residual = float(np.sqrt(np.mean((measured.image - gradient.image) ** 2)))
        step = gradient.step(args.damping, target=measured)[0]
        print(f"iteration {iteration}: estimate ({found[0]:+.6e}, {found[1]:+.6e}), rms residual of the image {residual:.3e}, "
              f"Strehl {gradient.strehl[0]:.4f}, d(Strehl)/d(y, z) ({gradient.dstrehl[0, 0]:+.3e}, {gradient.dstrehl[0, 1]:+.3e}), "
              f"step ({step[0]:+.3e}, {step[1]:+.3e})")
        lens.move_y(float(step[0])).move_z(float(step[1]))
        found += step
    print(f"decentre found ({found[0]:+.6e}, {found[1]:+.6e}), given ({dy:+.6e}, {dz:+.6e}), "
          f"error ({found[0] - dy:+.2e}, {found[1] - dz:+.2e})")


if __name__ == "__main__":
    main()
