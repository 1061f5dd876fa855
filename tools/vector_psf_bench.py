#!/usr/bin/env python3
"""The polarised diffraction PSF of the frame on the device (DeviceFrame.psf(fresnel=)), timed with device events after
warm-up against the scalar psf() of the same frame in the same session, on BASELINE config 2 at --rays rays
(3 generations, one wavelength, every detector row meets the reference sphere), at 64^2 and 128^2 pixels:

  psf              DeviceFrame.psf(det): the scalar Huygens sum, end to end (wavefront, sort, sum, fold, read-back)
  vector_psf_1     psf(det, fresnel=F) with F from polarised input: one state
  vector_psf_2     psf(det, fresnel=F) with F from unpolarised input: two states
  fresnel_fields   the pass that makes F: DeviceFrame.fresnel(fields=True, coatings=...)
  trace_psf        RayTracer.trace_psf(det, fresnel=...), 128^2: trace, Fresnel pass and vector PSF under one record plan

Prints one JSON line per figure, with ratio_per_state = (vector - wavefront) / states / (scalar - wavefront) of the
whole calls.  usage: tools/vector_psf_bench.py [--rays N] [--steps K]
(run under rocprofv3 --kernel-trace --stats for per-kernel times: k_vpsf_huygens against k_psf_huygens, told apart by
their grids: pixel tiles x ray slices x buckets)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd.materials import Coating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    coatings = {lens: Coating.quarter_wave(1.38, float(frame["wavelength"][0]))}
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation)}
    polarised = frame.fresnel(polarization=(0, 1, 1j), coatings=coatings, fields=True)
    unpolarised = frame.fresnel(coatings=coatings, fields=True)
    ms = device_ms(lambda: frame.fresnel(polarization=(0, 1, 1j), coatings=coatings, fields=True), args.steps)
    print(json.dumps({**common, "what": "fresnel_fields", "ms": ms}), flush=True)
    wavefront = device_ms(lambda: frame.wavefront(det, weights="intensity"), args.steps)
    print(json.dumps({**common, "what": "wavefront", "ms": wavefront}), flush=True)
    for pixels in (64, 128):
        scalar = device_ms(lambda: frame.psf(det, world_unit_um=1000.0, pixels=pixels), args.steps)
        got = frame.psf(det, world_unit_um=1000.0, pixels=pixels)
        terms = float(got.n_rays.sum()) * pixels * pixels
        print(json.dumps({**common, "what": "psf", "pixels": pixels, "ms": scalar, "terms_per_s": terms / scalar * 1e3,
                          "strehl": float(got.strehl[0])}), flush=True)
        for states, fresnel in ((1, polarised), (2, unpolarised)):
            ms = device_ms(lambda: frame.psf(det, world_unit_um=1000.0, pixels=pixels, fresnel=fresnel), args.steps)
            got = frame.psf(det, world_unit_um=1000.0, pixels=pixels, fresnel=fresnel)
            print(json.dumps({**common, "what": f"vector_psf_{states}", "pixels": pixels, "states": states, "ms": ms,
                              "terms_per_s": states * terms / ms * 1e3,
                              "ratio_per_state": (ms - wavefront) / states / (scalar - wavefront),
                              "strehl": float(got.strehl[0]), "strehl_apodized": float(got.strehl_apodized[0]),
                              "throughput": float(got.throughput[0])}), flush=True)
    ms = device_ms(lambda: tracer.trace_psf(det, world_unit_um=1000.0, fresnel=dict(polarization=(0, 1, 1j), coatings=coatings)),
                   max(2, args.steps // 2))
    print(json.dumps({**common, "what": "trace_psf", "pixels": 128, "states": 1, "ms": ms}), flush=True)


if __name__ == "__main__":
    main()
