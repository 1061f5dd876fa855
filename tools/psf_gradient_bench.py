#!/usr/bin/env python3
"""PSF sensitivities of the frame on the device (Sensitivity.psf_gradient, the entry point prt_frame_psf_gradient), timed
after warm-up on config 2's lens at --rays rays (3 generations), for K = 1, 6 and 16 parameters (--K to choose), at 64^2
and 128^2 pixels (--pixels to choose), in the manner of tools/vector_psf_bench.py and tools/mtf_gradient_bench.py:

  sensitivity   DeviceFrame.sensitivity(..., wavefront=w) with K design parameters: what psf_gradient needs first
  psf_gradient  Sensitivity.psf_gradient on that result, end to end (the passes and the read-back of the outputs)
  psf           DeviceFrame.psf on the same grid: the evaluate-only pass whose sum kernel k_psfg_huygens extends
  retrace       one trace_device() of the same rays: what a central difference pays twice a parameter, beside 2 psf()
  differences   2 K x (retrace + psf), from the two figures above: the cost of the same derivatives by central
                differences (a system changed between traces also recompiles its scene, which is not counted)

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms
(default 300 ms); each figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one
JSON line per figure.  --once runs every call once after a warm-up, for a kernel trace (rocprofv3 --kernel-trace --stats
-- python tools/psf_gradient_bench.py --once) that sets k_psfg_huygens beside k_psf_huygens on the same rays.
usage: tools/psf_gradient_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16] [--pixels 64 128] [--once]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402
from mtf_gradient_bench import parameters_of  # noqa: E402
from sensitivity_bench import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 6, 16])
    ap.add_argument("--pixels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation), "window_ms": args.window_ms, "repeats": args.repeats}

    def timed(fn):
        if args.once:
            fn()
            fn()
            torch.cuda.synchronize()
            return {"ms": float("nan")}
        return windows(fn, args.repeats, args.window_ms)

    retrace = timed(lambda: (tracer.trace_device(), torch.cuda.synchronize()))
    print(json.dumps({**common, "what": "retrace", **retrace}), flush=True)
    wave = frame.wavefront(det, weights="intensity")
    plain = {}
    for side in args.pixels:
        plain[side] = timed(lambda: frame.psf(det, world_unit_um=1000.0, pixels=side))
        print(json.dumps({**common, "what": "psf", "pixels": side, **plain[side]}), flush=True)
    for K in args.K:
        parameters = parameters_of(lens, det, K)
        first = timed(lambda: frame.sensitivity(det, parameters, [lens, det], wavefront=wave))
        print(json.dumps({**common, "what": "sensitivity", "K": K, **first}), flush=True)
        sens = frame.sensitivity(det, parameters, [lens, det], wavefront=wave)
        for side in args.pixels:
            got = sens.psf_gradient(world_unit_um=1000.0, pixels=side)
            new = timed(lambda: sens.psf_gradient(world_unit_um=1000.0, pixels=side))
            differences = 2 * K * (retrace["ms"] + plain[side]["ms"])
            print(json.dumps({**common, "what": "psf_gradient", "K": K, "pixels": side, **new,
                              "with_sensitivity_ms": new["ms"] + first["ms"], "psf_ms": plain[side]["ms"],
                              "psf_gradient_over_psf": new["ms"] / plain[side]["ms"], "differences_ms": differences,
                              "differences_over_one_pass": differences / (new["ms"] + first["ms"]),
                              "n_rays": int(got.n_rays.sum()), "n_unfollowed": int(got.n_unfollowed.sum()),
                              "strehl": float(got.strehl[0]), "dstrehl": got.dstrehl[0].tolist()[:4]}), flush=True)


if __name__ == "__main__":
    main()
