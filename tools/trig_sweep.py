#!/usr/bin/env python3
"""eps_hw: the largest distance between (v_cos_f32(t), v_sin_f32(t)) and the unit phasor of the float turn t, measured
through DeviceFrame.mtf.  One ray that ends at p1 = +1 or -1 exactly, about reference=(0, 0, 0), at azimuth 0 has
OTF(nu) = exp(-2 pi i nu p1): the phase nu p1 is exact in fp64, v_fract_f64 is exact, and a float turn converts without
rounding, so k_mtf_sum returns the instructions' results as they are (prt_frame_mtf takes 4096 frequencies a call).

  binades    every float turn of [2^-k-1, 2^-k), k = 0 .. --binades - 1 (2^23 turns each)
  grid       every multiple of 2^-24 in [0, 1), with the phase positive and negative (negative ones pass v_fract_f64)
  special    0, the quarter turns and eight neighbours each side, 2^-k down to 2^-59, 1 - 2^-24, 65 536 random floats,
             both signs; and fp64 turns that round in the conversion (1 - 2^-30 rounds up to 1.0f)

The search compares with fp64 sines and cosines (1e-16, far under the 1e-7 looked for); the winner of each sample is
then restated in np.longdouble.  Writes profiles/mtf/trig_sweep.json and, with --readme, the table between the
"trig-sweep" markers of profiles/mtf/README.md.  tests/diffraction_reference.py records the largest value as
EPS_HW_MEASURED and twice that, rounded up to one digit, as EPS_TRIG.
--from-json FILE rewrites the table from an earlier run's file, without a GPU.
usage: tools/trig_sweep.py [--binades 10] [--no-grid] [--out DIR] [--readme] [--from-json FILE]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
CHUNK = 4096


def one_ray(p):
    import torch

    from pyrayt_amd.frame import DeviceFrame

    rows = np.zeros((15, 1))
    rows[1], rows[5], rows[10], rows[12] = 1.0, 4.0, p, 1.0
    return DeviceFrame(torch.from_numpy(rows).to("cuda:0"), [1])


def otf(device, nus):
    return np.concatenate([device.mtf(4.0, nus[at:at + CHUNK], azimuths=(0.0,), reference=(0.0, 0.0, 0.0)).otf[0, 0, 0]
                           for at in range(0, len(nus), CHUNK)])


def exact_distance(device, nu, p):
    """The distance at one frequency, against longdouble: (value, the turn the instructions saw)."""
    cycles = LD(nu) * LD(p)
    turn = cycles - np.floor(cycles)
    got = otf(device, np.array([nu]))[0]
    return float(np.hypot(LD(got.real) - np.cos(2 * PI * turn), LD(got.imag) + np.sin(2 * PI * turn))), float(turn)


def largest(device, p, blocks):
    """Over the frequencies the blocks yield: (largest distance in longdouble, its turn, the count, the fp64 mean)."""
    best, count, total = (0.0, 0.0), 0, 0.0
    for nus in blocks:
        got = otf(device, nus)
        angle = 2 * np.pi * (nus * p - np.floor(nus * p))
        distance = np.hypot(got.real - np.cos(angle), got.imag + np.sin(angle))
        k = int(np.argmax(distance))
        if distance[k] > best[0]:
            best = (float(distance[k]), float(nus[k]))
        count, total = count + len(nus), total + float(distance.sum())
    value, turn = exact_distance(device, best[1], p)
    return dict(max=value, turn=turn, turn_hex=turn.hex(), samples=count, mean=total / count)


def binade_blocks(k, block=1 << 19):
    lo = 2.0 ** -(k + 1)
    for at in range(0, 1 << 23, block):
        yield lo + np.arange(at, at + block, dtype=np.float64) * (lo * 2.0 ** -23)


def grid_blocks(block=1 << 20):
    for at in range(0, 1 << 24, block):
        yield np.arange(at, at + block, dtype=np.float64) / float(1 << 24)


def special_turns():
    rng = np.random.default_rng(20)
    near = []
    for quarter in (0.0, 0.25, 0.5, 0.75, 1.0):
        lo = hi = np.float32(quarter)
        for _ in range(8):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            near += [float(lo), float(hi)]
    fixed = [0.0, 0.25, 0.5, 0.75, 1 - 2.0 ** -24] + [x for x in near if 0 <= x < 1] + [2.0 ** -k for k in range(1, 60)]
    floats = np.unique(np.concatenate([fixed, rng.random(65536, dtype=np.float32).astype(np.float64)]))
    rounded = np.array([1 - 2.0 ** -30, 1 - 2.0 ** -25, 1 - 2.0 ** -26, 0.25 + 2.0 ** -27, 0.5 - 2.0 ** -27, 0.75 + 2.0 ** -40])
    return floats, rounded


def table(rows, eps):
    lines = ["| turns sampled | samples | largest distance | at turn |", "|---|---|---|---|"]
    for name, r in rows:
        value = f"{r['max']:.4e}"
        lines.append(f"| {name} | {r['samples']} | {'**' + value + '**' if r is eps else value} | `{r['turn_hex']}` ({r['turn']:.9g}) |")
    return "\n".join(lines)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--binades", type=int, default=10)
    parser.add_argument("--no-grid", action="store_true")
    parser.add_argument("--readme", action="store_true")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtf"))
    parser.add_argument("--from-json")
    args = parser.parse_args()
    if args.from_json:
        rows = list(json.load(open(args.from_json))["samples"].items())
        return report(rows, args, measured=False)
    plus, minus = one_ray(1.0), one_ray(-1.0)
    rows = []
    for k in range(args.binades):
        rows.append((f"every float in [2^-{k + 1}, {'2^-%d' % k if k else '1'})", largest(plus, 1.0, binade_blocks(k))))
        print(json.dumps({rows[-1][0]: rows[-1][1]}), flush=True)
    if not args.no_grid:
        rows.append(("every multiple of 2^-24 in [0, 1), phase positive", largest(plus, 1.0, grid_blocks())))
        rows.append(("the same, phase negative (through `v_fract_f64`)", largest(minus, -1.0, grid_blocks())))
    floats, rounded = special_turns()
    rows.append(("0, quarter turns and 8 neighbours a side, 2^-k to 2^-59, 1 - 2^-24, 65 536 random floats",
                 largest(plus, 1.0, [floats])))
    rows.append(("the same, phase negative", largest(minus, -1.0, [floats[floats > 0]])))
    rows.append(("fp64 turns that round in the conversion (1 - 2^-30 rounds up to `1.0f`), both signs: what is left of "
                 "the first-order correction", max((largest(plus, 1.0, [rounded]), largest(minus, -1.0, [rounded])),
                                                   key=lambda r: r["max"])))
    report(rows, args, measured=True)


def report(rows, args, measured):
    eps = max((r for _, r in rows[:-1]), key=lambda r: r["max"])  # (the last row's turns are no floats)
    if measured:
        with open(os.path.join(args.out, "trig_sweep.json"), "w") as f:
            json.dump(dict(eps_hw=eps, samples=dict(rows)), f, indent=1)
    text = table(rows, eps)
    print(text)
    print(json.dumps(dict(eps_hw=eps["max"], turn=eps["turn_hex"], twice=2 * eps["max"])))
    if args.readme:
        path = os.path.join(ROOT, "profiles", "mtf", "README.md")
        readme = open(path).read()
        block = re.compile(r"(<!-- trig-sweep:begin -->\n).*?(\n<!-- trig-sweep:end -->)", re.S)
        assert block.search(readme), "profiles/mtf/README.md has no trig-sweep markers"
        open(path, "w").write(block.sub(lambda m: m.group(1) + text + m.group(2), readme))


if __name__ == "__main__":
    main()
