"""Dump every output of a seeded list of sensitivity() cases from one tree: python profiles/sensitivity_core/sens_dump.py TREE OUT.npz
A case that raises is dumped as the text of its exception."""
import os
import sys

tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path[:0] = [tree, os.path.join(tree, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import launch_scenes  # noqa: E402
import opd_scenes  # noqa: E402
import pyrayt_amd as prt  # noqa: E402
from pyrayt_amd.frame import DeviceFrame  # noqa: E402

assert os.path.abspath(prt.__file__).startswith(tree), prt.__file__
OUT = {}
NAMES = ("jacobian", "sums", "slopes", "dfield", "dopd", "dpupil", "opd", "pupil", "opd_sums")


def device_frame(frame, counts):
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, list(counts))


def host(value):
    return value.cpu().numpy() if hasattr(value, "cpu") else np.asarray(value)


def dump(key, call):
    try:
        got = call()
    except Exception as error:  # noqa: BLE001
        OUT[f"{key}/raised"] = np.frombuffer(f"{type(error).__name__}: {error}".encode(), dtype=np.uint8)
        return
    for name in NAMES:
        value = getattr(got, name, None)
        if value is not None:
            OUT[f"{key}/{name}"] = host(value).astype(np.float64)
    OUT[f"{key}/record"] = np.asarray([got.n_unknown, got.n_invalid, got.n_unfit, got.n_reflections], dtype=np.int64)


def motions(parts, K, seed):
    rng = np.random.default_rng(seed)
    return [prt.Motion(parts[k % len(parts)], translate=tuple(rng.uniform(-1, 1, 3)), rotate=tuple(rng.uniform(-1, 1, 3)),
                       pivot=tuple(rng.uniform(-0.5, 0.5, 3))) for k in range(K)]


def parameters_of(form, case, K, seed):
    rigid = motions(case.parts, 16, seed)
    old = [case.parameters[k] for k in (6, 7, 8, 12)]  # (Motion, Deformation, IndexChange among the launch scene's sixteen)
    if form in ("rigid", "rigid+slopes"):
        return rigid[:K]
    if form in ("design", "wavefront", "design+slopes"):
        return (old + rigid)[:K] if K > 1 else [old[2]]
    return list(case.parameters[:K]) if K > 1 else [case.parameters[form == "launch+wavefront" and 5 or 0]]


FORMS = ("rigid", "design", "wavefront", "launch", "launch+wavefront", "rigid+slopes", "design+slopes")
KS, JS = (1, 2, 7, 16), (1, 15, 36)


def run(key, dev, case, form, K, J, weights, kw, reference="centroid", system=None, surface=None, pars=None, seed=0):
    surface = case.surface if surface is None else surface
    pars = parameters_of(form, case, K, seed) if pars is None else pars

    def call():
        more = {}
        if "wavefront" in form:
            more["wavefront"] = dev.wavefront(surface, zernike=J, weights=weights, pupil_radius=0.4, **kw)
        if "slopes" in form:
            more["slopes"] = True
        return dev.sensitivity(surface, pars, case.parts if system is None else system, weights=weights, reference=reference,
                               **kw, **more)

    dump(key, call)


def groupings(frame, n):
    """(name, frame, keywords): three groups of n; one group; four with an empty third (the last source's ids moved up)."""
    moved = frame.copy()
    moved[moved[:, 4] >= 2 * n, 4] += n
    return [("g3", frame, dict(rays_per_source=n, n_groups=3)), ("g1", frame, {}),
            ("g2", frame, dict(rays_per_source=2 * n, n_groups=2)), ("g4e", moved, dict(rays_per_source=n, n_groups=4))]


at = 0
for n in (1, 255, 256, 257, 300):
    case = launch_scenes.build("fields", n)
    for gname, frame, kw in groupings(case.frame, n):
        dev = device_frame(frame, case.counts)
        n_groups = kw.get("n_groups", 1)
        for form in FORMS:
            K, J, weights = KS[at % 4], JS[at % 3], (None, "intensity")[at % 2]
            reference = "centroid" if at % 5 else np.random.default_rng(at).uniform(-0.1, 0.1, (n_groups, 3)) + [1.0, 0, 0]
            run(f"fields{n}/{gname}/{form}/K{K}J{J}w{weights}", dev, case, form, K, J, weights, kw, reference=reference, seed=at)
            at += 1

# K x J in full, on two fields of 300 (the opd scenes) and on the three fields of 300
case = launch_scenes.build("fields", 300)
dev = device_frame(case.frame, case.counts)
for K in KS:
    for J in JS:
        for form in ("wavefront", "launch+wavefront"):
            run(f"cross/fields300/{form}/K{K}J{J}", dev, case, form, K, J, "intensity", dict(rays_per_source=300, n_groups=3))
    for form in ("rigid", "design", "launch"):
        run(f"cross/fields300/{form}/K{K}", dev, case, form, K, 0, None, dict(rays_per_source=300, n_groups=3))
two = opd_scenes.build("two_fields", 300)
dev2 = device_frame(two.frame, two.counts)
for J in JS:
    dump(f"two_fields300/J{J}", lambda: dev2.sensitivity(two.surface, list(two.parameters), two.parts, rays_per_source=300, n_groups=2,
                                                         wavefront=dev2.wavefront(two.surface, zernike=J, weights="intensity",
                                                                                  rays_per_source=300, n_groups=2)))

# a row with a NaN end point, a surface left out of system, an empty selection, an empty frame: every form
kw = dict(rays_per_source=257, n_groups=3)
case = launch_scenes.build("fields", 257)
broken = case.frame.copy()
landed = np.flatnonzero(broken[:, 5] == case.surface.get_id() if hasattr(case.surface, "get_id") else broken[:, 5] == case.surface)
broken[landed[100], 9] = np.nan
lens, det = case.parts
on_det = [prt.Motion(det, translate=(1, 0, 0)), prt.Deformation(det, rotate=(0, 0, 1), pivot=(1, 0, 0)),
          prt.SourceMotion(None, translate=(0, 1, 0))]
empty = DeviceFrame(torch.empty((15, 0), dtype=torch.float64, device="cuda:0"), [0])
for form in FORMS:
    K = 3 if form.startswith("rigid") else 7
    run(f"nan_row/{form}", device_frame(broken, case.counts), case, form, K, 15, "intensity", kw)
    pars = on_det[:1] if form.startswith("rigid") else on_det[:2] if not form.startswith("launch") else on_det
    run(f"left_out/{form}", device_frame(case.frame, case.counts), case, form, K, 15, "intensity", kw, system=[det], pars=pars)
    run(f"nobody/{form}", device_frame(case.frame, case.counts), case, form, K, 15, "intensity", kw, surface=10 ** 6)
    run(f"empty/{form}", empty, case, form, K, 15, "intensity", kw)

# what the Python side refuses
dev = device_frame(case.frame, case.counts)
good = on_det[:2]
bad_rate, bad_range, bad_twist, bad_linear, bad_index = (prt.WavelengthChange(), prt.SourceMotion((3, 4), translate=(0, 1, 0)),
                                                          prt.SourceMotion(None, translate=(0, 1, 0)),
                                                          prt.Deformation(det, translate=(1, 0, 0)), prt.IndexChange(lens))
bad_rate.rate, bad_range.id_range, bad_twist.twist = float("inf"), (7.0, 3.0), np.full(9, np.nan)
bad_linear.linear, bad_index.rate = np.full((3, 3), np.inf), float("nan")
other = device_frame(case.frame, case.counts)
REFUSALS = {
    "no parameters": lambda: dev.sensitivity(det, [], case.parts),
    "not a parameter": lambda: dev.sensitivity(det, [good[0], (0, 16)], case.parts),
    "seventeen": lambda: dev.sensitivity(det, good * 9, case.parts),
    "weights": lambda: dev.sensitivity(det, good, case.parts, weights="weight"),
    "reference name": lambda: dev.sensitivity(det, good, case.parts, reference="centre"),
    "reference shape": lambda: dev.sensitivity(det, good, case.parts, reference=np.zeros((2, 3)), **kw),
    "reference nan": lambda: dev.sensitivity(det, good, case.parts, reference=(np.nan, 0, 0)),
    "surface None": lambda: dev.sensitivity(None, good, case.parts),
    "wavefront type": lambda: dev.sensitivity(det, good, case.parts, wavefront="centroid"),
    "wavefront other frame": lambda: dev.sensitivity(det, good, case.parts, wavefront=other.wavefront(det, weights="intensity")),
    "wavefront other groups": lambda: dev.sensitivity(det, good, case.parts, wavefront=dev.wavefront(det, weights="intensity"), **kw),
    "wavefront other weights": lambda: dev.sensitivity(det, good, case.parts, wavefront=dev.wavefront(det)),
    "no surfaces": lambda: dev.sensitivity(det, good, []),
    "not in system": lambda: dev.sensitivity(det, [prt.Motion(lens, translate=(1, 0, 0))], [det]),
    "of_source": lambda: dev.sensitivity(det, [prt.SourceMotion.of_source(0, translate=(0, 1, 0))], case.parts),
    "groups": lambda: dev.sensitivity(det, good, case.parts, rays_per_source=1, n_groups=70000),
    "empty with wavefront and slopes": lambda: empty.sensitivity(det, good, case.parts, wavefront=True, slopes=True),
    "a part of a frame": lambda: dev.generation(1).sensitivity(det, good, case.parts),
    "rate": lambda: dev.sensitivity(det, [bad_rate], case.parts),
    "range": lambda: dev.sensitivity(det, [bad_range], case.parts),
    "twist": lambda: dev.sensitivity(det, [bad_twist], case.parts),
    "linear": lambda: dev.sensitivity(det, [bad_linear], case.parts),
    "index rate": lambda: dev.sensitivity(det, [bad_index], case.parts),
}
for name, call in REFUSALS.items():
    dump(f"refusal/{name}", call)
    assert f"refusal/{name}/raised" in OUT, name

np.savez(out_path, **OUT)
raised = [k for k in OUT if k.endswith("/raised") and not k.startswith("refusal/")]
print(f"{tree}: {len(OUT)} arrays, {sum(v.size for v in OUT.values())} values, {len(raised)} cases raised")
for k in raised:
    print("  raised:", k, bytes(OUT[k]).decode()[:160])
