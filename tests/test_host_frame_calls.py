"""What every pass of ``pyrayt_amd.frame`` hands to the library, pinned without a GPU: a stand-in for ``engine.library()``
records each call, every argument reduced by its declared type in the binding's table, and the record of a hand-made CPU
frame going through the public methods is held to ``tests/golden/frame_calls.json``.  The file was written from the
commit before the calls were routed through ``engine.call`` (``python tests/test_host_frame_calls.py`` writes it again, on
purpose, after an ABI change), so an argument that moves, changes its value or turns from a pointer into NULL shows here.
``engine.call`` itself is tested at the end."""
import ctypes
import json
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_calls.json")
INTEGERS, REAL, POINTER = (ctypes.c_int, ctypes.c_int64), ctypes.c_double, ctypes.c_void_p


def signatures(engine):
    """The binding's table ``{name: (restype, argtypes)}``."""
    return engine.SIGNATURES


def reduced(value, kind):
    """An argument as the record keeps it: a pointer as "ptr", "NULL" or "handle" (a ``c_void_p`` object with a value: the
    stand-in communicator), a number as its value (NaN as "nan").  What ctypes would refuse is refused."""
    if kind is POINTER:
        if isinstance(value, ctypes.c_void_p):
            return "handle" if value.value else "NULL"
        assert value is None or (isinstance(value, int) and not isinstance(value, bool)), value
        return "ptr" if value else "NULL"
    if kind in INTEGERS:
        assert isinstance(value, (int, np.integer)), value
        return int(value)
    assert kind is REAL and isinstance(value, (int, float, np.integer, np.floating)), (value, kind)
    return "nan" if np.isnan(value) else float(value)


class Library:
    """``engine.library()``'s stand-in: every bound function records ``[name, arguments]`` and answers 4096 for a size,
    0 otherwise."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def __getattr__(self, name):
        if name not in self.table:
            raise AttributeError(name)
        kinds = self.table[name][1]

        def entry(*args):
            assert len(args) == len(kinds), (name, len(args), len(kinds))
            self.calls.append([name, [reduced(a, k) for a, k in zip(args, kinds)]])
            return 4096 if name.endswith("_workspace_bytes") else 0

        return entry


def stand_ins(monkeypatch):
    """The stand-ins in place: ``run(case)`` gives the case's record, ``{"calls": [...], "raised": a type's name or None}``.
    Outputs are zeros (``torch.empty`` is ``torch.zeros``), so some result objects cannot be built: the calls count."""
    from pyrayt_amd import engine, frame

    library = Library(signatures(engine))
    monkeypatch.setattr(engine, "library", lambda: library)
    monkeypatch.setattr(engine, "_stream_ptr", lambda torch, device: None)
    monkeypatch.setattr(torch, "empty", torch.zeros)
    monkeypatch.setattr(frame, "_all_reduce_sum", lambda tensor, group: tensor)
    monkeypatch.setattr(frame, "_all_reduce_min", lambda tensor, group: tensor)
    monkeypatch.setattr(frame, "_all_reduce_max", lambda value, group, comm, device: value)

    def run(case):
        library.calls = []
        raised = None
        try:
            case()
        except Exception as error:  # noqa: BLE001
            raised = type(error).__name__
        return {"calls": library.calls, "raised": raised}

    return run


@pytest.fixture
def recorded(monkeypatch):
    return stand_ins(monkeypatch)


def make_frame(n=8, generations=2):
    """``generations`` generations of ``n`` rays along +x: ids 0..n-1, generation g from x = g to x = g + 1 on surface
    g + 1, at heights on a ring so that no two rays share a point; the (15, 0) frame of one empty generation for n = 0."""
    from pyrayt_amd.frame import COLUMNS, DeviceFrame

    rows = np.zeros((len(COLUMNS), n * generations))
    col = {name: rows[k] for k, name in enumerate(COLUMNS)}
    for g in range(generations):
        part = slice(g * n, (g + 1) * n)
        angle = 2 * np.pi * np.arange(n) / max(n, 1)
        col["generation"][part], col["surface"][part], col["id"][part] = g, g + 1, np.arange(n)
        col["intensity"][part], col["wavelength"][part], col["index"][part] = 100.0, 0.55 + 0.1 * (np.arange(n) % 2), 1.0
        col["x0"][part], col["x1"][part], col["x_tilt"][part] = g, g + 1, 1.0
        for a, b in (("y0", "y1"), ("z0", "z1")):
            col[a][part] = col[b][part] = 0.25 * (np.cos(angle) if a == "y0" else np.sin(angle))
    if not n:  # (as a trace without rows makes it: torch's own empty block, whose strides are 1)
        return DeviceFrame(torch.zeros((len(COLUMNS), 0), dtype=torch.float64), [0])
    return DeviceFrame(torch.from_numpy(rows), [n] * generations)


def cases():
    """``{name: callable}``: the frames of the issue -- two generations of 8 rays, the same with a surface that selects
    nothing (7), the empty frame -- through every method that reaches the library, on both sides of every pointer that
    may be NULL and of the generation slice."""
    import pyrayt_amd.frame as F
    from pyrayt_amd.materials import BasicRefractor, Coating
    from pyrayt_amd.scene import MATERIAL_DTYPE, PRIM_DTYPE

    full, empty = make_frame(), make_frame(0)
    comm = SimpleNamespace(_handle=ctypes.c_void_p(1))
    point, nu = (0.0, 0.1, 0.0), (0.0, 1.0, 2.0)
    system = SimpleNamespace(prims=np.zeros(2, dtype=PRIM_DTYPE), materials=np.zeros(1, dtype=MATERIAL_DTYPE))
    system.prims["surface_id"] = (1, 2)
    out = {}

    def add(name, call, frames=(("full", full),)):
        for label, frame in frames:
            out[f"{name}[{label}]"] = (lambda call=call, frame=frame: call(frame))

    everywhere = (("full", full), ("empty", empty))
    # statistics
    add("group_stats", lambda f: f.group_stats(), everywhere)
    add("group_stats-filtered", lambda f: f.group_stats(surface=2, generation=1, rays_per_source=4), everywhere)
    add("group_stats-nothing", lambda f: f.group_stats(surface=7))
    add("group_stats-comm", lambda f: f.group_stats(surface=2, rays_per_source=4, n_groups=2, comm=comm), everywhere)
    add("group_stats-group", lambda f: f.group_stats(surface=2, rays_per_source=4, group="ranks"), everywhere)
    add("mean_square", lambda f: f.mean_square("y1"), everywhere)
    add("mean_square-filtered", lambda f: f.mean_square("axis_intercept", about=0.5, transform="sin", surface=2,
                                                        generation="last", rays_per_source=4, group="ranks"), everywhere)
    add("histogram", lambda f: f.histogram("y1"), everywhere)
    add("histogram-weights", lambda f: f.histogram("y1", bins=4, range=(-1.0, 1.0), weights="intensity", surface=2,
                                                   generation=1, rays_per_source=4))
    add("histogram-last", lambda f: f.histogram("z1", generation="last", group="ranks"), everywhere)
    add("histogram-nothing", lambda f: f.histogram("y1", surface=7))
    add("histogram2d", lambda f: f.histogram2d("y1", "z1", bins=(3, 2), weights="intensity", generation="last"))
    add("histogram2d-edges", lambda f: f.histogram2d("y1", "z1", bins=(np.array([-1.0, 0.0, 0.5, 1.0]), 2)))
    # the joins by ray id
    add("optical_path", lambda f: f.optical_path(), everywhere)
    add("launch_index", lambda f: f.launch_index(), everywhere)
    add("launch", lambda f: f.launch(surface=2, generation="last"))
    add("paths", lambda f: f.paths(), everywhere)
    add("paths-plain", lambda f: f.paths(weights=None, rays_per_source=4, max_paths=16))
    add("fresnel", lambda f: f.fresnel(), everywhere)
    add("fresnel-fields", lambda f: f.fresnel(polarization=(0, 1, 0), lossless=(1,), fields=True), everywhere)
    add("fresnel-complex", lambda f: f.fresnel(polarization=(0, 1, 1j), fields=True))
    quarter = Coating([(1.38, 0.1)], substrate=BasicRefractor(1.5))
    add("fresnel-coated", lambda f: f.fresnel(coatings={2: quarter}, fields=True), everywhere)
    add("fresnel-coated-lossless", lambda f: f.fresnel(polarization=(0, 0, 1), lossless=(1,), coatings={2: quarter}))
    # wavefront and the Huygens sums
    add("wavefront", lambda f: f.wavefront(2), everywhere)
    add("wavefront-point", lambda f: f.wavefront(2, reference=point, radius=3.0, pupil_radius=0.5, zernike=6,
                                                 weights="intensity", generation=1, rays_per_source=4))
    add("wavefront-last", lambda f: f.wavefront(None, generation="last"))
    add("wavefront-nothing", lambda f: f.wavefront(7))
    psf = dict(world_unit_um=1000.0, pixels=(4, 3), pixel_size=0.01)
    add("psf", lambda f: f.psf(2, **psf), everywhere)
    add("psf-default-step", lambda f: f.psf(2, world_unit_um=1000.0, pixels=4))
    add("psf-plain", lambda f: f.psf(2, weights=None, reference=point, generation="last", rays_per_source=4, **psf))
    add("psf-nothing", lambda f: f.psf(7, **psf))
    add("psf-focus", lambda f: f.psf(2, focus=(-0.1, 0.0, 0.1), **psf))
    add("psf-focus-untracked", lambda f: f.psf(2, focus=(0.0,), track=None, weights=None, generation=1, **psf))
    add("psf-fresnel", lambda f: f.psf(2, fresnel=f.fresnel(polarization=(0, 1, 0), fields=True), **psf))
    add("psf-fresnel-complex", lambda f: f.psf(2, fresnel=f.fresnel(polarization=(0, 1, 1j), fields=True),
                                               generation="last", weights=None, **psf))
    add("psf-fresnel-unpolarised", lambda f: f.psf(2, fresnel=f.fresnel(fields=True), generation=1, **psf))
    # the image passes
    add("mtf", lambda f: f.mtf(2, nu), everywhere)
    add("mtf-point", lambda f: f.mtf(None, nu, azimuths=(0.0,), focus=(-0.1, 0.1), reference=point, weights=None,
                                     generation="last", rays_per_source=4))
    add("mtf-nothing", lambda f: f.mtf(7, nu, generation=1))
    add("energy-fractions", lambda f: f.enclosed_energy(2), everywhere)
    add("energy-radii", lambda f: f.enclosed_energy(2, radii=(0.1, 0.2), fractions=None, shape="square",
                                                    follow_centroid=False, reference=point, weights=None, generation=1))
    add("energy-both", lambda f: f.enclosed_energy(2, radii=(0.1,), focus=(0.0, 0.1), generation="last",
                                                   rays_per_source=4))
    add("energy-nothing", lambda f: f.enclosed_energy(7, radii=(0.1,)))
    add("ray_aberrations", lambda f: f.ray_aberrations(2), everywhere)
    add("ray_aberrations-direction", lambda f: f.ray_aberrations(None, pupil="direction", reference=point, pupil_radius=0.5,
                                                                 zernike=6, zones=0, weights="intensity", generation=1,
                                                                 rays_per_source=4))
    add("ray_aberrations-chief", lambda f: f.ray_aberrations(2, reference="chief", zones=4, generation="last"))
    add("ray_aberrations-nothing", lambda f: f.ray_aberrations(7))
    # sensitivities, and what is made of their results
    glass = SimpleNamespace(surface_ids=((1, SimpleNamespace(material=BasicRefractor(1.5))),))
    rigid = [F.Motion(1, translate=(1, 0, 0)), F.Motion(2, rotate=(0, 0, 1))]
    design = rigid + [F.Deformation(1, linear=np.eye(3)), F.IndexChange(glass)]
    launch = rigid[:1] + [F.SourceMotion((0, 4), translate=(0, 1, 0)), F.WavelengthChange()]

    def sensitivity(parameters, **more):
        return lambda f: f.sensitivity(2, parameters, system, **more)

    add("sensitivity-rigid", sensitivity(rigid), everywhere)
    add("sensitivity-rigid-point", sensitivity(rigid, weights=None, reference=point, generation="last", rays_per_source=4))
    add("sensitivity-nothing", lambda f: f.sensitivity(7, rigid, system))
    add("sensitivity-design", sensitivity(design, generation=1), everywhere)
    add("sensitivity-wavefront", sensitivity(design, wavefront=True), everywhere)
    add("sensitivity-launch", sensitivity(launch, rays_per_source=4), everywhere)
    add("sensitivity-slopes", sensitivity(rigid, slopes=True, weights=None))
    add("sensitivity-launch-wavefront", sensitivity(rigid, slopes=True, wavefront=True, generation="last"), everywhere)
    add("mtf_gradient", lambda f: sensitivity(rigid, slopes=True)(f).mtf_gradient(nu))
    add("mtf_gradient-centre", lambda f: sensitivity(rigid, slopes=True, weights=None, rays_per_source=4)(f).mtf_gradient(
        nu, azimuths=(0.0,), focus=(0.0, 0.1), reference="centroid", centre=point))
    add("mtf_gradient-nothing", lambda f: f.sensitivity(7, rigid, system, slopes=True).mtf_gradient(nu))
    for follow in ("ray", "pupil"):
        add(f"psf_gradient-{follow}",
            lambda f, follow=follow: sensitivity(rigid, wavefront=True)(f).psf_gradient(follow=follow, **psf))
        add(f"tolerance-{follow}", lambda f, follow=follow: sensitivity(rigid, wavefront=True, weights=None)(f).tolerance(
            np.array([[0.1, 0.0], [0.0, 0.1], [0.1, 0.1]]), world_unit_um=1000.0, follow=follow,
            compensators=("focus", "tilt", 1) if follow == "ray" else ()))
    add("psf_gradient-nothing", lambda f: f.sensitivity(7, rigid, system, wavefront=True).psf_gradient(**psf))
    # (the three calls of tests/test_host_mtf_tolerance.py::test_the_pass_calls_the_library_as_the_header_declares_it)
    trials, sampling = np.array([[0.1, 0.0], [0.0, 0.1], [0.1, 0.1]]), dict(azimuths=(0.0,), focus=(0.0, 0.1))
    add("mtf_tolerance-centre", lambda f: sensitivity(rigid, slopes=True, rays_per_source=4)(f).mtf_tolerance(
        trials, nu, compensators=("focus",), centre=point, **sampling))
    add("mtf_tolerance", lambda f: sensitivity(rigid, slopes=True)(f).mtf_tolerance(trials, nu, **sampling))
    add("mtf_tolerance-nothing", lambda f: f.sensitivity(7, rigid, system, slopes=True).mtf_tolerance(
        trials, nu, reference="fixed", **sampling))
    return out


def frame_entry_points():
    """Every ``prt_frame_*`` name that ``pyrayt_amd/frame.py`` reaches the library by."""
    text = open(os.path.join(ROOT, "pyrayt_amd", "frame.py")).read()
    return sorted(set(re.findall(r"\bprt_frame_\w+", re.sub(r'(?s:""".*?""")|#[^\n]*', "", text))))


def record_all(run):
    return {name: run(case) for name, case in cases().items()}


def test_every_pass_calls_the_library_as_the_golden_record_says(recorded):
    golden = json.load(open(GOLDEN))
    found = record_all(recorded)
    assert sorted(found) == sorted(golden)
    differing = [name for name in golden if found[name] != golden[name]]
    assert not differing, {name: (found[name], golden[name]) for name in differing[:2]}


def test_the_golden_record_holds_every_entry_point_of_frame_py():
    from pyrayt_amd import engine

    golden = json.load(open(GOLDEN))
    seen = {name for case in golden.values() for name, _ in case["calls"]}
    table = signatures(engine)
    wanted = set(frame_entry_points())
    assert len(wanted) >= 29 and wanted <= set(table)
    wanted |= {name + "_workspace_bytes" for name in wanted if name + "_workspace_bytes" in table}
    assert wanted <= seen, sorted(wanted - seen)


# ---- engine.call ------------------------------------------------------------------------------------------------------------
class TwoFunctions:
    """A library of one entry point and its size function, with ``prt_last_error``."""

    def __init__(self, size=4096, code=0):
        self.size, self.code, self.calls = size, code, []

    def prt_pass_workspace_bytes(self, *args):
        self.calls.append(("size", args))
        return self.size

    def prt_pass(self, *args):
        self.calls.append(("pass", args))
        return self.code

    def prt_last_error(self):
        return b"prt_pass: n_groups in [1, 65535]"


@pytest.fixture
def two_functions(monkeypatch):
    from pyrayt_amd import engine

    def install(**answers):
        library = TwoFunctions(**answers)
        monkeypatch.setattr(engine, "library", lambda: library)
        monkeypatch.setattr(engine, "_stream_ptr", lambda torch, device: "stream")
        return library

    return install


def test_call_turns_its_arguments_into_pointers_and_puts_workspace_and_stream_last(two_functions):
    from pyrayt_amd import engine

    library = two_functions()
    tensor, nothing, array = torch.zeros(3, dtype=torch.float64), torch.zeros((2, 0)), np.arange(4.0)
    assert engine.call("prt_pass", tensor, nothing, array, None, 7, 2.5, device=tensor.device) == 0
    (name, args), = library.calls  # (no size asked for: no workspace)
    assert name == "pass" and args == (tensor.data_ptr(), None, array.ctypes.data, None, 7, 2.5, "stream")
    library.calls.clear()
    engine.call("prt_pass", tensor, 1, device=tensor.device, size=(3, 2))
    (_, size_args), (_, args) = library.calls
    assert size_args == (3, 2) and args[:2] == (tensor.data_ptr(), 1) and args[3] == "stream" and len(args) == 4
    assert isinstance(args[2], int) and args[2] not in (0, tensor.data_ptr())  # (the workspace, before the stream)


def test_call_sizes_by_another_entry_point_and_checks_the_size_and_the_return_code(two_functions):
    from pyrayt_amd import engine

    device = torch.device("cpu")
    library = two_functions()
    library.prt_other_workspace_bytes = lambda *args: library.calls.append(("other", args)) or 64
    engine.call("prt_pass", 1, device=device, size=(5,), sized_by="prt_other")
    assert [name for name, _ in library.calls] == ["other", "pass"]
    library = two_functions(size=-1)
    with pytest.raises(ValueError, match="n_groups in"):
        engine.call("prt_pass", 1, device=device, size=(5,))
    assert [name for name, _ in library.calls] == ["size"]  # (a refused size: the pass is not called)
    library = two_functions(code=-1)
    with pytest.raises(ValueError, match=r"prt_pass: n_groups in \[1, 65535\]"):
        engine.call("prt_pass", 1, device=device)
    library = two_functions(code=-7)
    with pytest.raises(RuntimeError, match="-7"):
        engine.call("prt_pass", 1, device=device)


if __name__ == "__main__":  # (write the golden record from the code as it stands: on purpose, after an ABI change)
    sys.path.insert(0, ROOT)
    patch = pytest.MonkeyPatch()
    try:
        record = record_all(stand_ins(patch))
    finally:
        patch.undo()
    with open(GOLDEN, "w") as out:
        json.dump(record, out, indent=0, sort_keys=True)
        out.write("\n")
    calls = [call for case in record.values() for call in case["calls"]]
    print(f"{GOLDEN}: {len(record)} cases, {len(calls)} calls, {sum(len(args) for _, args in calls)} arguments")
