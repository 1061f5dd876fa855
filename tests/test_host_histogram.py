"""Histograms of the result frame (prt_frame_range / prt_frame_histogram), the host side: the ABI is declared, bound
and exported; the edges are numpy's own for every form of ``bins`` / ``range``, with numpy's errors; bad arguments are
refused before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "prt.h")
NEW = ("prt_frame_range", "prt_frame_histogram_workspace_bytes", "prt_frame_histogram")


@pytest.fixture(scope="module")
def lib():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "pyrayt_amd", "csrc")], check=True)
    return engine.library()


def test_histogram_entry_points_are_declared_bound_and_exported(lib):
    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(engine.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in engine.EXPORTED_SYMBOLS, name
        assert hasattr(raw, name), name
    assert engine.PRT_VERSION >= 230


def _auto(lo_hi):
    calls = []

    def finite_range(axis):
        calls.append(axis)
        return lo_hi[axis]
    return finite_range, calls


@pytest.mark.parametrize("bins,range_", [(10, (-1.0, 2.0)), (1, (0.0, 1.0)), (7, (3.0, 3.0)), (1000, (-1e-3, 5e-4)),
                                         (np.array([0.0, 0.5, 0.5, 2.0, 7.0]), None),
                                         ([-3, -1, 0, 4], (0.0, 1.0)), (np.linspace(-1, 1, 33), None)])
def test_one_dimensional_edges_are_numpys(bins, range_):
    from pyrayt_amd.frame import histogram_edges

    finite_range, calls = _auto([(-1.0, 1.0)])
    edges, uniform = histogram_edges(bins, range_, 1, finite_range)
    want = np.histogram(np.empty(0), bins=bins, range=range_)[1]
    assert np.array_equal(edges[0], want) and edges[0].dtype == np.float64
    assert uniform == (np.ndim(bins) == 0,) and not calls


def test_automatic_range_is_asked_for_only_when_numpy_would_look_at_the_data():
    from pyrayt_amd.frame import histogram_edges

    finite_range, calls = _auto([(-2.0, 5.0), (4.0, 4.0)])
    edges, _ = histogram_edges(16, None, 1, finite_range)
    assert calls == [0] and np.array_equal(edges[0], np.histogram(np.array([-2.0, 5.0]), bins=16)[1])
    finite_range, calls = _auto([(-2.0, 5.0), (4.0, 4.0)])
    edges, uniform = histogram_edges((8, [0, 1, 2]), ((-1, 1), None), 2, finite_range)
    assert calls == [] and uniform == (True, False)
    edges, uniform = histogram_edges(8, (None, (0, 3)), 2, finite_range)
    assert calls == [0]
    edges, _ = histogram_edges(8, None, 2, finite_range)
    # a single value v: (v - 0.5, v + 0.5), as numpy
    want = np.histogram2d(np.array([-2.0, 5.0]), np.array([4.0, 4.0]), bins=8)
    assert np.array_equal(edges[0], want[1]) and np.array_equal(edges[1], want[2])


@pytest.mark.parametrize("bins,range_", [(10, ((-1.0, 2.0), (0.0, 1.0))), ((3, 5), ((0, 1), (2, 2))),
                                         ([np.array([0.0, 1.0, 3.0]), np.array([-1.0, 0.0, 0.0, 1.0])], None),
                                         ((4, np.array([0.0, 0.25, 1.0])), ((1, 2), None)),
                                         (np.array([0.0, 1.0, 2.0, 4.0]), None),
                                         ((1024, 1024), ((-0.1, 0.1), (-0.1, 0.1)))])
def test_two_dimensional_edges_are_numpys(bins, range_):
    from pyrayt_amd.frame import histogram_edges

    edges, uniform = histogram_edges(bins, range_, 2, _auto([(0.0, 1.0), (0.0, 1.0)])[0])
    _, wx, wy = np.histogram2d(np.empty(0), np.empty(0), bins=bins, range=range_)
    assert np.array_equal(edges[0], wx) and np.array_equal(edges[1], wy)


def _message(call):
    with pytest.raises(ValueError) as info:
        call()
    return str(info.value)


@pytest.mark.parametrize("bins,range_", [(10, (2.0, 1.0)), (10, (0.0, np.inf)), (10, (np.nan, 1.0)),
                                         (10, (1.0, 1.0 + 1e-15)), (0, (0.0, 1.0)), (-3, None),
                                         (np.array([0.0, 2.0, 1.0]), None)])
def test_one_dimensional_errors_are_numpys(bins, range_):
    from pyrayt_amd.frame import histogram_edges

    want = _message(lambda: np.histogram(np.empty(0) if range_ is not None else np.zeros(3), bins=bins, range=range_))
    assert _message(lambda: histogram_edges(bins, range_, 1, _auto([(0.0, 1.0)])[0])) == want


@pytest.mark.parametrize("bins,range_", [(10, ((2.0, 1.0), (0, 1))), (10, ((0, 1), (0, np.inf))),
                                         ([np.array([0.0, 2.0, 1.0]), 4], None), ((0, 3), ((0, 1), (0, 1)))])
def test_two_dimensional_errors_are_numpys(bins, range_):
    from pyrayt_amd.frame import histogram_edges

    empty = np.empty(0) if range_ is not None else np.zeros(3)
    want = _message(lambda: np.histogram2d(empty, empty, bins=bins, range=range_))
    assert _message(lambda: histogram_edges(bins, range_, 2, _auto([(0.0, 1.0), (0.0, 1.0)])[0])) == want


@pytest.mark.parametrize("dims", [1, 2])
def test_string_estimators_are_refused(dims):
    from pyrayt_amd.frame import histogram_edges

    with pytest.raises(ValueError, match="not supported"):
        histogram_edges("auto", None, dims, _auto([(0.0, 1.0), (0.0, 1.0)])[0])
    if dims == 2:
        with pytest.raises(ValueError, match="not supported"):
            histogram_edges(("fd", 4), None, 2, _auto([(0.0, 1.0), (0.0, 1.0)])[0])


def test_bad_arguments_are_refused_before_a_device_is_touched(lib):
    """prt_frame_histogram / prt_frame_range validate on the host, like prt_scene_create: PRT_ERR_ARG with a message,
    and no device is needed to find out (the output pointers are never written)."""
    nan = float("nan")
    edges = np.linspace(0.0, 1.0, 5)
    bad = np.array([0.0, 1.0, 0.5, 2.0, 3.0])
    with_nan = np.array([0.0, nan, 1.0, 2.0, 3.0])
    fake = ctypes.c_void_p(0x1000)  # (not dereferenced: every case fails validation first)

    def call(n_groups=1, rps=0.0, xq=10, xe=edges, nx=4, yq=-1, ye=None, ny=0, wcol=-1, weights=None, rows=None,
             n_rows=0, ld=0):
        return lib.prt_frame_histogram(0, rows, ld, n_rows, nan, nan, rps, n_groups, xq,
                                       None if xe is None else xe.ctypes.data, nx, 1, yq,
                                       None if ye is None else ye.ctypes.data, ny, 0, wcol, fake, weights, fake, None)

    cases = [dict(nx=0), dict(xq=16), dict(xq=-1), dict(yq=16, ye=edges, ny=4), dict(yq=11, ye=edges, ny=0),
             dict(xe=bad), dict(xe=with_nan), dict(yq=11, ye=bad, ny=4), dict(xe=None), dict(wcol=15, weights=fake),
             dict(wcol=1), dict(weights=fake), dict(n_groups=2), dict(n_groups=0, rps=10.0), dict(n_rows=5, ld=5),
             dict(n_rows=5, ld=4, rows=fake)]
    for case in cases:
        assert call(**case) == -1, case
        assert lib.prt_last_error(), case
    box = ctypes.c_void_p(0x2000)
    assert lib.prt_frame_range(0, None, 0, 0, nan, nan, 16, box, None) == -1
    assert lib.prt_frame_range(0, None, 0, 0, nan, nan, 3, None, None) == -1
    assert lib.prt_frame_histogram_workspace_bytes(1, 4, 0, 0) == 5 * 8
    assert lib.prt_frame_histogram_workspace_bytes(4, 1024, 1024, 1) == 2050 * 8
    assert lib.prt_frame_histogram_workspace_bytes(1, 0, 3, 0) == -1
    assert lib.prt_frame_histogram_workspace_bytes(0, 3, 3, 0) == -1
