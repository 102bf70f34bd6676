"""mnc_amd/csrc/ws_layout.h carves one device allocation into the typed sub-buffers of a workspace (voting, proposal, the host-array
entry points).  A layout runs twice, with a null base for the size and with the allocation for the pointers.  The header has no HIP
include, so it is compiled for the host here and held to what the kernels rely on: 256-byte aligned members that do not overlap,
and a size that is the same in both passes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("wslayout") / "ws_layout_shim.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "ws_layout_shim.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.ws_layout_run.restype = ctypes.c_size_t
    lib.ws_layout_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


def _run(lib, base, members):
    counts = np.array([c for c, _ in members], np.uint64)
    elem = np.array([e for _, e in members], np.int32)
    addrs = np.zeros(len(members), np.uint64)
    total = lib.ws_layout_run(base, counts.ctypes.data, elem.ctypes.data, len(members), addrs.ctypes.data)
    return int(total), [int(a) for a in addrs]


def _up256(x):
    return (x + 255) // 256 * 256


def _layouts():
    n, dim, batch = 600, 5, 20
    cb = (n + 63) // 64
    yield "nms", [(n * dim, 4), (batch * n, 4), (batch * n * cb, 8), (batch * n, 4), (batch, 4)]
    yield "nms without an order", [(n * dim, 4), (n * cb, 8), (n, 4), (1, 4)]
    yield "render, no instance", [(0, 48), (0, 4), (375 * 500, 4), (375 * 500, 4)]
    yield "render", [(7, 48), (7 * 21 * 21, 4), (375 * 500, 4), (375 * 500, 4)]
    yield "sds without ground truth", [(4 * 3, 8), (3 * 441, 1), (3, 4), (3, 4), (0, 4), (0, 8), (0, 8), (0, 1), (3, 4), (3, 8), (3, 8)]
    yield "all empty", [(0, 4), (0, 1), (0, 8)]
    yield "one byte each", [(1, 1)] * 5
    yield "exact multiples", [(256, 1), (64, 4), (32, 8), (16, 48)]
    yield "one short of and one past a multiple", [(255, 1), (257, 1), (63, 4), (65, 4)]
    rng = np.random.default_rng(0)
    for k in range(20):
        m = int(rng.integers(1, 24))
        counts = rng.integers(0, 5000, m) * (rng.random(m) > 0.25)
        yield "random %d" % k, [(int(c), int(e)) for c, e in zip(counts, rng.choice([1, 4, 8, 48], m))]


@pytest.mark.parametrize("name,members", list(_layouts()), ids=[n for n, _ in _layouts()])
def test_members_are_aligned_disjoint_and_sized_alike_in_both_passes(shim, name, members):
    size, offs = _run(shim, None, members)                       # sizing pass: null base, the addresses are the offsets
    buf = np.zeros(size + 512, np.uint8)
    base = _up256(buf.ctypes.data)                               # (hipMalloc returns at least this alignment)
    total, addrs = _run(shim, base, members)
    assert total == size
    assert [a - base for a in addrs] == offs
    assert all(o % 256 == 0 for o in offs)
    ends = [o + c * e for o, (c, e) in zip(offs, members)]
    assert all(end <= nxt for end, nxt in zip(ends, offs[1:] + [size]))          # in order, none reaches into the next
    assert size == sum(_up256(c * e) for c, e in members)
