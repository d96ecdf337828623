"""The status codes of the whole-ball normals entry points (include/dicp_hip.h: dicp_normals_ball_workspace_bytes / _forward / _records /
_gather) for every class of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3),
shape (2), alignment (5).  As tests/test_iss_ball_entry_codes.py: every call here is invalid, so nothing is launched.  The ValueErrors of
the Python front end (dicp_amd/normals.py: estimate_normals_ball), raised before any device work, are here too.
"""
import ctypes

import pytest
import torch

from dicp_amd import _lib
from dicp_amd.normals import estimate_normals_ball

NULL, SHAPE, DTYPE, ENUM, ALIGN = 1, 2, 3, 4, 5
F32, F64 = _lib.F32, _lib.F64
P = ctypes.c_void_p
OK = P(4096)
OUT = P(8192)
NAN, INF = float("nan"), float("inf")
BIG = 1 << 62


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def entry(fn, good):
    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert a != list(good), "a valid call would launch"
        return fn(*a)
    return call


def all_equal(call, positions, value, code, **kw):
    got = {i: call(**dict(kw, **{"a%d" % i: value})) for i in positions}
    assert got == {i: code for i in positions}


def test_the_abi_version_stays(lib):
    assert lib.dicp_abi_version() == 11 == _lib.ABI_VERSION
    for name in ("dicp_normals_ball_workspace_bytes", "dicp_normals_ball_forward", "dicp_normals_ball_records", "dicp_normals_ball_gather"):
        assert name in _lib.EXPORTS


def test_workspace_bytes(lib):
    f = lib.dicp_normals_ball_workspace_bytes
    slots = lib.dicp_ball_grid_slots(3000)
    assert f(2, 3000) == (2 * slots * 11 * 8 + 255) // 256 * 256 and f(1, 1) == 256          # 11 doubles a sorted slot, 2 slots at least
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 5) == 0 and f(5, -1) == 0 and f(1, (1 << 30) + 1) == 0
    assert f(1 << 16, 1 << 15) == 0 and f(1 << 15, (1 << 16) - 1) > 0                          # N m = 2^31; just below


def test_normals_ball_forward_entry(lib):
    # (dtype, plans, keys, perm, rows4, N, m, radius, min_neighbors, viewpoint, viewpoint_per_cloud, workspace, workspace_bytes, normals_out,
    #  curvature_out, eigenvalues_out, count_out, visited, stream)
    need = lib.dicp_normals_ball_workspace_bytes(2, 3000)
    f = entry(lib.dicp_normals_ball_forward, [F32, OK, OK, OK, OK, 2, 3000, 0.5, 3, None, 0, OUT, need, OK, None, None, None, None, None])
    all_equal(f, (1, 2, 3, 4, 11, 13), None, NULL)
    assert f(a9=OK, a14=OK, a15=OK, a16=OK, a1=P(4098)) == ALIGN                  # the viewpoint and three outputs are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=-1) == SHAPE and f(a6=(1 << 30) + 1, a12=BIG) == SHAPE
    assert f(a5=1 << 16, a6=1 << 15, a12=BIG) == SHAPE                            # N m = 2^31
    for r in (0.0, -1.0, NAN, INF, -INF, 1e200):                                  # (1e200: its square is not finite)
        assert f(a7=r) == SHAPE
    assert f(a7=1e-200, a1=P(4098)) == ALIGN and f(a7=1e150, a1=P(4098)) == ALIGN
    for n in (2, 1, 0, -3):
        assert f(a8=n) == SHAPE
    assert f(a8=4, a1=P(4098)) == ALIGN and f(a8=2 ** 31 - 1, a1=P(4098)) == ALIGN
    assert f(a10=2) == SHAPE and f(a10=-1) == SHAPE and f(a10=1, a1=P(4098)) == ALIGN
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 2), P(4096 + 4), ALIGN)                                      # plans and keys: 8 bytes
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64) == ALIGN       # rows4: 4 elements
    all_equal(f, (9, 13, 14, 15), P(4096 + 2), ALIGN)
    all_equal(f, (9, 13, 14, 15), P(4096 + 4), ALIGN, a0=F64)
    assert f(a16=P(4096 + 2)) == ALIGN and f(a17=P(4096 + 4)) == ALIGN and f(a17=OK, a1=P(4098)) == ALIGN       # visited: optional, 8 bytes
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


def test_normals_ball_records_entry(lib):
    # (dtype, plans, perm, rows4, N, m, g_normals, g_curvature, workspace, workspace_bytes, records, stream)
    need = lib.dicp_normals_ball_workspace_bytes(2, 3000)
    f = entry(lib.dicp_normals_ball_records, [F32, OK, OK, OK, 2, 3000, OK, None, OUT, need, OK, None])
    all_equal(f, (1, 2, 3, 8, 10), None, NULL)
    assert f(a6=None, a1=P(4098)) == ALIGN and f(a7=OK, a1=P(4098)) == ALIGN      # the cotangents are optional, each of them
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a4=0) == SHAPE and f(a5=0) == SHAPE and f(a4=-1) == SHAPE and f(a5=(1 << 30) + 1, a9=BIG) == SHAPE
    assert f(a4=1 << 16, a5=1 << 15, a9=BIG) == SHAPE
    assert f(a9=need - 1) == SHAPE and f(a9=need, a1=P(4098)) == ALIGN
    assert f(a8=P(8192 + 128)) == ALIGN
    assert f(a1=P(4096 + 4)) == ALIGN and f(a2=P(4096 + 2)) == ALIGN
    assert f(a3=P(4096 + 8)) == ALIGN and f(a3=P(4096 + 16), a0=F64) == ALIGN
    all_equal(f, (6, 7), P(4096 + 2), ALIGN)
    all_equal(f, (6, 7), P(4096 + 4), ALIGN, a0=F64)
    assert f(a10=P(4096 + 4)) == ALIGN                                            # the records are doubles
    assert f(a1=None, a0=2) == NULL and f(a0=2, a5=0) == DTYPE and f(a5=0, a1=P(4098)) == SHAPE


def test_normals_ball_gather_entry(lib):
    # (dtype, plans, keys, perm, rows4, N, m, c, radius, records, grad_out, visited, stream)
    f = entry(lib.dicp_normals_ball_gather, [F32, OK, OK, OK, OK, 2, 3000, 3, 0.5, OK, OUT, None, None])
    all_equal(f, (1, 2, 3, 4, 9, 10), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=-1) == SHAPE and f(a6=(1 << 30) + 1) == SHAPE
    assert f(a5=1 << 16, a6=1 << 15) == SHAPE
    for c in (2, 0, -1, 1 << 30):
        assert f(a7=c) == SHAPE
    assert f(a7=6, a1=P(4098)) == ALIGN
    for r in (0.0, -1.0, NAN, INF, 1e200):
        assert f(a8=r) == SHAPE
    all_equal(f, (1, 2, 9), P(4096 + 4), ALIGN)                                   # plans, keys and records: 8 bytes
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64) == ALIGN
    assert f(a10=P(8192 + 2)) == ALIGN and f(a10=P(8192 + 4), a0=F64) == ALIGN
    assert f(a11=P(4096 + 4)) == ALIGN and f(a11=OK, a1=P(4098)) == ALIGN         # visited: optional, 8 bytes
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


# ------------------------------------------------------------------ the Python front end: ValueError, no device touched
def bad_calls():
    p, Pb = torch.zeros(5, 3), torch.zeros(2, 5, 3)
    return [(p.half(), {}), (torch.zeros(5, 2), {}), ("p", {}), (torch.zeros(0, 3), {}), ([], {}), (torch.zeros(2, 2, 5, 3), {}),
            (Pb, {"rows": torch.tensor([3, 6])}), (Pb, {"rows": torch.tensor([3.0, 2.0])}), (Pb, {"rows": torch.tensor([3])}),
            ([p, p], {"rows": torch.tensor([3, 3])})] \
        + [(p, {"min_neighbors": v}) for v in (2, 0, -1, 3.0, True, "5", None, 2 ** 31)] \
        + [(p, {flag: v}) for flag in ("return_curvature", "return_eigenvalues", "return_counts") for v in (1, 0, None, "yes")] \
        + [(p, {"viewpoint": v}) for v in (torch.zeros(2), torch.zeros(2, 3), torch.zeros(3, dtype=torch.bool), torch.zeros(1, 3, 1))] \
        + [(Pb, {"viewpoint": torch.zeros(3, 3)})]


BAD_RADII = (None, 0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5), 10 ** 400, 1e200)


def test_estimate_normals_ball_arguments():
    p = torch.zeros(5, 3)
    for pts, kw in bad_calls():
        with pytest.raises(ValueError, match="estimate_normals_ball"):
            estimate_normals_ball(pts, 0.5, **kw)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="estimate_normals_ball"):
            estimate_normals_ball(p, r)
    with pytest.raises(TypeError):
        estimate_normals_ball(p)                                                  # the radius is required
