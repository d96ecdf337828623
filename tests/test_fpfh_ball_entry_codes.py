"""The status codes of the whole-ball FPFH entry points (include/dicp_hip.h: dicp_fpfh_ball_workspace_bytes / dicp_fpfh_ball_pack /
dicp_fpfh_ball_spfh / dicp_fpfh_ball_combine) for every class of bad call, on a machine without a GPU: the checks run before any launch,
in the order null (1), dtype (3), enum (4: the int64 flag of `at`), shape (2), alignment (5).  As tests/test_iss_ball_entry_codes.py:
every call here is invalid, so nothing is launched.  The ValueErrors of the Python front end (dicp_amd/fpfh.py: fpfh_features_ball /
compute_fpfh(whole_ball=, at=)), raised before any device work, are here too.
"""
import ctypes

import pytest
import torch

from dicp_amd import _lib
from dicp_amd.fpfh import compute_fpfh, fpfh_features_ball

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
    for name in ("dicp_fpfh_ball_workspace_bytes", "dicp_fpfh_ball_pack", "dicp_fpfh_ball_spfh", "dicp_fpfh_ball_combine"):
        assert name in _lib.EXPORTS


def test_workspace_bytes(lib):
    f = lib.dicp_fpfh_ball_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256                                          # noqa: E731
    assert f(F32, 2, 3000) == up(2 * 3000 * 34 * 8) + up(2 * 3000 * 16) + up(2 * 3000 * 4)
    assert f(F64, 2, 3000) == up(2 * 3000 * 34 * 8) + up(2 * 3000 * 32) + up(2 * 3000 * 4)
    assert f(F32, 1, 1) == 512 + 256 + 256                                         # (one row: 272 bytes of table)
    for bad in ((2, 2, 3000), (-1, 2, 3000), (F32, 0, 3000), (F32, 2, 0), (F32, -1, 5), (F32, 1 << 16, 1 << 15), (F32, 1, (1 << 30) + 1)):
        assert f(*bad) == 0


def test_fpfh_ball_pack_entry(lib):
    # (dtype, plans, perm, rows4, normals, N, m, workspace, workspace_bytes, stream)
    need = lib.dicp_fpfh_ball_workspace_bytes(F32, 2, 3000)
    f = entry(lib.dicp_fpfh_ball_pack, [F32, OK, OK, OK, OK, 2, 3000, OUT, need, None])
    all_equal(f, (1, 2, 3, 4, 7), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=-1) == SHAPE and f(a6=(1 << 30) + 1, a8=BIG) == SHAPE
    assert f(a5=1 << 16, a6=1 << 15, a8=BIG) == SHAPE                             # N m = 2^31
    assert f(a8=need - 1) == SHAPE and f(a8=need, a1=P(4098)) == ALIGN
    assert f(a0=F64) == SHAPE and f(a0=F64, a8=lib.dicp_fpfh_ball_workspace_bytes(F64, 2, 3000), a1=P(4098)) == ALIGN      # float64 needs more
    assert f(a7=P(8192 + 128)) == ALIGN
    assert f(a1=P(4096 + 4)) == ALIGN and f(a2=P(4096 + 2)) == ALIGN
    assert f(a3=P(4096 + 8)) == ALIGN and f(a3=P(4096 + 16), a0=F64, a8=BIG) == ALIGN                                      # rows4: 4 elements
    assert f(a4=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 4), a0=F64, a8=BIG) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


def test_fpfh_ball_spfh_entry(lib):
    # (dtype, plans, keys, perm, rows4, N, m, radius, workspace, workspace_bytes, spfh, visited, stream)
    need = lib.dicp_fpfh_ball_workspace_bytes(F32, 2, 3000)
    f = entry(lib.dicp_fpfh_ball_spfh, [F32, OK, OK, OK, OK, 2, 3000, 0.5, OUT, need, None, None, None])
    all_equal(f, (1, 2, 3, 4, 8), None, NULL)
    assert f(a10=OK, a1=P(4098)) == ALIGN                                         # spfh is optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=-1) == SHAPE and f(a6=(1 << 30) + 1, a9=BIG) == SHAPE
    assert f(a5=1 << 16, a6=1 << 15, a9=BIG) == SHAPE
    for r in (0.0, -1.0, NAN, INF, -INF, 1e200):                                  # (1e200: its square is not finite)
        assert f(a7=r) == SHAPE
    assert f(a7=1e-200, a1=P(4098)) == ALIGN and f(a7=1e150, a1=P(4098)) == ALIGN
    assert f(a9=need - 1) == SHAPE and f(a9=need, a1=P(4098)) == ALIGN
    assert f(a8=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 2), P(4096 + 4), ALIGN)                                      # plans and keys: 8 bytes
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64, a9=BIG) == ALIGN
    assert f(a10=P(4096 + 2)) == ALIGN and f(a11=P(4096 + 4)) == ALIGN and f(a11=OK, a1=P(4098)) == ALIGN      # visited: optional, 8 bytes
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


def test_fpfh_ball_combine_entry(lib):
    # (dtype, plans, keys, perm, rows4, at, at64, q, N, m, radius, workspace, workspace_bytes, out, visited, stream)
    need = lib.dicp_fpfh_ball_workspace_bytes(F32, 2, 3000)
    f = entry(lib.dicp_fpfh_ball_combine, [F32, OK, OK, OK, OK, None, 0, 0, 2, 3000, 0.5, OUT, need, OK, None, None])
    all_equal(f, (1, 2, 3, 4, 11, 13), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a6=2) == ENUM and f(a6=-1) == ENUM and f(a6=2, a5=OK, a7=5) == ENUM
    assert f(a6=1, a1=P(4098)) == ALIGN                                           # (the flag alone, without at: a valid value)
    assert f(a8=0) == SHAPE and f(a9=0) == SHAPE and f(a8=1 << 16, a9=1 << 15, a12=BIG) == SHAPE
    for r in (0.0, -1.0, NAN, INF, 1e200):
        assert f(a10=r) == SHAPE
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a7=1) == SHAPE and f(a7=-1) == SHAPE                                 # q without at
    assert f(a5=OK) == SHAPE and f(a5=OK, a7=-3) == SHAPE                         # at without q
    assert f(a5=OK, a7=1 << 30) == SHAPE and f(a5=OK, a7=(1 << 30) - 1, a1=P(4098)) == ALIGN      # N q = 2^31
    assert f(a5=P(4096 + 2), a7=5) == ALIGN and f(a5=P(4096 + 4), a7=5, a1=P(4098)) == ALIGN      # at: 4 bytes as int32 ...
    assert f(a5=P(4096 + 4), a6=1, a7=5) == ALIGN and f(a5=P(4096 + 8), a6=1, a7=5, a1=P(4098)) == ALIGN       # ... 8 as int64
    assert f(a11=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 2), P(4096 + 4), ALIGN)
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64, a12=BIG) == ALIGN
    assert f(a13=P(4096 + 2)) == ALIGN and f(a13=P(4096 + 4), a0=F64, a12=BIG) == ALIGN
    assert f(a14=P(4096 + 4)) == ALIGN and f(a14=OK, a1=P(4098)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=7) == DTYPE and f(a6=7, a9=0) == ENUM and f(a9=0, a1=P(4098)) == SHAPE


# ------------------------------------------------------------------ the Python front end: ValueError, no device touched
BAD_RADII = (None, 0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5), 10 ** 400, 1e200)


def bad_clouds():
    """(points, normals, keywords)"""
    p, n, Pb, Nb = torch.zeros(5, 3), torch.ones(5, 3), torch.zeros(2, 5, 3), torch.ones(2, 5, 3)
    return [(p.half(), n.half(), {}), (torch.zeros(5, 2), n, {}), ("p", n, {}), (torch.zeros(0, 3), torch.zeros(0, 3), {}), ([], [], {}),
            (torch.zeros(2, 2, 5, 3), n, {}), (p, n, {"rows": torch.tensor([3])}), (Pb, Nb, {"rows": torch.tensor([3, 6])}),
            (Pb, Nb, {"rows": torch.tensor([3.0, 2.0])}), ([p, p], [n, n], {"rows": torch.tensor([3, 3])}),
            (p, n.double(), {}), (p, torch.ones(5, 4), {}), (p, torch.ones(4, 3), {}), (p, Nb, {}), (Pb, n, {}), (p, "n", {}), ([p, p], [n], {}),
            ([p, p], [n, torch.ones(4, 3)], {})]


def bad_at():
    """(points, normals, at)"""
    p, n, Pb, Nb = torch.zeros(5, 3), torch.ones(5, 3), torch.zeros(2, 5, 3), torch.ones(2, 5, 3)
    i = torch.tensor([0, 1])
    return [(p, n, [0, 1]), (p, n, "at"), (p, n, i.float()), (p, n, i.bool()), (p, n, i.to(torch.int16)), (p, n, i.reshape(1, 2)),
            (p, n, torch.zeros(0, dtype=torch.int64)), (p, n, torch.tensor(1)), (Pb, Nb, i), (Pb, Nb, torch.zeros(3, 2, dtype=torch.int64)),
            (Pb, Nb, torch.zeros(2, 0, dtype=torch.int32)), (Pb, Nb, torch.zeros(2, 2, 2, dtype=torch.int64)), (Pb, Nb, [i, i]), ([p, p], [n, n], i),
            ([p, p], [n, n], [i]), ([p, p], [n, n], [i, i.int()]), ([p, p], [n, n], [i, i.reshape(1, 2)]), ([p, p], [n, n], [i, "x"]), ([p, p], [n, n], []),
            (p, n, i.to("meta"))]


def test_fpfh_features_ball_arguments():
    p, n = torch.zeros(5, 3), torch.ones(5, 3)
    for pts, nrm, kw in bad_clouds() + [(p, n, {"return_spfh": 1}), (p, n, {"return_spfh": None})]:
        with pytest.raises(ValueError, match="fpfh_features_ball"):
            fpfh_features_ball(pts, nrm, 0.5, **kw)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="fpfh_features_ball"):
            fpfh_features_ball(p, n, r)
    for pts, nrm, at in bad_at():
        with pytest.raises(ValueError, match="fpfh_features_ball"):
            fpfh_features_ball(pts, nrm, 0.5, at=at)


def test_compute_fpfh_whole_ball_arguments():
    p, n = torch.zeros(5, 3), torch.ones(5, 3)
    for w in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(p, n, 0.5, whole_ball=w)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(p, n, r, whole_ball=True)
    for pts, nrm, kw in bad_clouds() + [(p, n, {"k": 0}), (p, n, {"k": 33}), (p, n, {"k": 2.0})]:
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(pts, nrm, 0.5, whole_ball=True, **kw)
    for pts, nrm, at in bad_at():
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(pts, nrm, 0.5, whole_ball=True, at=at)
    at = torch.tensor([0, 1])
    for kw in ({}, {"whole_ball": False}, {"k": 8}):
        with pytest.raises(ValueError, match="compute_fpfh.*whole_ball=True"):
            compute_fpfh(p, n, 0.5, at=at, **kw)                                   # at without whole_ball: the k-slot form is not touched
