"""The status codes of the FPFH entry points (include/dicp_hip.h: dicp_fpfh_spfh / dicp_fpfh_combine, dicp_fpfh_workspace_bytes) for every
class of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment
(5).  As tests/test_ransac_entry_codes.py: every call here is invalid, so nothing is launched.  The ValueErrors of the Python front end
(dicp_amd/fpfh.py), raised before any device work, are here too.
"""
import ctypes

import pytest
import torch

from dicp_amd import _lib
from dicp_amd.fpfh import compute_fpfh, fpfh_features

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


def test_workspace_bytes(lib):
    assert lib.dicp_fpfh_workspace_bytes(2, 3000) == 2 * 3000 * 48               # one 48-byte row per point (a multiple of 256 here)
    assert lib.dicp_fpfh_workspace_bytes(1, 1) == 256
    assert lib.dicp_fpfh_workspace_bytes(0, 10) == 0 and lib.dicp_fpfh_workspace_bytes(2, 0) == 0
    assert lib.dicp_fpfh_workspace_bytes(1 << 16, 1 << 15) == 0                  # N m = 2^31


def test_fpfh_spfh_entry(lib):
    # (dtype, points, c, normals, idx, idx64, rows, N, m, k, radius, workspace, workspace_bytes, spfh, stream)
    need = lib.dicp_fpfh_workspace_bytes(2, 3000)
    f = entry(lib.dicp_fpfh_spfh, [F32, OK, 3, OK, OK, 1, None, 2, 3000, 16, 0.0, OUT, need, None, None])
    all_equal(f, (1, 3, 4, 11), None, NULL)
    assert f(a6=OK, a13=OK, a1=P(4098)) == ALIGN                # rows and spfh are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=2) == ENUM and f(a5=-1) == ENUM
    assert f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a9=0) == SHAPE and f(a9=33) == SHAPE and f(a2=2) == SHAPE
    assert f(a9=32, a1=P(4098)) == ALIGN and f(a9=1, a1=P(4098)) == ALIGN and f(a2=7, a1=P(4098)) == ALIGN
    assert f(a7=1 << 16, a8=1 << 15, a12=BIG) == SHAPE
    for r in (-1.0, NAN, INF, -INF):
        assert f(a10=r) == SHAPE
    assert f(a10=0.5, a1=P(4098)) == ALIGN and f(a10=1e-200, a1=P(4098)) == ALIGN
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 3), P(4096 + 2), ALIGN)
    all_equal(f, (1, 3), P(4096 + 4), ALIGN, a0=F64)
    assert f(a4=P(4096 + 4)) == ALIGN and f(a4=P(4096 + 2), a5=0) == ALIGN and f(a6=P(4096 + 2)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a9=0) == DTYPE and f(a9=0, a1=P(4098)) == SHAPE


def test_fpfh_combine_entry(lib):
    # (dtype, points, c, idx, idx64, rows, N, m, k, radius, workspace, workspace_bytes, out, stream)
    need = lib.dicp_fpfh_workspace_bytes(2, 3000)
    f = entry(lib.dicp_fpfh_combine, [F32, OK, 3, OK, 1, None, 2, 3000, 16, 0.0, OUT, need, OK, None])
    all_equal(f, (1, 3, 10, 12), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a4=2) == ENUM
    assert f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a8=33) == SHAPE and f(a2=2) == SHAPE
    for r in (-1.0, NAN, INF):
        assert f(a9=r) == SHAPE
    assert f(a11=need - 1) == SHAPE and f(a11=need, a1=P(4098)) == ALIGN
    assert f(a10=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 12), P(4096 + 2), ALIGN)
    all_equal(f, (1, 12), P(4096 + 4), ALIGN, a0=F64)
    assert f(a3=P(4096 + 4)) == ALIGN and f(a3=P(4096 + 2), a4=0) == ALIGN and f(a5=P(4096 + 2)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a8=0) == DTYPE and f(a8=0, a1=P(4098)) == SHAPE


# ------------------------------------------------------------------ the Python front end: ValueError, no device touched
def test_fpfh_features_arguments():
    p, n, i = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 4, dtype=torch.int64)
    Pb, Nb, Ib = torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), torch.zeros(2, 5, 4, dtype=torch.int64)
    bad = [
        (p.half(), n.half(), i, {}),                                # dtypes
        (p, n.double(), i, {}),
        (p, n, i.float(), {}),
        (p, n, i.to(torch.int16), {}),
        (torch.zeros(5, 2), n, i, {}),                              # shapes
        (p, torch.zeros(5, 4), i, {}),
        (p, torch.zeros(4, 3), i, {}),
        (p, n, torch.zeros(4, 4, dtype=torch.int64), {}),           # not a self search
        (Pb, Nb, torch.zeros(2, 6, 4, dtype=torch.int64), {}),
        (p, n, torch.zeros(5, 0, dtype=torch.int64), {}),           # k
        (p, n, torch.zeros(5, 33, dtype=torch.int64), {}),
        (p, Nb, i, {}),                                             # forms
        (Pb, Nb, i, {}),
        (Pb, [n, n], Ib, {}),
        ([p, p], [n, n], Ib, {}),
        ([p, p], [n, n[:4]], [i, i], {}),
        ([p, p], [n, n], [i, i[:4]], {}),
        ([p, p], [n], [i, i], {}),
        (p, n.to("meta"), i, {}),                                   # devices
        (p, n, i.to("meta"), {}),
        (p, n, i, {"rows": torch.tensor([3])}),                     # rows
        (Pb, Nb, Ib, {"rows": torch.tensor([3, 6])}),
        (Pb, Nb, Ib, {"rows": torch.tensor([3.0, 2.0])}),
        ([p, p], [n, n], [i, i], {"rows": torch.tensor([3, 3])}),
        (torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int64), {}),
        (p, n, i, {"return_spfh": 1}),
        (p, "n", i, {}),
        (p, n, None, {}),
    ]
    bad += [(p, n, i, {"radius": r}) for r in (0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5), 10 ** 400)]
    for pts, nrm, idx, kw in bad:
        with pytest.raises(ValueError, match="fpfh_features"):
            fpfh_features(pts, nrm, idx, **kw)


def test_compute_fpfh_arguments():
    p, n = torch.zeros(5, 3), torch.zeros(5, 3)
    for r in (None, 0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5)):
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(p, n, r)
    for k in (0, 33, 8.0, True):
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(p, n, 0.5, k=k)
    for pts, nrm, kw in ((torch.zeros(5, 2), n, {}), (p, torch.zeros(5, 2), {}), (p, n.double(), {}), (p, torch.zeros(4, 3), {}),
                         (p, n, {"rows": torch.tensor([3])}), (torch.zeros(2, 5, 3), n, {})):
        with pytest.raises(ValueError, match="compute_fpfh"):
            compute_fpfh(pts, nrm, 0.5, **kw)
    with pytest.raises(ValueError, match="radius"):
        compute_fpfh(p, n, 1e-50)                                   # not > 0 in float32
