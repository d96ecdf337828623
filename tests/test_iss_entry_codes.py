"""The status codes of the ISS entry points (include/dicp_hip.h: dicp_iss_saliency / dicp_iss_maxima, dicp_iss_workspace_bytes) for every
class of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment
(5).  As tests/test_fpfh_entry_codes.py: every call here is invalid, so nothing is launched.  The ValueErrors of the Python front end
(dicp_amd/iss.py), raised before any device work, are here too.
"""
import ctypes

import pytest
import torch

from dicp_amd import _lib
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints, iss_saliency

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
    assert lib.dicp_iss_workspace_bytes(2, 3200) == 2 * 3200 * 8                 # one double per point (a multiple of 256 here)
    assert lib.dicp_iss_workspace_bytes(2, 3000) == 48128                        # rounded up to 256
    assert lib.dicp_iss_workspace_bytes(1, 1) == 256 and lib.dicp_iss_workspace_bytes(3, 33) == 1024
    assert lib.dicp_iss_workspace_bytes(0, 10) == 0 and lib.dicp_iss_workspace_bytes(2, 0) == 0 and lib.dicp_iss_workspace_bytes(-1, 5) == 0
    assert lib.dicp_iss_workspace_bytes(1 << 16, 1 << 15) == 0                   # N m = 2^31
    assert lib.dicp_iss_workspace_bytes(1, (1 << 31) - 1) == ((((1 << 31) - 1) * 8 + 255) // 256) * 256


def test_iss_saliency_entry(lib):
    # (dtype, points, c, idx, idx64, rows, N, m, k, radius, gamma21, gamma32, min_neighbors, workspace, workspace_bytes, saliency_out,
    #  eigenvalues_out, count_out, stream)
    need = lib.dicp_iss_workspace_bytes(2, 3000)
    f = entry(lib.dicp_iss_saliency, [F32, OK, 3, OK, 1, None, 2, 3000, 16, 0.0, 0.975, 0.975, 5, OUT, need, OK, None, None, None])
    all_equal(f, (1, 3, 13), None, NULL)
    assert f(a5=OK, a15=None, a16=OK, a17=OK, a1=P(4098)) == ALIGN                # rows and the three outputs are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a4=2) == ENUM and f(a4=-1) == ENUM
    assert f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a8=33) == SHAPE and f(a2=2) == SHAPE
    assert f(a8=32, a1=P(4098)) == ALIGN and f(a8=1, a1=P(4098)) == ALIGN and f(a2=7, a1=P(4098)) == ALIGN
    assert f(a6=1 << 16, a7=1 << 15, a14=BIG) == SHAPE
    for r in (-1.0, NAN, INF, -INF):
        assert f(a9=r) == SHAPE
    assert f(a9=0.5, a1=P(4098)) == ALIGN and f(a9=1e-200, a1=P(4098)) == ALIGN
    for g in (0.0, -0.5, 1.0000001, NAN, INF):
        assert f(a10=g) == SHAPE and f(a11=g) == SHAPE
    assert f(a10=1.0, a11=1e-300, a1=P(4098)) == ALIGN
    assert f(a12=0) == SHAPE and f(a12=-3) == SHAPE and f(a12=1, a1=P(4098)) == ALIGN
    assert f(a14=need - 1) == SHAPE and f(a14=need, a1=P(4098)) == ALIGN
    assert f(a13=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 15, 16), P(4096 + 2), ALIGN)
    all_equal(f, (1, 15, 16), P(4096 + 4), ALIGN, a0=F64)
    assert f(a17=P(4096 + 2)) == ALIGN
    assert f(a3=P(4096 + 4)) == ALIGN and f(a3=P(4096 + 2), a4=0) == ALIGN and f(a5=P(4096 + 2)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a8=0) == DTYPE and f(a8=0, a1=P(4098)) == SHAPE


def test_iss_maxima_entry(lib):
    # (dtype, points, c, idx, idx64, rows, N, m, k, radius, min_neighbors, workspace, workspace_bytes, mask_out, stream)
    need = lib.dicp_iss_workspace_bytes(2, 3000)
    f = entry(lib.dicp_iss_maxima, [F32, OK, 3, OK, 1, None, 2, 3000, 16, 0.0, 5, OUT, need, OK, None])
    all_equal(f, (1, 3, 11, 13), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a4=2) == ENUM
    assert f(a6=0) == SHAPE and f(a7=0) == SHAPE and f(a8=0) == SHAPE and f(a8=33) == SHAPE and f(a2=2) == SHAPE
    assert f(a6=1 << 16, a7=1 << 15, a12=BIG) == SHAPE
    for r in (-1.0, NAN, INF):
        assert f(a9=r) == SHAPE
    assert f(a10=0) == SHAPE and f(a10=1, a1=P(4098)) == ALIGN
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(8192 + 128)) == ALIGN
    assert f(a1=P(4096 + 2)) == ALIGN and f(a1=P(4096 + 4), a0=F64) == ALIGN
    assert f(a3=P(4096 + 4)) == ALIGN and f(a3=P(4096 + 2), a4=0) == ALIGN and f(a5=P(4096 + 2)) == ALIGN
    assert f(a13=P(4097), a1=P(4098)) == ALIGN                                    # (the mask is bytes: any address)
    assert f(a1=None, a0=2) == NULL and f(a0=2, a8=0) == DTYPE and f(a8=0, a1=P(4098)) == SHAPE


# ------------------------------------------------------------------ the Python front end: ValueError, no device touched
def bad_clouds():
    p, i = torch.zeros(5, 3), torch.zeros(5, 4, dtype=torch.int64)
    Pb, Ib = torch.zeros(2, 5, 3), torch.zeros(2, 5, 4, dtype=torch.int64)
    return [
        (p.half(), i, {}),                                          # dtypes
        (p, i.float(), {}),
        (p, i.to(torch.int16), {}),
        (torch.zeros(5, 2), i, {}),                                 # shapes
        (p, torch.zeros(4, 4, dtype=torch.int64), {}),              # not a self search: one row of slots per point
        (Pb, torch.zeros(2, 6, 4, dtype=torch.int64), {}),
        (p, torch.zeros(5, 0, dtype=torch.int64), {}),              # k
        (p, torch.zeros(5, 33, dtype=torch.int64), {}),
        (Pb, i, {}),                                                # forms
        (p, Ib, {}),
        ([p, p], Ib, {}),
        ([p, p], [i, i[:4]], {}),
        ([p, p], [i], {}),
        (p, i.to("meta"), {}),                                      # devices
        (p, i, {"rows": torch.tensor([3])}),                        # rows
        (Pb, Ib, {"rows": torch.tensor([3, 6])}),
        (Pb, Ib, {"rows": torch.tensor([3.0, 2.0])}),
        ([p, p], [i, i], {"rows": torch.tensor([3, 3])}),
        (torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int64), {}),
        ("p", i, {}),
        (p, None, {}),
    ] + [(p, i, {g: v}) for g in ("gamma21", "gamma32") for v in (0.0, -0.1, 1.5, NAN, INF, "1", True, None, torch.tensor(0.5))] \
      + [(p, i, {"min_neighbors": v}) for v in (0, -1, 2.0, True, "5", None, 2 ** 31)]


BAD_RADII = (0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5), 10 ** 400)


def test_iss_saliency_arguments():
    p, i = torch.zeros(5, 3), torch.zeros(5, 4, dtype=torch.int64)
    bad = bad_clouds() + [(p, i, {"radius": r}) for r in BAD_RADII] + [(p, i, {"return_eigenvalues": 1}), (p, i, {"return_counts": None})]
    for pts, idx, kw in bad:
        with pytest.raises(ValueError, match="iss_saliency"):
            iss_saliency(pts, idx, **kw)


def test_iss_keypoints_arguments():
    p, i = torch.zeros(5, 3), torch.zeros(5, 4, dtype=torch.int64)
    bad = bad_clouds() + [(p, i, {name: r}) for name in ("salient_radius", "non_max_radius") for r in BAD_RADII]
    bad += [(p, i, {"return_saliency": 1}),
            (p, i, {"nms_idx": torch.zeros(4, 4, dtype=torch.int64)}), (p, i, {"nms_idx": torch.zeros(5, 33, dtype=torch.int64)}),
            (p, i, {"nms_idx": torch.zeros(5, 4)}), (p, i, {"nms_idx": [i]}), (p, i, {"nms_idx": torch.zeros(1, 5, 4, dtype=torch.int64)}),
            ([p, p], [i, i], {"nms_idx": [i, i[:3]]}), (p, i, {"nms_idx": "idx"})]
    for pts, idx, kw in bad:
        with pytest.raises(ValueError, match="iss_keypoints"):
            iss_keypoints(pts, idx, **kw)


def test_compute_iss_keypoints_arguments():
    p = torch.zeros(5, 3)
    for r in (None,) + BAD_RADII:
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, r)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, non_max_radius=r)
    for k in (0, 33, 8.0, True):
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, k=k)
    for kw in ({"gamma21": 0.0}, {"gamma32": 1.5}, {"gamma21": True}, {"min_neighbors": 0}, {"min_neighbors": 2.5}, {"return_index": 1},
               {"rows": torch.tensor([3])}):
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, **kw)
    for pts in (torch.zeros(5, 2), p.half(), "p", torch.zeros(0, 3), [], torch.zeros(2, 2, 5, 3)):
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(pts, 0.5)
