"""The status codes of the whole-ball ISS entry points (include/dicp_hip.h: dicp_iss_ball_saliency / dicp_iss_ball_maxima) for every class
of bad call, on a machine without a GPU: the checks run before any launch, in the order null (1), dtype (3), shape (2), alignment (5).
As tests/test_iss_entry_codes.py: every call here is invalid, so nothing is launched.  The ValueErrors of the Python front end
(dicp_amd/iss.py: iss_saliency_ball / iss_keypoints_ball / compute_iss_keypoints(whole_ball=)), raised before any device work, are here too.
"""
import ctypes

import pytest
import torch

from dicp_amd import _lib
from dicp_amd.iss import compute_iss_keypoints, iss_keypoints_ball, iss_saliency_ball

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
    assert "dicp_iss_ball_saliency" in _lib.EXPORTS and "dicp_iss_ball_maxima" in _lib.EXPORTS


def test_iss_ball_saliency_entry(lib):
    # (dtype, plans, keys, perm, rows4, N, m, radius, gamma21, gamma32, min_neighbors, workspace, workspace_bytes, saliency_out,
    #  eigenvalues_out, count_out, visited, stream)
    need = lib.dicp_iss_workspace_bytes(2, 3000)
    f = entry(lib.dicp_iss_ball_saliency, [F32, OK, OK, OK, OK, 2, 3000, 0.5, 0.975, 0.975, 5, OUT, need, OK, None, None, None, None])
    all_equal(f, (1, 2, 3, 4, 11), None, NULL)
    assert f(a13=None, a14=OK, a15=OK, a1=P(4098)) == ALIGN                       # the three outputs are optional
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=-1) == SHAPE and f(a6=(1 << 30) + 1, a12=BIG) == SHAPE
    assert f(a5=1 << 16, a6=1 << 15, a12=BIG) == SHAPE                            # N m = 2^31
    for r in (0.0, -1.0, NAN, INF, -INF, 1e200):                                  # (1e200: its square is not finite)
        assert f(a7=r) == SHAPE
    assert f(a7=1e-200, a1=P(4098)) == ALIGN and f(a7=1e150, a1=P(4098)) == ALIGN
    for g in (0.0, -0.5, 1.0000001, NAN, INF):
        assert f(a8=g) == SHAPE and f(a9=g) == SHAPE
    assert f(a8=1.0, a9=1e-300, a1=P(4098)) == ALIGN
    assert f(a10=0) == SHAPE and f(a10=-3) == SHAPE and f(a10=1, a1=P(4098)) == ALIGN
    assert f(a12=need - 1) == SHAPE and f(a12=need, a1=P(4098)) == ALIGN
    assert f(a11=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 2), P(4096 + 4), ALIGN)                                      # plans and keys: 8 bytes
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64) == ALIGN       # rows4: 4 elements
    all_equal(f, (13, 14), P(4096 + 2), ALIGN)
    all_equal(f, (13, 14), P(4096 + 4), ALIGN, a0=F64)
    assert f(a15=P(4096 + 2)) == ALIGN and f(a16=P(4096 + 4)) == ALIGN and f(a16=OK, a1=P(4098)) == ALIGN       # visited: optional, 8 bytes
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


def test_iss_ball_maxima_entry(lib):
    # (dtype, plans, keys, perm, rows4, N, m, radius, min_neighbors, workspace, workspace_bytes, mask_out, visited, stream)
    need = lib.dicp_iss_workspace_bytes(2, 3000)
    f = entry(lib.dicp_iss_ball_maxima, [F32, OK, OK, OK, OK, 2, 3000, 0.5, 5, OUT, need, OK, None, None])
    all_equal(f, (1, 2, 3, 4, 9, 11), None, NULL)
    assert f(a0=2) == DTYPE and f(a0=-1) == DTYPE
    assert f(a5=0) == SHAPE and f(a6=0) == SHAPE and f(a5=1 << 16, a6=1 << 15, a10=BIG) == SHAPE
    for r in (0.0, -1.0, NAN, INF, 1e200):
        assert f(a7=r) == SHAPE
    assert f(a8=0) == SHAPE and f(a8=1, a1=P(4098)) == ALIGN
    assert f(a10=need - 1) == SHAPE and f(a10=need, a1=P(4098)) == ALIGN
    assert f(a9=P(8192 + 128)) == ALIGN
    all_equal(f, (1, 2), P(4096 + 4), ALIGN)
    assert f(a3=P(4096 + 2)) == ALIGN and f(a4=P(4096 + 8)) == ALIGN and f(a4=P(4096 + 16), a0=F64) == ALIGN
    assert f(a11=P(4097), a1=P(4098)) == ALIGN                                    # (the mask is bytes: any address)
    assert f(a12=P(4096 + 4)) == ALIGN and f(a12=OK, a1=P(4098)) == ALIGN
    assert f(a1=None, a0=2) == NULL and f(a0=2, a6=0) == DTYPE and f(a6=0, a1=P(4098)) == SHAPE


# ------------------------------------------------------------------ the Python front end: ValueError, no device touched
def bad_clouds():
    p, Pb = torch.zeros(5, 3), torch.zeros(2, 5, 3)
    return [(p.half(), {}), (torch.zeros(5, 2), {}), ("p", {}), (torch.zeros(0, 3), {}), ([], {}), (torch.zeros(2, 2, 5, 3), {}),
            (p, {"rows": torch.tensor([3])}), (Pb, {"rows": torch.tensor([3, 6])}), (Pb, {"rows": torch.tensor([3.0, 2.0])}),
            ([p, p], {"rows": torch.tensor([3, 3])})] \
        + [(p, {g: v}) for g in ("gamma21", "gamma32") for v in (0.0, -0.1, 1.5, NAN, INF, "1", True, None, torch.tensor(0.5))] \
        + [(p, {"min_neighbors": v}) for v in (0, -1, 2.0, True, "5", None, 2 ** 31)]


BAD_RADII = (None, 0.0, -1.0, INF, NAN, "1", True, torch.tensor(0.5), 10 ** 400, 1e200)


def test_iss_saliency_ball_arguments():
    p = torch.zeros(5, 3)
    for pts, kw in bad_clouds() + [(p, {"return_eigenvalues": 1}), (p, {"return_counts": None})]:
        with pytest.raises(ValueError, match="iss_saliency_ball"):
            iss_saliency_ball(pts, 0.5, **kw)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="iss_saliency_ball"):
            iss_saliency_ball(p, r)


def test_iss_keypoints_ball_arguments():
    p = torch.zeros(5, 3)
    for pts, kw in bad_clouds() + [(p, {"return_saliency": 1})]:
        with pytest.raises(ValueError, match="iss_keypoints_ball"):
            iss_keypoints_ball(pts, 0.5, **kw)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="iss_keypoints_ball"):
            iss_keypoints_ball(p, r)
    for r in BAD_RADII[1:]:                                                        # (None: the salient radius)
        with pytest.raises(ValueError, match="iss_keypoints_ball"):
            iss_keypoints_ball(p, 0.5, non_max_radius=r)


def test_compute_iss_keypoints_whole_ball_arguments():
    p = torch.zeros(5, 3)
    for w in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, whole_ball=w)
    for r in BAD_RADII:
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, r, whole_ball=True)
    for r in BAD_RADII[1:]:
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, non_max_radius=r, whole_ball=True)
    for kw in ({"gamma21": 0.0}, {"min_neighbors": 0}, {"return_index": 1}, {"rows": torch.tensor([3])}):
        with pytest.raises(ValueError, match="compute_iss_keypoints"):
            compute_iss_keypoints(p, 0.5, whole_ball=True, **kw)
