"""What the six public point-cloud functions do with their cloud arguments, in one table (no GPU needed).

Every function takes one cloud, a padded batch with row counts, or a list.  The refusals they share and the differences they keep are held
here side by side, through the public functions only; a new operator is added to OPS and to the table of differences below.

    |                                  | normals    | voxel      | knn / chamfer | fps        | ball       |
    | empty cloud, list of empty ones  | ValueError | ValueError | accepted      | accepted   | accepted   |
    | rows with N elements, not 1-D    | accepted   | accepted   | ValueError    | ValueError | ValueError |
    | rows (1 of them) with one cloud  | accepted   | accepted   | ValueError    | ValueError | ValueError |
    | k                                | 3..32      | -          | 1..32 (knn)   | 1..2^31-1  | 1..32      |

A refusal is a ValueError raised before any device work: on a machine without a GPU it must not turn into the "no HIP device" error.
"Accepted" means the argument checks let the call through: without a GPU it then ends in that error, with one it returns.
"""
import numpy as np
import pytest
import torch

from dicp_amd.ball import ball_query
from dicp_amd.fps import sample_farthest_points
from dicp_amd.knn import chamfer_distance, knn_points
from dicp_amd.normals import estimate_normals
from dicp_amd.voxel import voxel_downsample

HAVE_GPU = torch.cuda.is_available()


def _partner(arg):
    """a valid second cloud in the form of arg, as far as arg has one"""
    if isinstance(arg, (list, tuple)):
        return [torch.zeros(5, 3) for _ in arg] or [torch.zeros(5, 3)]
    if isinstance(arg, torch.Tensor) and arg.dim() == 3:
        return torch.zeros(arg.shape[0], 5, 3, dtype=arg.dtype if arg.dtype in (torch.float32, torch.float64) else torch.float32)
    return torch.zeros(5, 3, dtype=arg.dtype if isinstance(arg, torch.Tensor) and arg.dtype == torch.float64 else torch.float32)


def _two(fn, side, **fixed):
    def call(arg, rows=None, **kw):
        other = _partner(arg)
        if side == "x":
            return fn(arg, other, x_rows=rows, **fixed, **kw)
        return fn(other, arg, y_rows=rows, **fixed, **kw)
    return call


OPS = {
    "estimate_normals": lambda p, rows=None, k=4: estimate_normals(p, k=k, rows=rows),
    "voxel_downsample": lambda p, rows=None: voxel_downsample(p, 0.25, rows=rows),
    "sample_farthest_points": lambda p, rows=None, k=4: sample_farthest_points(p, k, rows=rows),
    "knn_points[x]": _two(knn_points, "x"), "knn_points[y]": _two(knn_points, "y"),
    "chamfer_distance[x]": _two(chamfer_distance, "x"), "chamfer_distance[y]": _two(chamfer_distance, "y"),
    "ball_query[x]": _two(ball_query, "x", radius=0.3), "ball_query[y]": _two(ball_query, "y", radius=0.3),
}
LENIENT = ("estimate_normals", "voxel_downsample")         # no empty clouds; rows of any shape with N elements
K_RANGE = {"estimate_normals": (3, 32), "sample_farthest_points": (1, 2 ** 31 - 1), "knn_points[x]": (1, 32), "ball_query[x]": (1, 32)}
ALL = sorted(OPS)


def _refused(op, *a, **kw):
    with pytest.raises(ValueError):
        OPS[op](*a, **kw)


def _accepted(op, *a, **kw):
    try:
        OPS[op](*a, **kw)
    except ValueError as e:
        pytest.fail("%s refused a valid argument: %s" % (op, e))
    except RuntimeError as e:
        assert not HAVE_GPU and "no HIP device" in str(e), e


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


REFUSED_POINTS = {
    "none": None, "numpy": np.zeros((10, 3), dtype=np.float32),
    "half": _z(10, 3, dtype=torch.float16), "bfloat16": _z(10, 3, dtype=torch.bfloat16), "int64": _z(10, 3, dtype=torch.int64),
    "int32_batch": _z(2, 10, 3, dtype=torch.int32), "complex": _z(10, 3, dtype=torch.complex64),
    "two_columns": _z(10, 2), "two_columns_batch": _z(2, 10, 2), "one_dim": _z(3), "four_dim": _z(1, 2, 10, 3), "no_clouds": _z(0, 10, 3),
    "empty_list": [], "empty_tuple": (), "list_of_batches": [_z(2, 5, 3)], "list_with_a_number": [_z(5, 3), 1.0],
    "list_with_half": [_z(5, 3), _z(5, 3, dtype=torch.float16)], "list_two_columns": [_z(5, 2), _z(6, 2)],
    "list_mixed_dtype": [_z(10, 3), _z(5, 3, dtype=torch.float64)], "list_mixed_columns": [_z(10, 3), _z(5, 4)],
}


@pytest.mark.parametrize("case", sorted(REFUSED_POINTS))
@pytest.mark.parametrize("op", ALL)
def test_invalid_clouds_are_refused(op, case):
    _refused(op, REFUSED_POINTS[case])


REFUSED_ROWS = {
    "with_a_list": ([_z(10, 3), _z(5, 3)], [10, 5]), "with_a_list_tensor": ([_z(10, 3)], torch.tensor([10])),
    "two_for_one_cloud": (_z(10, 3), [10, 10]),
    "too_few": (_z(2, 10, 3), [3]), "too_many": (_z(2, 10, 3), [3, 4, 5]), "scalar_for_two": (_z(2, 10, 3), torch.tensor(3)),
    "float": (_z(2, 10, 3), [1.0, 2.0]), "float64_tensor": (_z(2, 10, 3), torch.tensor([1.0, 2.0], dtype=torch.float64)),
    "bool": (_z(2, 10, 3), torch.tensor([True, False])),
    "above_m": (_z(2, 10, 3), [3, 11]), "negative": (_z(2, 10, 3), torch.tensor([-1, 3])), "above_m_int32": (_z(2, 10, 3), torch.tensor([11, 3], dtype=torch.int32)),
}


@pytest.mark.parametrize("case", sorted(REFUSED_ROWS))
@pytest.mark.parametrize("op", ALL)
def test_invalid_row_counts_are_refused(op, case):
    _refused(op, *REFUSED_ROWS[case])


@pytest.mark.parametrize("op", [o for o in ALL if o != "estimate_normals"])
def test_complex_row_counts_are_refused(op):
    """(estimate_normals does not refuse them by a ValueError of its own before the shared front end)"""
    _refused(op, _z(2, 10, 3), torch.tensor([3, 4], dtype=torch.complex64))


ACCEPTED = {
    "single": (_z(10, 3),), "single_f64": (_z(10, 3, dtype=torch.float64),), "batch": (_z(2, 10, 3),), "list": ([_z(10, 3), _z(5, 3)],), "tuple": ((_z(10, 3), _z(5, 3)),),
    "four_columns": (_z(10, 4),), "five_columns_batch": (_z(2, 10, 5),), "six_columns": (_z(10, 6),), "seven_columns_list": ([_z(10, 7), _z(4, 7)],),
    "rows_list": (_z(2, 10, 3), [3, 10]), "rows_zero": (_z(2, 10, 3), [0, 10]), "rows_int64": (_z(2, 10, 3), torch.tensor([10, 0])),
    "rows_uint8": (_z(2, 10, 3), torch.tensor([10, 4], dtype=torch.uint8)), "list_with_an_empty_cloud": ([_z(10, 3), _z(0, 3)],),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
@pytest.mark.parametrize("op", ALL)
def test_valid_clouds_pass_the_checks(op, case):
    _accepted(op, *ACCEPTED[case])


EMPTY = {"single": _z(0, 3), "batch": _z(2, 0, 3), "list": [_z(0, 3), _z(0, 3)], "six_columns": _z(0, 6)}


@pytest.mark.parametrize("case", sorted(EMPTY))
@pytest.mark.parametrize("op", ALL)
def test_empty_clouds(op, case):
    (_refused if op in LENIENT else _accepted)(op, EMPTY[case])


ROWS_NOT_1D = {"column": (_z(2, 10, 3), torch.tensor([[3], [4]])), "row": (_z(2, 10, 3), torch.tensor([[3, 4]])),
               "scalar_for_one": (_z(1, 10, 3), torch.tensor(3)), "one_for_one_cloud": (_z(10, 3), [10])}


@pytest.mark.parametrize("case", sorted(ROWS_NOT_1D))
@pytest.mark.parametrize("op", ALL)
def test_row_counts_that_are_not_one_per_cloud_in_one_dimension(op, case):
    (_accepted if op in LENIENT else _refused)(op, *ROWS_NOT_1D[case])


@pytest.mark.parametrize("op", sorted(K_RANGE))
def test_k_range(op):
    lo, hi = K_RANGE[op]
    for k in (lo - 1, hi + 1, -1, True, float(lo), "4", None, torch.tensor(4)):
        _refused(op, _z(40, 3), k=k)
    _accepted(op, _z(40, 3), k=lo)
    if hi <= 32 or not HAVE_GPU:                            # (on a GPU the largest k of sample_farthest_points would be sampled: 2^31 slots)
        _accepted(op, _z(40, 3), k=hi)


PAIRS = {
    "forms": (_z(10, 3), _z(1, 10, 3)), "forms_list": ([_z(10, 3)], _z(1, 10, 3)), "dtypes": (_z(10, 3), _z(10, 3, dtype=torch.float64)),
    "counts": (_z(2, 10, 3), _z(3, 10, 3)), "list_counts": ([_z(10, 3)], [_z(10, 3), _z(5, 3)]),
}


@pytest.mark.parametrize("case", sorted(PAIRS))
@pytest.mark.parametrize("fn", [knn_points, chamfer_distance, lambda x, y: ball_query(x, y, 0.3)], ids=["knn_points", "chamfer_distance", "ball_query"])
def test_clouds_that_do_not_go_together_are_refused(fn, case):
    with pytest.raises(ValueError):
        fn(*PAIRS[case])
