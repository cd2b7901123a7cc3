"""``multi_dot`` and ``lincomb`` (csrc/lbfgs.hip) on the GPU: the bodies of test_lbfgs_kernels.py
on ``cuda`` (integer data bitwise against int64, normal data within the derived bounds, every
row-count branch, float4 / float4 + tail / scalar layouts, NaN all around), what the extension
refuses, and the unbounded device L-BFGS run to its gradient tolerance on the HIP kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lbfgs_kernels as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("layout,n", T.EXACT_CASES)
def test_multi_dot_exact(layout, n):
    T.check_multi_dot_exact(DEV, layout, n)


@pytest.mark.parametrize("layout", ["b", "c"])
@pytest.mark.parametrize("n,rows", T.TWO_TRIPS)
def test_multi_dot_exact_second_trip(n, rows, layout):
    """The grid-stride loop's second trip: n beyond 4 * 2048 blocks * lanes per chunk set."""
    T.check_multi_dot_exact(DEV, layout, n, rows=rows, ncs=T.TWO_TRIPS_NCS)


@pytest.mark.parametrize("layout,n", T.BOUND_CASES)
def test_multi_dot_bound(layout, n):
    T.check_multi_dot_bound(DEV, layout, n)


def test_bound_has_teeth():
    T.check_bound_has_teeth(DEV)


@pytest.mark.parametrize("layout", T.LINCOMB_LAYOUTS)
@pytest.mark.parametrize("n", T.LINCOMB_N)
@pytest.mark.parametrize("kind", ["int", "normal"])
def test_lincomb(kind, n, layout):
    T.check_lincomb(DEV, kind, layout, n)


def test_lincomb_refuses_257_rows():
    T.check_lincomb_refuses_257_rows(DEV)


def test_the_extension_refuses_bad_arguments():
    T.check_refuses_bad_arguments(DEV)


@pytest.mark.parametrize("m", [1, 10, 120])
@pytest.mark.parametrize("n", [1027, 1028])
def test_lbfgs_reaches_gtol(n, m):
    """n = 1027: the scalar path, 1028: float4; m = 120: 243 rows in 8 row groups."""
    T.check_lbfgs_reaches_gtol(DEV, n, m)
