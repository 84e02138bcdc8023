"""field_offsets_fit (csrc/field_offsets.h): whether the marching 3-D kernels' 32-bit byte offsets reach every zone of a Grid,
nc*8 + max(2 sK, sJ)*8 + 8 < 2^32 -- the function aa_create asks before it builds a 3-D Grid, compiled here with the host compiler
into fixtures/field_offsets_probe.cpp.  (tests/test_gpu_scalar_addressing.py runs the accessors themselves at the ends of the range.)"""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "atmospheric-athena_amd")
LIMIT = 1 << 32


@pytest.fixture(scope="module")
def fit(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("field_offsets") / "field_offsets_probe.so")
    subprocess.check_call(["g++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "fixtures", "field_offsets_probe.cpp"), "-o", so])
    L = C.CDLL(so)
    L.probe_field_offsets_fit.restype = C.c_int
    L.probe_field_offsets_fit.argtypes = [C.c_longlong] * 3
    return lambda nc, sJ, sK: bool(L.probe_field_offsets_fit(nc, sJ, sK))


def pool(n1, n2, n3, pad=True):
    """sJ, sK, nc as aa_create lays a Grid of n1 x n2 x n3 zones (ghost zones included) out"""
    sJ = (n1 + 15) // 16 * 16 if pad else n1
    return sJ * n2 * n3, sJ, sJ * n2


def test_the_headline_grid_fits(fit):
    nc, sJ, sK = pool(520, 520, 520)            # 512^3 and four ghost zones a side
    assert nc * 8 < LIMIT // 3                   # 1.2 GB a field
    assert fit(nc, sJ, sK) and fit(*pool(520, 520, 520, pad=False))
    assert fit(*pool(73, 13, 14)) and fit(1, 1, 1)


@pytest.mark.parametrize("sJ,n2", [(528, 520), (16, 16), (1040, 8)])
def test_just_below_and_just_above_the_limit(fit, sJ, n2):
    """nc steps by whole planes; the last plane count that keeps nc*8 + 2 sK*8 + 8 below 2^32 fits, the next one does not"""
    sK = sJ * n2
    far = max(2 * sK, sJ)
    n3 = (LIMIT - 8 - far * 8 - 1) // (8 * sK)              # the largest n3 with sK*n3*8 + far*8 + 8 <= 2^32 - 1
    assert fit(sK * n3, sJ, sK)
    assert not fit(sK * (n3 + 1), sJ, sK)
    # ... and zone by zone, whatever the planes: the bound itself
    nc_last = (LIMIT - 8 - far * 8 - 1) // 8
    assert nc_last * 8 + far * 8 + 8 < LIMIT <= (nc_last + 1) * 8 + far * 8 + 8
    assert fit(nc_last, sJ, sK) and not fit(nc_last + 1, sJ, sK)


def test_the_row_stride_counts_where_it_is_the_longer_hop(fit):
    """a Grid one row deep per plane pair: sJ > 2 sK cannot happen in the pool, but the rule is max(2 sK, sJ)"""
    nc = (LIMIT - 8) // 8 - 1000
    assert fit(nc, 999, 400) and not fit(nc, 1000, 400) and not fit(nc, 16, 500)


def test_what_cannot_be_a_grid_does_not_fit(fit):
    assert not fit(-1, 16, 256) and not fit(1 << 62, 16, 256) and not fit(1000, 16, 1 << 62)


def test_aa_create_asks_the_guard():
    """one code path: aa_create refuses, nothing falls back to other kernels"""
    src = open(os.path.join(PKG, "csrc", "api.hip")).read()
    assert '#include "field_offsets.h"' in src
    assert "!one_d && !two_d && !field_offsets_fit(d.nc, d.sJ, d.sK)" in src
