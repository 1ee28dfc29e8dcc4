"""Host side of the lockstep multi-vector Lanczos, without a GPU: the grouping
function of dmft-ed_amd/csrc/ed_lockstep_groups.hpp (a host-only header,
compiled here with plain g++ behind a small main) and the refusals of
ed_sector_hxv_multi / ed_sector_lanc_tridiag_lockstep that the arguments alone
decide, before any device call.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from edgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <vector>
#include "ed_lockstep_groups.hpp"
int main() {
  for (int n = 1; n <= 33; n++) {
    std::vector<int> first(edg::lockstep_max_groups(n)), width(first.size());
    const int g = edg::lockstep_groups(n, first.data(), width.data());
    if (g > (int)first.size()) return 1;
    std::printf("%d:", n);
    for (int k = 0; k < g; k++) std::printf(" %d,%d", first[k], width[k]);
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def groups(tmp_path_factory):
    d = tmp_path_factory.mktemp("lockstep")
    src, exe = d / "groups.cpp", d / "groups"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        n, rest = line.split(":")
        table[int(n)] = [tuple(int(t) for t in pair.split(",")) for pair in rest.split()]
    return table


def test_every_seed_is_covered_once_and_in_order(groups):
    assert sorted(groups) == list(range(1, 34))
    for n, gs in groups.items():
        seeds = [q for first, width in gs for q in range(first, first + width)]
        assert seeds == list(range(n)), (n, gs)


def test_widths_come_from_the_kernel_set_and_do_not_increase(groups):
    for n, gs in groups.items():
        widths = [w for _, w in gs]
        assert set(widths) <= {8, 4, 2, 1}, (n, widths)
        assert widths == sorted(widths, reverse=True), (n, widths)
        # the widest group that fits comes first: 8s, then the binary digits of the rest
        assert widths == [8] * (n // 8) + [w for w in (4, 2, 1) if (n % 8) & w], (n, widths)
    assert [w for _, w in groups[13]] == [8, 4, 1]


# ------------------------------------------------------------------ refusals
ERR_ARG = 1
P = ctypes.c_void_p


def _last():
    return _lib.load().ed_gpu_last_error().decode()


def test_hxv_multi_refuses_bad_arguments_before_any_device_call():
    """No sector exists here: every refusal below is decided by the arguments
    alone, and the blocks (host arrays standing in for device blocks) stay as
    they were."""
    lib = _lib.load()
    x, y = np.full(16, np.nan), np.full(16, np.nan)
    px, py = P(x.ctypes.data), P(y.ctypes.data)
    for nvec in (0, 3, 5, 16, -1):
        assert lib.ed_sector_hxv_multi(None, 0, nvec, px, py, None) == ERR_ARG
        assert "nvec" in _last()
    assert lib.ed_sector_hxv_multi(None, 2, 4, px, py, None) == ERR_ARG and "vtype" in _last()
    assert lib.ed_sector_hxv_multi(None, 0, 4, None, py, None) == ERR_ARG and "null" in _last()
    assert lib.ed_sector_hxv_multi(None, 0, 4, px, None, None) == ERR_ARG and "null" in _last()
    assert lib.ed_sector_hxv_multi(None, 0, 4, px, px, None) == ERR_ARG and "overlaps" in _last()
    assert lib.ed_sector_hxv_multi(None, 0, 4, px, py, None) == ERR_ARG and "null sector" in _last()
    assert np.all(np.isnan(x)) and np.all(np.isnan(y))


def test_lockstep_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    v = np.full(16, np.nan)
    a, b = np.full(8, np.nan), np.full(8, np.nan)
    n = np.full(2, -7, dtype=np.int32)
    pv, pa, pb, pn = (P(t.ctypes.data) for t in (v, a, b, n))
    assert lib.ed_sector_lanc_tridiag_lockstep(None, 0, 0, pv, 4, 1e-13, pa, pb, pn) == ERR_ARG and "nseed" in _last()
    assert lib.ed_sector_lanc_tridiag_lockstep(None, 0, 2, pv, 0, 1e-13, pa, pb, pn) == ERR_ARG and "nitermax" in _last()
    assert lib.ed_sector_lanc_tridiag_lockstep(None, 3, 2, pv, 4, 1e-13, pa, pb, pn) == ERR_ARG and "vtype" in _last()
    assert lib.ed_sector_lanc_tridiag_lockstep(None, 0, 2, pv, 4, 1e-13, pa, pb, pn) == ERR_ARG and "null" in _last()
    assert np.all(np.isnan(a)) and np.all(np.isnan(b)) and np.all(n == -7)
