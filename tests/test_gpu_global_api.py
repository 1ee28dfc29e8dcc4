"""The reference-shaped global API at the end of csrc/ed_lib.hip (ed_gpu_init,
ed_gpu_build_sector, ed_gpu_hxv, ed_gpu_eigh, ...) through ctypes: its
products on every ed_mode, and its state machine — rebuild on a live sector,
calls with no sector, finalize then build, Nloc mismatches, the ncv clamp of
ed_gpu_eigh.  Every error case is one the library refuses by a host-side check
before any launch."""
import ctypes

import numpy as np
import pytest

import cases
from edgpu import _lib
from edgpu._lib import ED_DIRECT, ED_STORED, SectorInfo
from edgpu.hamiltonian import Sector
from oracle.oracle import Oracle, spmv, start_vector

pytestmark = pytest.mark.gpu

ED_OK, ED_ERR_ARG, ED_ERR_STATE = 0, 1, 2
SMALL = [("c2", cases.c2, (3, 5)), ("superc", cases.superc, (1, 0)), ("nonsu2_replica", cases.nonsu2_replica, (4, 0))]
SENTINEL = -7.25


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class Api:
    def __init__(self):
        self.lib = _lib.load()
        self._params = None

    def init(self, cfg):
        self._params = cfg.to_ctypes()
        return self.lib.ed_gpu_init(ctypes.byref(self._params))

    def build(self, q1, q2, flags=ED_STORED):
        dim = ctypes.c_int64(-1)
        rc = self.lib.ed_gpu_build_sector(q1, q2, flags, ctypes.byref(dim))
        return rc, dim.value

    def build_rows(self, q1, q2, row0, nrows, flags=ED_STORED):
        dim = ctypes.c_int64(-1)
        rc = self.lib.ed_gpu_build_sector_rows(q1, q2, flags, row0, nrows, ctypes.byref(dim))
        return rc, dim.value

    def vecdim(self):
        n = ctypes.c_int32(-1)
        return self.lib.ed_gpu_vecdim(ctypes.byref(n)), n.value

    def hxv(self, nloc, v, hv, mpi=False):
        fn = self.lib.ed_gpu_hxv_mpi if mpi else self.lib.ed_gpu_hxv
        return fn(ctypes.byref(ctypes.c_int32(nloc)), _ptr(v), _ptr(hv))

    def eigh(self, neigen, nblock, nitermax, dim, v0=None):
        ev = np.full(neigen, SENTINEL)
        vec = np.zeros((neigen, dim), dtype=np.complex128)
        nconv = ctypes.c_int32(-1)
        rc = self.lib.ed_gpu_eigh(neigen, nblock, nitermax, 1e-12, None if v0 is None else _ptr(v0), _ptr(ev),
                                  _ptr(vec), ctypes.byref(nconv))
        return rc, ev, vec, nconv.value

    def current(self):
        h = ctypes.c_void_p()
        rc = self.lib.ed_gpu_current_sector(ctypes.byref(h))
        return rc, h

    def info(self):
        rc, h = self.current()
        assert rc == ED_OK and h.value
        info = SectorInfo()
        assert self.lib.ed_sector_get_info(h, ctypes.byref(info)) == ED_OK
        return info

    def last_error(self):
        return self.lib.ed_gpu_last_error().decode()


@pytest.fixture
def api():
    a = Api()
    assert a.lib.ed_gpu_finalize() == ED_OK      # whatever an earlier test left
    yield a
    assert a.lib.ed_gpu_finalize() == ED_OK


def _dense(cfg, q1, q2):
    orc = Oracle(cfg)
    hmap = orc.build_sector(q1, q2)
    csr = orc.build_csr(hmap)
    return csr, np.array([spmv(csr, col) for col in np.eye(len(hmap))]).T


@pytest.mark.parametrize("name", [c[0] for c in SMALL])
def test_global_hxv_equals_the_handle_api_and_the_oracle(api, name):
    _, factory, (q1, q2) = next(c for c in SMALL if c[0] == name)
    cfg = factory()
    orc = Oracle(cfg)
    csr = orc.build_csr(orc.build_sector(q1, q2))
    assert api.init(cfg) == ED_OK
    rc, dim = api.build(q1, q2)
    assert rc == ED_OK and dim == len(csr[0]) - 1
    assert api.vecdim() == (ED_OK, dim)
    x = start_vector(dim)
    hv = np.full(dim, SENTINEL, dtype=np.complex128)
    assert api.hxv(dim, x, hv) == ED_OK
    with Sector(cfg, q1, q2, stored=True) as S:
        np.testing.assert_array_equal(hv, S.hxv(x))
        np.testing.assert_array_equal(hv, spmv(csr, x))
        info = api.info()                                  # ed_gpu_current_sector: a live handle
        for f in ("dim", "nnz", "ns", "mode", "q1", "q2", "flags", "row0", "nrows"):
            assert getattr(info, f) == getattr(S.info, f), f
        assert (info.q1, info.q2 if cfg.ed_mode == "normal" else 0) == (q1, q2)
    nnz = ctypes.c_int64(-1)
    assert api.lib.ed_gpu_nnz(ctypes.byref(nnz)) == ED_OK and nnz.value == len(csr[1])
    rp, cols, vals = np.zeros(dim + 1, np.int64), np.zeros(nnz.value, np.int32), np.zeros(nnz.value, np.complex128)
    assert api.lib.ed_gpu_dump_csr(_ptr(rp), _ptr(cols), _ptr(vals)) == ED_OK
    for got, want in zip((rp, cols, vals), csr):
        np.testing.assert_array_equal(got, want)


def test_build_on_a_live_sector_replaces_it_and_frees_it(api):
    import torch

    cfg = cases.c2()
    assert api.init(cfg) == ED_OK
    assert api.build(0, 8) == (ED_OK, 1)
    assert api.info().dim == 1
    assert api.build(3, 5) == (ED_OK, 3136)            # replaces the live (0,8) sector
    # the current handle is the new sector, not a stale one (its address says
    # nothing: the allocator may hand the freed sector's block out again)
    info = api.info()
    assert (info.dim, info.q1, info.q2, info.nrows) == (3136, 3, 5, 3136)
    assert api.vecdim() == (ED_OK, 3136)
    x = start_vector(3136)
    hv = np.zeros(3136, dtype=np.complex128)
    assert api.hxv(3136, x, hv) == ED_OK
    bytes_one = api.info().device_bytes                 # with the staging vectors of ed_gpu_hxv
    assert bytes_one > 3136 * 16
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):                                 # each build frees the sector before it
        assert api.build(3, 5) == (ED_OK, 3136)
        assert api.hxv(3136, x, hv) == ED_OK
    assert api.info().device_bytes == bytes_one
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    print(f"free memory before {free0}, after 50 rebuilds {free1}, one sector {bytes_one} bytes")
    assert free0 - free1 <= bytes_one                   # a leaking sector_free would hold 50 of them


def test_every_entry_point_refuses_without_a_sector(api):
    cfg = cases.superc()
    lib = api.lib
    assert api.build(1, 0)[0] == ED_ERR_STATE and "ed_gpu_init" in api.last_error()      # not even params
    assert api.init(cfg) == ED_OK
    buf = np.full(64, SENTINEL, dtype=np.complex128)
    out = np.full(64, SENTINEL, dtype=np.complex128)
    a, b = np.zeros(8), np.zeros(8)
    i32, i64, f64 = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_double(SENTINEL)
    calls = {
        "ed_gpu_vecdim": lambda: lib.ed_gpu_vecdim(ctypes.byref(i32)),
        "ed_gpu_hxv": lambda: api.hxv(64, buf, out),
        "ed_gpu_hxv_mpi": lambda: api.hxv(64, buf, out, mpi=True),
        "ed_gpu_nnz": lambda: lib.ed_gpu_nnz(ctypes.byref(i64)),
        "ed_gpu_dump_csr": lambda: lib.ed_gpu_dump_csr(_ptr(a), _ptr(b), _ptr(out)),
        "ed_gpu_lanc_eigh": lambda: lib.ed_gpu_lanc_eigh(64, 1e-12, 10, ctypes.byref(f64), _ptr(out), ctypes.byref(i32)),
        "ed_gpu_eigh": lambda: lib.ed_gpu_eigh(2, 23, 64, 1e-12, _ptr(buf), _ptr(a), _ptr(out), ctypes.byref(i32)),
        "ed_gpu_lanc_tridiag": lambda: lib.ed_gpu_lanc_tridiag(_ptr(buf), 8, 1e-13, _ptr(a), _ptr(b), ctypes.byref(i32)),
        "ed_gpu_current_sector": lambda: api.current()[0],
    }
    entry = [n for n in _lib.SIGNATURES if n.startswith("ed_gpu_")]
    stateless = {"ed_gpu_init", "ed_gpu_set_device", "ed_gpu_build_sector", "ed_gpu_build_sector_rows",
                 "ed_gpu_mpi_split", "ed_gpu_delete_sector", "ed_gpu_finalize", "ed_gpu_last_error"}
    assert set(calls) == set(entry) - stateless           # a new entry point needs its case here
    for name, call in calls.items():
        assert call() == ED_ERR_STATE, name
        assert api.last_error(), name
    assert np.all(out == SENTINEL) and not a.any() and not b.any()
    assert (i32.value, i64.value, f64.value) == (-1, -1, SENTINEL)


def test_finalize_then_build_needs_init_again(api):
    cfg = cases.superc()
    assert api.init(cfg) == ED_OK
    assert api.build(1, 0) == (ED_OK, 210)
    assert api.lib.ed_gpu_finalize() == ED_OK
    assert api.current()[0] == ED_ERR_STATE                # finalize dropped the sector
    rc, _ = api.build(1, 0)
    assert rc == ED_ERR_STATE and api.last_error()
    assert api.build_rows(1, 0, 0, 10)[0] == ED_ERR_STATE
    assert api.init(cfg) == ED_OK
    assert api.build(1, 0) == (ED_OK, 210)
    assert api.lib.ed_gpu_delete_sector() == ED_OK
    assert api.lib.ed_gpu_delete_sector() == ED_OK         # delete_Hv_sector twice
    assert api.current()[0] == ED_ERR_STATE
    assert api.build(1, 0) == (ED_OK, 210)                 # the parameters survive delete_sector


@pytest.mark.parametrize("flags", [ED_STORED, ED_DIRECT])
def test_nloc_mismatch_leaves_hv_untouched(api, flags):
    cfg = cases.nonsu2_replica()
    q1, q2 = 4, 0
    csr, _ = _dense(cfg, q1, q2)
    dim = 70
    x = start_vector(dim)
    ref = spmv(csr, x)
    assert api.init(cfg) == ED_OK
    assert api.build(q1, q2, flags) == (ED_OK, dim)
    for mpi in (False, True):                              # a whole sector holds dim rows
        for nloc in (dim - 1, dim + 1, 0):
            hv = np.full(dim + 1, SENTINEL, dtype=np.complex128)
            assert api.hxv(nloc, x, hv, mpi=mpi) == ED_ERR_ARG, (mpi, nloc)
            assert "Nloc" in api.last_error()
            assert np.all(hv == SENTINEL)
        hv = np.full(dim + 1, SENTINEL, dtype=np.complex128)
        assert api.hxv(dim, x, hv, mpi=mpi) == ED_OK
        np.testing.assert_array_equal(hv[:dim], ref)
        assert hv[dim] == SENTINEL
    # a true row block [20, 45): Nloc is the rows held, the vector the whole sector's
    assert api.build_rows(q1, q2, 20, 25, flags) == (ED_OK, dim)
    assert api.vecdim() == (ED_OK, 25)
    for nloc in (dim, 24, 26, 0):
        hv = np.full(dim, SENTINEL, dtype=np.complex128)
        assert api.hxv(nloc, x, hv, mpi=True) == ED_ERR_ARG, nloc
        assert np.all(hv == SENTINEL)
    hv = np.full(dim, SENTINEL, dtype=np.complex128)
    assert api.hxv(dim, x, hv) != ED_OK                    # cc_sparse_HxV needs the whole sector
    assert np.all(hv == SENTINEL)
    assert api.hxv(25, x, hv, mpi=True) == ED_OK
    np.testing.assert_array_equal(hv[:25], ref[20:45])
    assert np.all(hv[25:] == SENTINEL)
    # a rank without rows (dim < MpiSize): vecDim 0, the product a no-op
    for row0 in (0, dim):
        assert api.build_rows(q1, q2, row0, 0, flags) == (ED_OK, dim)
        assert api.vecdim() == (ED_OK, 0)
        hv = np.full(dim, SENTINEL, dtype=np.complex128)
        assert api.hxv(0, x, hv, mpi=True) == ED_OK
        assert np.all(hv == SENTINEL)
        assert api.hxv(1, x, hv, mpi=True) == ED_ERR_ARG
    assert api.build_rows(q1, q2, dim - 3, 4, flags)[0] == ED_ERR_ARG       # rows beyond the sector
    assert api.current()[0] == ED_ERR_STATE                                  # and no sector is left behind


def test_eigh_ncv_clamp(api):
    cfg = cases.nonsu2_replica()
    q1, q2, dim = 4, 0, 70
    _, A = _dense(cfg, q1, q2)
    assert np.max(np.abs(A - A.conj().T)) < 1e-14
    w = np.linalg.eigvalsh(A)
    assert api.init(cfg) == ED_OK
    assert api.build(q1, q2) == (ED_OK, dim)
    x = start_vector(dim)
    # Nblock below Neigen+1 is raised to it, above 64 (and above dim) lowered: both still solve
    for neigen, nblock, nitermax in ((3, 1, 5000), (3, 4, 5000), (6, 23, 512), (6, 65, 512), (6, 1000, 512)):
        rc, ev, vec, nconv = api.eigh(neigen, nblock, nitermax, dim, x)
        assert rc == ED_OK, (neigen, nblock, api.last_error())
        print(f"neigen {neigen} nblock {nblock}: nconv {nconv}, max error {np.max(np.abs(ev - w[:neigen])):.2e}")
        assert nconv == neigen
        assert np.all(np.abs(ev - w[:neigen]) <= 1e-10 * np.maximum(1.0, np.abs(w[:neigen])))
        res = A @ vec.T - vec.T * ev
        assert np.max(np.linalg.norm(res, axis=0)) < 1e-8 * max(1.0, np.max(np.abs(w[:neigen])))
    # Neigen >= dim (>= the clamped ncv): refused by the host check, outputs untouched
    for neigen in (dim, dim + 5, 64):
        rc, ev, vec, nconv = api.eigh(neigen, 23, 512, dim, x)
        assert rc == ED_ERR_ARG and "nev" in api.last_error(), neigen
        assert np.all(ev == SENTINEL) and not vec.any() and nconv == -1
    # the dim-1 sector c2 (0,8): ncv is clamped to 1, no Neigen fits
    assert api.init(cases.c2()) == ED_OK
    assert api.build(0, 8) == (ED_OK, 1)
    for neigen, nblock in ((1, 23), (1, 1), (6, 23)):
        rc, ev, vec, nconv = api.eigh(neigen, nblock, 512, 1, np.ones(1, dtype=np.complex128))
        assert rc == ED_ERR_ARG, (neigen, nblock)
        assert np.all(ev == SENTINEL) and nconv == -1
    hv = np.zeros(1, dtype=np.complex128)                  # the sector itself is usable
    assert api.hxv(1, np.ones(1, dtype=np.complex128), hv) == ED_OK
