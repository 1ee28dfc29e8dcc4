"""The Fortran boundary on every ed_mode and bath: fortran/ed_gpu_replay packs
each model with ed_gpu_pack_params and drives it through the global API
(ed_gpu_build_sector, gpuMatVec_cc, ed_gpu_dump_csr, the row split with
gpuMatVec_mpi_cc / ed_gpu_hxv_mpi, ed_gpu_lanc_eigh, ed_gpu_lanc_tridiag,
ed_gpu_eigh); everything it writes is compared with the oracle and with numpy
on the oracle's matrix, never with another GPU result."""
import functools

import numpy as np
import pytest

import cases
from fortran_model import (boundary_cases, parse_lines, read_csr, read_hv, read_rows, read_tridiag, run_replay,
                           write_model)
from oracle.oracle import Oracle, lanc_tridiag, spmv, start_vector

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in boundary_cases()}
EIG_MIN, EIG_MAX = 23, 1300        # eigen section: Nblock=23 < dim <= 1300 (dense truth in milliseconds)
NO_EIGEN = {"replica_cplx_vr"}     # its stored H is complex-symmetric, not Hermitian (cases.replica_cplx_vr)


@functools.lru_cache(maxsize=None)
def _truth(name):
    """Per sector of the case, computed once and shared by stored and direct:
    hmap, CSR, H·x, and for the eigen-marked sectors the dense spectrum and
    the oracle's Lanczos coefficients.  Nothing here is modified afterwards."""
    _, factory, sectors = CASES[name]
    cfg = factory()
    orc = Oracle(cfg)
    out = {}
    for q1, q2 in sectors:
        hmap = orc.build_sector(q1, q2)
        csr = orc.build_csr(hmap)
        dim = len(hmap)
        x = start_vector(dim)
        t = dict(dim=dim, csr=csr, hv=spmv(csr, x), eigen=False)
        if EIG_MIN < dim <= EIG_MAX and name not in NO_EIGEN:
            rp, cols, vals = csr
            A = np.zeros((dim, dim), dtype=np.complex128)
            np.add.at(A, (np.repeat(np.arange(dim), np.diff(rp)), cols), vals)
            scale = float(np.max(np.abs(A)))
            if np.max(np.abs(A - A.conj().T)) <= 1e-14 * scale:
                t.update(eigen=True, w=np.linalg.eigvalsh(A), tri=lanc_tridiag(csr, x, 40),
                         cplx=bool(np.any(A.imag)), scale=scale)
        out[(q1, q2)] = t
    return cfg, out


def _rel(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def test_eigen_selection_covers_every_mode():
    """The dim / Hermiticity filter leaves eigen-marked sectors in every
    ed_mode and at least one with a complex H."""
    per_mode, cplx = {}, 0
    for name in CASES:
        cfg, truth = _truth(name)
        marked = [t for t in truth.values() if t["eigen"]]
        per_mode[cfg.ed_mode] = per_mode.get(cfg.ed_mode, 0) + len(marked)
        cplx += sum(t["cplx"] for t in marked)
        assert not (name in NO_EIGEN and marked)
    assert set(per_mode) == {"normal", "superc", "nonsu2"}
    assert all(n > 0 for n in per_mode.values()), per_mode
    assert cplx > 0
    assert any(t["eigen"] and q2 != 0 for (q1, q2), t in _truth("nonsu2_jz")[1].items())   # (n, twoJz) through q2


@pytest.mark.parametrize("form", ["stored", "direct"])
@pytest.mark.parametrize("name", list(CASES))
def test_replay(name, form, tmp_path):
    cfg, truth = _truth(name)
    model = tmp_path / "model.bin"
    write_model(cfg, model)
    args = []
    for (q1, q2), t in truth.items():
        args += [str(q1), f"{q2}e" if t["eigen"] else str(q2)]
    # one child for all of the case's sectors; a non-zero exit ends the test here
    r = run_replay("replay", model, form, tmp_path, *args, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REPLAY_OK" in r.stdout
    sec, rows = parse_lines(r.stdout, "SECTOR"), parse_lines(r.stdout, "ROWS")
    lanc, eigh, tri = parse_lines(r.stdout, "LANC"), parse_lines(r.stdout, "EIGH"), parse_lines(r.stdout, "TRI")
    assert set(sec) == set(truth)
    assert set(lanc) == set(eigh) == set(tri) == {k for k, t in truth.items() if t["eigen"]}
    mpi_cc = 0
    for (q1, q2), t in truth.items():
        dim, ref = t["dim"], t["hv"]
        assert int(sec[q1, q2]["DIM"]) == dim and int(sec[q1, q2]["VECDIM"]) == dim
        hv = read_hv(tmp_path, q1, q2)
        assert hv.shape == (dim,)
        if form == "stored":
            rp, cols, vals = read_csr(tmp_path, q1, q2)
            np.testing.assert_array_equal(rp, t["csr"][0])
            np.testing.assert_array_equal(cols, t["csr"][1])
            np.testing.assert_array_equal(vals, t["csr"][2])
            np.testing.assert_array_equal(hv, ref)
        else:
            print(f"{name} {form} ({q1},{q2}) dim {dim}: serial H.v rel {_rel(hv, ref):.2e}")
            assert _rel(hv, ref) < 1e-13          # the Kronecker kernel may be taken
        # row split: 1 rank (all rows: through gpuMatVec_mpi_cc), 3 ranks, dim+2 ranks
        ranks = sorted({1, 3} | ({dim + 2} if dim <= 300 else set()))
        assert sorted(k[2] for k in rows if k[:2] == (q1, q2)) == sorted(ranks)
        for P in ranks:
            ln = rows[q1, q2, P]
            got = read_rows(tmp_path, P, q1, q2)
            assert got.shape == (dim,)
            whole = sum(1 for rank in range(P) if (dim // P + (dim % P if rank == P - 1 else 0)) == dim)
            assert int(ln["MPI_CC"]) == whole
            assert int(ln["EMPTY"]) == (P - 1 if dim < P else 0)
            mpi_cc += whole
            if form == "direct" and whole:
                assert _rel(got, ref) < 1e-13     # a whole-sector build: as the serial product
            else:
                np.testing.assert_array_equal(got, ref)   # stored, or the generic matrix-free kernel
        if not t["eigen"]:
            continue
        w = t["w"]
        e0 = float(lanc[q1, q2]["E0"])
        print(f"{name} {form} ({q1},{q2}): E0-w0 {e0 - w[0]:.2e} nlanc {lanc[q1, q2]['NLANC']} "
              f"resid {lanc[q1, q2]['RESID']} eigres {eigh[q1, q2]['EIGRES']}")
        assert abs(e0 - w[0]) <= 1e-10 * max(1.0, abs(w[0]))
        assert float(lanc[q1, q2]["RESID"]) < 1e-5
        ev = np.array([float(eigh[q1, q2][f"EV{i}"]) for i in range(1, 7)])
        assert np.all(np.abs(ev - w[:6]) <= 1e-10 * np.maximum(1.0, np.abs(w[:6]))), (ev, w[:6])
        assert int(eigh[q1, q2]["NCONV"]) == 6
        # scale of the solver's own convergence test, |r_i| <= tol * |theta_i|
        assert float(eigh[q1, q2]["EIGRES"]) < 1e-8 * max(1.0, float(np.max(np.abs(w[:6]))))
        a, b = read_tridiag(tmp_path, q1, q2)
        a0, b0, _ = t["tri"]
        assert int(tri[q1, q2]["NTRI"]) >= 15
        assert b[0] == 0.0
        np.testing.assert_allclose(a[:15], a0[:15], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b[:15], b0[:15], rtol=1e-10, atol=1e-12)
    assert mpi_cc >= len(truth)       # gpuMatVec_mpi_cc ran in every sector


def test_replay_jz_breaking_model_stops_with_the_library_message(tmp_path):
    """A spin flip at fixed Lz (the model of test_gpu_jz.py) leaves the
    (n, twoJz) sector: build_Hv_sector fails with ED_ERR_UNSUPPORTED (5) and
    the shim stops with the library's message."""
    cfg = cases.nonsu2_jz()
    cfg.impHloc[0, 1, 0, 0] = cfg.impHloc[1, 0, 0, 0] = 0.1
    model = tmp_path / "model.bin"
    write_model(cfg, model)
    r = run_replay("replay", model, "stored", tmp_path, 6, 0, timeout=120)
    assert r.returncode != 0
    assert "ED_GPU ERROR in build_Hv_sector (rc=5)" in r.stdout and "Jz_basis" in r.stdout, r.stdout + r.stderr
    assert "REPLAY_OK" not in r.stdout
