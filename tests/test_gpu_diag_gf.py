"""ed_diag sector loop and the normal-mode Green's function on the GPU against
the oracle-backed CPU pipeline (same algorithms, oracle pieces)."""
import numpy as np
import pytest

from edgpu.diag import DiagOptions, ed_diag, to_host
from edgpu.farm import farm_diag
from edgpu.params import make_config
from oracle_solver import solve_sector_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg_kw,method", [
    (dict(Norb=1, Nbath=4), "arpack"),                       # configs[0]: dense sectors
    (dict(Norb=1, Nbath=5), "lanczos"),
    (dict(Norb=1, Nbath=5), "arpack"),
    (dict(Norb=1, Nbath=3, Nspin=2, ed_mode="nonsu2"), "arpack"),
    (dict(Norb=2, Nbath=2, Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.25, bath="random", seed=3), "arpack"),
])
def test_ed_diag_matches_oracle(cfg_kw, method):
    cfg = make_config(**cfg_kw)
    opt = DiagOptions(lanc_method=method)
    ref = farm_diag(cfg, opt, solver=solve_sector_oracle).states
    res, sl = ed_diag(cfg, opt)
    assert sl.sectors == ref.sectors
    np.testing.assert_allclose(sl.energies, ref.energies, rtol=1e-10, atol=1e-10)
    for v, r in zip(sl.vectors, ref.vectors):       # same eigenvector up to a phase
        if v is not None and len(sl.vectors) == 1:
            assert abs(abs(np.vdot(to_host(v), r)) - 1.0) < 1e-8


def test_gf_normal_matches_oracle():
    from edgpu.gf import GFOptions, build_gf_normal
    from oracle_gf import build_gf_normal_oracle

    cfg = make_config(Norb=1, Nbath=5, bath="random", seed=5)
    _, sl = ed_diag(cfg, DiagOptions(lanc_method="lanczos"))
    gopt = GFOptions(Lmats=400, Lreal=400)
    rec = []
    Gm, Gr = build_gf_normal(cfg, sl, gopt, record=rec)
    Gm0, Gr0, rec0 = build_gf_normal_oracle(cfg, sl, gopt)
    assert len(rec) == len(rec0)
    for r, r0 in zip(rec, rec0):
        assert r["nlanc"] == r0["nlanc"]
        assert abs(r["norm2"] - r0["norm2"]) < 1e-13
        np.testing.assert_allclose(r["alfa"][:15], r0["alfa"][:15], rtol=1e-10, atol=1e-12)
    rel_m = np.max(np.abs(Gm - Gm0)) / np.max(np.abs(Gm0))
    rel_r = np.max(np.abs(Gr - Gr0)) / np.max(np.abs(Gr0))
    print(f"G(iw) rel diff {rel_m:.2e}, G(w) rel diff {rel_r:.2e}")
    assert rel_m < 1e-10          # north_star bar for G(iw)
    # real axis: eps=0.01 broadening amplifies pole-position differences ~1/eps^2;
    # 200 unreorthogonalised steps on a 300-dim sector make ghost poles whose
    # positions differ at rounding level between CPU and GPU summation orders
    assert rel_r < 1e-5
    # sum rule {c, c+} = 1: the two seed weights of each (state, site) add to 1
    w = {}
    for r in rec:
        key = (r["ispin"], r["iorb"], r["isector"])
        w[key] = w.get(key, 0.0) + r["norm2"]
    assert all(abs(v - 1.0) < 1e-12 for v in w.values())


@pytest.mark.parametrize("cfg_kw", [
    dict(Norb=1, Nbath=3, Nspin=2, ed_mode="nonsu2", bath="random", seed=2),   # configs[4] family
    dict(Norb=1, Nbath=4, Nspin=2, ed_mode="nonsu2"),
])
def test_gf_nonsu2_matches_oracle(cfg_kw):
    """build_gf_nonsu2: diagonal and spin-off-diagonal components (mixed seeds
    (c+_i + c+_j), (c+_i + i c+_j), recombination) vs the oracle pipeline."""
    from edgpu.gf import GFOptions, build_gf
    from oracle_gf import build_gf_oracle

    cfg = make_config(**cfg_kw)
    _, sl = ed_diag(cfg, DiagOptions(lanc_method="lanczos"))
    gopt = GFOptions(Lmats=300, Lreal=300)
    Gm, Gr = build_gf(cfg, sl, gopt)
    Gm0, Gr0 = build_gf_oracle(cfg, sl, gopt)
    scale = np.max(np.abs(Gm0))
    assert np.max(np.abs(Gm - Gm0)) / scale < 1e-10
    assert np.max(np.abs(Gr - Gr0)) / np.max(np.abs(Gr0)) < 1e-5
    # spin-off-diagonal components are present (ed_vsf_ratio != 0 mixes spins)
    assert np.max(np.abs(Gm0[0, 1, 0, 0])) > 1e-6 * scale


def test_gf_nonsu2_replica_matches_oracle():
    """build_gf_nonsu2 with a replica bath: the spin-off-diagonal components
    are computed where dmft_bath%mask is set (impHloc spin flip on the orbital,
    ED_GF_NONSU2.f90:203-217, ED_BATH/dmft_aux.f90:283-295)."""
    from cases import nonsu2_replica
    from edgpu.gf import GFOptions, build_gf, mixed_pairs
    from oracle_gf import build_gf_oracle

    cfg = nonsu2_replica()
    assert mixed_pairs(cfg)              # the case's impHloc has a spin flip
    _, sl = ed_diag(cfg, DiagOptions(lanc_method="lanczos"))
    gopt = GFOptions(Lmats=300, Lreal=300)
    Gm, Gr = build_gf(cfg, sl, gopt)
    Gm0, Gr0 = build_gf_oracle(cfg, sl, gopt)
    scale = np.max(np.abs(Gm0))
    assert np.max(np.abs(Gm - Gm0)) / scale < 1e-10
    assert np.max(np.abs(Gm0[0, 1, 0, 0])) > 1e-6 * scale


@pytest.mark.parametrize("cfg_kw", [
    dict(Norb=1, Nbath=4, Nspin=2, ed_mode="nonsu2", bath="random", seed=5),
    dict(Norb=2, Nbath=2, Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.25, bath="random", seed=3),
])
def test_gf_threaded_seeds_bit_identical(cfg_kw):
    """Seeds on 4 host threads (one sector cache each) give exactly the serial
    loop's G: per-job contributions are added in job order."""
    from edgpu.gf import GFOptions, build_gf

    cfg = make_config(**cfg_kw)
    _, sl = ed_diag(cfg, DiagOptions())
    G1 = build_gf(cfg, sl, GFOptions(Lmats=400, Lreal=400, workers=1))
    G4 = build_gf(cfg, sl, GFOptions(Lmats=400, Lreal=400, workers=4))
    for a, b in zip(G1, G4):
        assert np.any(a != 0)
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("cfg_kw", [
    dict(Norb=1, Nbath=6, Nspin=2, ed_mode="nonsu2", bath="random", seed=20251015),   # configs[4]
    dict(Norb=2, Nbath=2, Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.25, bath="random", seed=3),
])
def test_gf_batched_seeds_bit_identical(cfg_kw):
    """Seeds grouped by target sector and tridiagonalised in one batched
    persistent launch (ed_sector_lanc_tridiag_batch, one workgroup per seed)
    give exactly the per-seed loop's G; the batch entry point also matches a
    per-seed run on its own."""
    from edgpu.gf import GFOptions, build_gf

    cfg = make_config(**cfg_kw)
    _, sl = ed_diag(cfg, DiagOptions())
    Gs = build_gf(cfg, sl, GFOptions(Lmats=400, Lreal=400, workers=1, batch=False))
    Gb = build_gf(cfg, sl, GFOptions(Lmats=400, Lreal=400, batch=True))
    for a, b in zip(Gs, Gb):
        assert np.any(a != 0)
        np.testing.assert_array_equal(a, b)


def test_lanc_tridiag_batch_matches_single():
    import torch

    from edgpu.gf import _tridiag_batch, _tridiag_dev
    from edgpu.hamiltonian import Sector

    cfg = make_config(Norb=1, Nbath=6, Nspin=2, ed_mode="nonsu2", bath="random", seed=7)
    with Sector(cfg, 6, 0, stored=True, real=True) as S:
        g = torch.Generator(device="cuda:0").manual_seed(5)
        for cplx in (False, True):
            dt = torch.complex128 if cplx else torch.float64
            seeds = torch.rand(5, S.dim, dtype=dt, device="cuda:0", generator=g)
            seeds = seeds / torch.linalg.vector_norm(seeds, dim=1, keepdim=True)
            a, b, n = _tridiag_batch(S, seeds.contiguous(), 120, not cplx, 1e-13)
            for k in range(5):
                a1, b1, n1 = _tridiag_dev(S, seeds[k].contiguous(), 120, not cplx, 1e-13)
                assert n1 == n[k]
                np.testing.assert_array_equal(a1, a[k])
                np.testing.assert_array_equal(b1, b[k])


@pytest.mark.parametrize("options", [(), ("no_batch",), ("no_persist",)], ids=["default", "no_batch", "no_persist"])
def test_lanc_tridiag_entries_agree(options):
    """The three entries of the single-run tridiagonalisation give the same
    bits for every seed: the batch entry (one persistent launch under (), the
    per-seed loop under no_batch and no_persist), the device-vector entry and
    the host-vector entry (Sector.lanc_tridiag).  Within one set of options
    all three run the same recurrence on the same start vector, so alpha, beta
    and nlanc are compared with assert_array_equal; across options nothing is
    compared (the persistent and the multi-kernel recurrence sum in different
    orders).  lanc_geom says which recurrence ran: persistent unless
    no_persist, so the three cases cannot be one branch run three times.
    The sector of test_lanc_tridiag_batch_matches_single (nonsu2 Norb=1
    Nbath=6 (6, 0), 3,003 rows) runs the multi-kernel recurrence under every
    option, so this test takes the smallest sector of persist_shape_cases.py
    that is persistent by default: nb3_2_2, normal Norb=1 Nbath=3 (2, 2),
    stored, real, 36 rows (nitermax 40 is past its dimension: the runs end
    early, and nlanc is compared too)."""
    import torch

    from edgpu.gf import _tridiag_batch, _tridiag_dev
    from edgpu.hamiltonian import Sector

    cfg = make_config(Norb=1, Nbath=3)
    nseed, nitermax = 3, 40
    with Sector(cfg, 2, 2, stored=True, real=True, options=options) as S:
        assert S.dim == 36
        g = torch.Generator(device="cuda:0").manual_seed(5)
        for cplx in (False, True):
            mode = S.lanc_geom(real=not cplx)["mode"]
            if "no_persist" in options:
                assert mode == -1
            else:
                assert mode >= 0
            dt = torch.complex128 if cplx else torch.float64
            seeds = torch.rand(nseed, S.dim, dtype=dt, device="cuda:0", generator=g)
            seeds = (seeds / torch.linalg.vector_norm(seeds, dim=1, keepdim=True)).contiguous()
            host = seeds.cpu().numpy()
            a, b, n = _tridiag_batch(S, seeds, nitermax, not cplx, 1e-13)
            assert np.all(n > 0) and np.any(a != 0)
            for k in range(nseed):
                for a1, b1, n1 in (_tridiag_dev(S, seeds[k], nitermax, not cplx, 1e-13),
                                   S.lanc_tridiag(host[k], nitermax, 1e-13, real=not cplx)):
                    assert n1 == n[k]
                    np.testing.assert_array_equal(a1, a[k])
                    np.testing.assert_array_equal(b1, b[k])


def test_device_pole_sums_match_reference_loop():
    """ed_gf_add_poles (device G, one launch for many continued fractions)
    against the reference's loop written out in numpy (ED_GF_NORMAL.f90:620-631:
    for each pole j, G(i) = G(i) + (pesoBZ*Z(1,j))*Z(1,j)/(iw - isign*de)),
    fractions added in list order into their components: 1e-13 relative."""
    from edgpu.gf import PoleSums, matsubara, realaxis, tridiag_poles

    rng = np.random.default_rng(11)
    wm, wr = matsubara(1000.0, 300), realaxis(-5.0, 5.0, 200)
    P = PoleSums(2, 2, wm, wr, 0.01, 0)
    Gm = np.zeros((2, 2, 2, 2, len(wm)), dtype=np.complex128)
    Gr = np.zeros((2, 2, 2, 2, len(wr)), dtype=np.complex128)
    ref_m, ref_r = np.zeros_like(Gm), np.zeros_like(Gr)
    for f in range(7):
        n = int(rng.integers(1, 40))
        a = rng.normal(size=n)
        b = np.concatenate([[0.0], np.abs(rng.normal(size=n - 1))])
        E, z = tridiag_poles(a, b, n, first_row=True)
        comp = (int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)))
        pbz = complex(rng.uniform(0.1, 1.0), rng.uniform(-1, 1) if f % 2 else 0.0)
        ei, sg = float(rng.normal()), (1, -1)[f % 2]
        P.add(comp, pbz, ei, E, z, sg)
        s, t, o = comp
        for j in range(n):
            peso = (pbz * z[j]) * z[j]
            ref_m[s, t, o, o] += peso / (1j * wm - sg * (E[j] - ei))
            ref_r[s, t, o, o] += peso / ((wr + 1j * 0.01) - sg * (E[j] - ei))
    P.flush()
    P.to_host(Gm, Gr)
    for got, ref in ((Gm, ref_m), (Gr, ref_r)):
        assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(np.abs(ref))
