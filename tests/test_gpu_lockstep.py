"""Block stored H·X (ed_sector_hxv_multi, k_spmv_mv) and the lockstep
multi-vector Lanczos (ed_sector_lanc_tridiag_lockstep) on the MI355X.

1. H·X column by column against ed_sector_hxv_dev on an ED_OPT_STORED_EXACT
   sector: bit-equal, every element written, two calls identical.
2. Lockstep alpha / beta against ed_sector_lanc_tridiag_batch on an
   ED_OPT_NO_PERSIST sector (the sequential multi-kernel runs): the first
   STEPS = 8 steps to 1e-12 (max|alpha| + 2 max|beta|), the pole sums of the
   full fractions to 1e-10 of max|G| on the Matsubara grid.  A CPU Lanczos
   whose two dot products are summed in a permuted block order holds 1.6e-16
   on the first 8 steps and 1.2e-13 on the pole sums at these shapes (c2 (4,4),
   hybrid (3,3), replica_cplx (3,3); 100 steps), so 8 steps stand.  The poles
   are measured from the sector's lowest energy, as add_to_lanczos_gf does
   (iw - (E_j - E_0)): interior Ritz values of a fixed-length run are not
   converged and only the fraction as a whole is comparable.
3. build_gf, build_gf_superc and build_chi with lockstep=True on sectors
   forced to ED_OPT_NO_PERSIST against the dense truths of orbmix_truth,
   superc_truth and chi_pair_truth, at those suites' bars.
4. Refusals leave NaN-filled outputs untouched.
"""
import ctypes

import numpy as np
import pytest

import cases
from edgpu import _lib, chi, gf
from edgpu.diag import DiagOptions, ed_diag
from edgpu.gf import GFOptions, _tridiag_batch, build_gf, build_gf_superc, matsubara, realaxis, tridiag_poles
from edgpu.hamiltonian import Sector
from edgpu.sectors import setup_pointers

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = 1, 5
STEPS = 8

# name -> (model of tests/cases.py, sector, packed words?, complex vectors?)
FORMS = {
    "real_packed": (cases.c2, (4, 4), True, False),              # dim 4900 = 76 slices + 36 rows, 20 blocks
    "real_plain_sell": (cases.hybrid, (3, 3), False, False),     # dim 400, plain SELL arrays (ED_NO_PACK), 2 blocks
    "complex_h_packed": (cases.replica_cplx, (3, 3), True, True),
    "complex_h_plain_sell": (cases.replica_cplx, (3, 3), False, True),
    "complex_vectors_real_h": (cases.c2, (4, 4), True, True),
    "complex_vectors_plain_sell": (cases.hybrid, (3, 3), False, True),
}


def _sector(form, *options):
    make, (q1, q2), pack, _ = FORMS[form]
    cfg = make()
    return Sector(cfg, q1, q2, stored=True, real=cfg.is_real(), pack=pack, options=options)


def _random(shape, cplx, seed):
    import torch

    rng = np.random.default_rng(seed)
    a = rng.normal(size=shape)
    if cplx:
        a = a + 1j * rng.normal(size=shape)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------ 1. block H·X
@pytest.mark.parametrize("form", list(FORMS))
def test_block_hxv_is_bit_equal_to_the_one_pass_kernel(form):
    import torch

    _, _, pack, cplx = FORMS[form]
    with _sector(form, "stored_exact") as S:
        assert bool(S.info.packed) == pack
        assert S.dim % 64 != 0                                   # the last slice is partial
        assert S.dim > 256                                       # more than one block
        longest = int(np.max(np.diff(S.dump_csr()[0]))) - 1      # off-diagonal elements of the longest row
        assert longest > 4                                       # beyond one chunk of the NV = 8 kernels (4 real, 2 complex)
        for nvec in (1, 2, 4, 8):
            X = _random((S.dim, nvec), cplx, 100 + nvec)
            ref = torch.empty_like(X)
            for v in range(nvec):
                col, out = X[:, v].contiguous(), torch.empty(S.dim, dtype=X.dtype, device=X.device)
                S.hxv_dev(col, out)
                ref[:, v] = out
            Y = torch.full_like(X, float("nan"))
            S.hxv_multi(X, Y)
            Y2 = torch.full_like(X, float("nan"))
            S.hxv_multi(X, Y2)
            torch.cuda.synchronize()
            y, y2, r = Y.cpu().numpy(), Y2.cpu().numpy(), ref.cpu().numpy()
            assert not np.any(np.isnan(y)), (form, nvec)      # every element written
            assert y.tobytes() == r.tobytes(), (form, nvec, np.max(np.abs(y - r)))
            assert y.tobytes() == y2.tobytes(), (form, nvec)


def test_block_hxv_and_lockstep_where_each_xcd_sweeps_its_own_rows():
    """Norb=1, Nbath=11, sector (6,6): 853,776 rows = 3,336 blocks, past the
    1,024 from which the packed kernel remaps its blocks per XCD and rounds the
    grid down to a multiple of 8 (3,336 is one; the partials are sized by it)."""
    import torch

    from edgpu.params import make_config

    cfg = make_config(Norb=1, Nbath=11, bath="random", seed=3)
    with Sector(cfg, 6, 6, stored=True, real=True, options=("stored_exact",)) as S:
        assert S.dim == 853776 and S.dim % 64 != 0 and S.info.packed and (S.dim + 255) // 256 >= 1024
        for cplx, nvec in ((False, 8), (True, 2)):
            X = _random((S.dim, nvec), cplx, nvec)
            Y = torch.full_like(X, float("nan"))
            S.hxv_multi(X, Y)
            for v in range(nvec):
                col, out = X[:, v].contiguous(), torch.empty(S.dim, dtype=X.dtype, device=X.device)
                S.hxv_dev(col, out)
                assert torch.equal(Y[:, v].contiguous().view(torch.float64), out.view(torch.float64)), (cplx, nvec, v)
        del X, Y
        seeds = _random((3, S.dim), False, 9)
        a0, b0, n0 = _tridiag_batch(S, seeds, STEPS, True, 1e-13)
        a1, b1, n1 = S.lanc_tridiag_lockstep(seeds, STEPS, 1e-13)
        scale = np.max(np.abs(a0)) + 2 * np.max(np.abs(b0))
        d = max(np.max(np.abs(a1 - a0)), np.max(np.abs(b1 - b0))) / scale
        print(f"(6,6) of Nbath=11, 3 seeds, {STEPS} steps: alpha/beta {d:.2e}")
        assert list(n1) == list(n0) == [STEPS] * 3 and d <= 1e-12


# ------------------------------------------- 2. lockstep against sequential
_E0 = {}


def _e0(form, S):
    """lowest energy of the form's sector, once"""
    if form not in _E0:
        _E0[form] = S.lanc_eigh(nitermax=300, threshold=1e-13, vector=False, real=not FORMS[form][3])[0]
    return _E0[form]


def _pole_sum(a, b, n, e0, wm):
    E, z2 = tridiag_poles(a, b, n)
    return np.sum(z2[None, :] / (1j * wm[:, None] - (E[None, :] - e0)), axis=1)


def _compare(form, S, cplx, e0, seeds, nlanc, threshold, want_n=None):
    """lockstep against the batch entry (sequential on this sector) on the same seeds; returns both results"""
    assert S.lanc_mode(real=not cplx) < 0                        # the batch entry runs the seeds one after the other
    a0, b0, n0 = _tridiag_batch(S, seeds, nlanc, not cplx, threshold)
    a1, b1, n1 = S.lanc_tridiag_lockstep(seeds, nlanc, threshold)
    assert np.array_equal(n0, n1), (n0, n1)
    if want_n is not None:
        assert list(n1) == list(want_n), (n1, want_n)
    wm = matsubara(100.0, 32)
    worst_ab = worst_g = 0.0
    for q in range(seeds.shape[0]):
        n = int(n1[q])
        if n == 0:
            assert not np.any(a1[q]) and not np.any(b1[q])
            continue
        k = min(STEPS, n)
        scale = np.max(np.abs(a0[q])) + 2 * np.max(np.abs(b0[q]))
        worst_ab = max(worst_ab, max(np.max(np.abs(a1[q, :k] - a0[q, :k])), np.max(np.abs(b1[q, :k] - b0[q, :k]))) / scale)
        g0, g1 = _pole_sum(a0[q], b0[q], n, e0, wm), _pole_sum(a1[q], b1[q], n, e0, wm)
        worst_g = max(worst_g, np.max(np.abs(g1 - g0)) / np.max(np.abs(g0)))
        assert b1[q, 0] == 0.0 and not np.any(a1[q, n:]) and not np.any(b1[q, n + 1:])     # unpack_tridiag's layout
    print(f"{form}: {seeds.shape[0]} seeds, nlanc {nlanc}: alpha/beta of the first {STEPS} steps {worst_ab:.2e}, "
          f"pole sums {worst_g:.2e}")
    assert worst_ab <= 1e-12
    assert worst_g <= 1e-10
    return (a0, b0, n0), (a1, b1, n1)


@pytest.mark.parametrize("form", ["real_packed", "complex_h_plain_sell", "complex_vectors_real_h"])
@pytest.mark.parametrize("nseed", [1, 3, 8, 13])
def test_lockstep_matches_the_sequential_runs(form, nseed):
    nlanc = 60
    with _sector(form, "no_persist") as S:
        cplx = FORMS[form][3]
        seeds = _random((nseed, S.dim), cplx, 7 * nseed)
        _compare(form, S, cplx, _e0(form, S), seeds, nlanc, 1e-13, want_n=[nlanc] * nseed)


def test_an_eigenvector_seed_stops_alone():
    """c2: the ground state of ed_diag as seed 2 of 5 (group 4 + 1) ends with
    nlanc = 1; its neighbours run on and give what they give without it."""
    import torch

    nlanc, thr = 40, 1e-10         # ed_diag's ground state: ||H v - E v|| = 1.6e-14 measured
    cfg = cases.c2()
    _, sl = ed_diag(cfg, DiagOptions())
    sec = setup_pointers(cfg)[sl.sectors[0] - 1]
    with Sector(cfg, sec.q1, sec.q2, stored=True, real=True, options=("no_persist",)) as S:
        v = sl.vectors[0]
        v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        gs = torch.from_numpy(np.ascontiguousarray(np.real(v), dtype=np.float64)).cuda()
        assert gs.numel() == S.dim
        seeds = _random((5, S.dim), False, 3)
        plain = S.lanc_tridiag_lockstep(seeds, nlanc, thr)
        seeds[2] = gs
        torch.cuda.synchronize()
        _, (a1, b1, n1) = _compare("c2 ground state", S, False, sl.energies[0], seeds, nlanc, thr,
                                   want_n=[nlanc, nlanc, 1, nlanc, nlanc])
        print(f"eigenvector seed: alpha - E0 = {a1[2, 0] - sl.energies[0]:.2e}, beta_2 = {b1[2, 1]:.2e}")
        assert abs(a1[2, 0] - sl.energies[0]) < 1e-9
        for q in (0, 1, 3, 4):                                   # same group or not: the same numbers as without it
            assert a1[q].tobytes() == plain[0][q].tobytes() and b1[q].tobytes() == plain[1][q].tobytes()


def test_a_zero_seed_gives_no_fraction():
    import torch

    form, nlanc = "complex_vectors_real_h", 30
    with _sector(form, "no_persist") as S:
        seeds = _random((3, S.dim), True, 11)
        plain = S.lanc_tridiag_lockstep(seeds, nlanc, 1e-13)
        seeds[1] = 0
        torch.cuda.synchronize()
        _, (a1, b1, n1) = _compare(form, S, True, _e0(form, S), seeds, nlanc, 1e-13, want_n=[nlanc, 0, nlanc])
        assert not np.any(a1[1]) and not np.any(b1[1])
        for q in (0, 2):
            assert a1[q].tobytes() == plain[0][q].tobytes() and b1[q].tobytes() == plain[1][q].tobytes()


# ------------------------------------------------------------ 3. end to end
@pytest.fixture
def lockstep_only(monkeypatch):
    """Every sector of a GF / chi build runs without the persistent kernels
    (so the lockstep entry is the one that serves), and the calls that reach
    the entry are counted."""
    calls = []
    get = gf._SectorCache.get

    def get_no_persist(self, sec, hamiltonian):
        new = (sec.q1, sec.q2, hamiltonian) not in self.d
        S = get(self, sec, hamiltonian)
        if new:
            S.set_options("no_persist")
        return S

    run = Sector.lanc_tridiag_lockstep

    def counted(self, seeds, nlanc, threshold=1e-13):
        calls.append(int(seeds.shape[0]))
        return run(self, seeds, nlanc, threshold)

    monkeypatch.setattr(gf._SectorCache, "get", get_no_persist)
    monkeypatch.setattr(Sector, "lanc_tridiag_lockstep", counted)
    return calls


@pytest.mark.parametrize("fused", [False, True])
def test_build_gf_hybrid_under_lockstep(lockstep_only, fused):
    import orbmix_truth as ot

    T = ot.truth("H2")
    cfg = T.cfg
    g = GFOptions(Lmats=32, Lreal=32, eps=ot.EPS["H2"], lockstep=True, fused_seeds=fused)
    _, sl = ed_diag(cfg, DiagOptions())
    Gm, Gr = build_gf(cfg, sl, g)
    Tm, Tr = T.gf(matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal), g.eps)
    dm = max(np.max(np.abs(Gm[s, s] - Tm[s])) for s in range(cfg.Nspin)) / np.max(np.abs(Tm))
    dr = max(np.max(np.abs(Gr[s, s] - Tr[s])) for s in range(cfg.Nspin)) / np.max(np.abs(Tr))
    print(f"H2 lockstep (fused_seeds={fused}): {len(lockstep_only)} calls of {sorted(set(lockstep_only))} seeds; "
          f"G(iw) {dm:.2e}, G(w) {dr:.2e}")
    assert len(lockstep_only) > 0 and max(lockstep_only) > 1
    assert dm < 1e-10 and dr < 1e-5


def test_build_gf_superc_under_lockstep(lockstep_only):
    import superc_truth as st

    T = st.truth("S2")
    g = GFOptions(Lmats=32, Lreal=32, eps=st.EPS["S2"], lockstep=True)
    _, sl = ed_diag(T.cfg, DiagOptions())
    wm, wr = matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal)
    got = build_gf_superc(T.cfg, sl, g)
    dm, dr, _ = st.distances(T.gf_of_list(sl, wm, wr, g.eps), got, wm, wr, g.eps)
    print(f"S2 lockstep: {len(lockstep_only)} calls of {sorted(set(lockstep_only))} seeds; (iw) {dm:.2e}, (w) {dr:.2e}")
    assert len(lockstep_only) > 0
    assert dm < 1e-10 and dr < 1e-5


def test_build_chi_pair_and_exc_under_lockstep(lockstep_only):
    import chi_pair_truth as pt

    T, copt = pt.truth("C2"), pt.options("C2", lockstep=True)
    _, sl = ed_diag(T.cfg, DiagOptions())
    got = chi.build_chi(T.cfg, sl, copt, pair=True, exc=True)
    d = pt.distances(T.pair_exc_of_list(sl, copt), got, T.cfg.Norb)
    print(f"C2 lockstep: {len(lockstep_only)} calls of {sorted(set(lockstep_only))} seeds; iv {d[0]:.2e}, tau {d[1]:.2e}, "
          f"w {d[2]:.2e}")
    assert len(lockstep_only) > 0
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5


def test_the_option_asks_the_sector(lockstep_only, monkeypatch):
    """With the persistent kernels available the small sector keeps today's
    batched launch: the choice is made by asking the sector, before any call."""
    with _sector("real_packed") as S:
        assert S.lanc_mode(real=True) >= 0
        seeds = _random((3, S.dim), False, 5)
        a0, b0, n0 = _tridiag_batch(S, seeds, 20, True, 1e-13)
        a1, b1, n1 = _tridiag_batch(S, seeds, 20, True, 1e-13, lockstep=True)
        assert lockstep_only == [] and a0.tobytes() == a1.tobytes() and b0.tobytes() == b1.tobytes()
        S.set_options("no_persist")
        _tridiag_batch(S, seeds, 20, True, 1e-13, lockstep=True)
        assert lockstep_only == [2]                             # 3 seeds: a group of 2, the tail through the batch entry
        # complex vectors: only up to the largest size at which they measured faster
        assert gf._lockstep_seeds(S, 5, False) == 4 and gf._lockstep_seeds(S, 1, False) == 0
        monkeypatch.setattr(gf, "LOCKSTEP_COMPLEX_MAX_DIM", S.dim - 1)
        assert gf._lockstep_seeds(S, 5, False) == 0 and gf._lockstep_seeds(S, 5, True) == 4
    cfg = cases.c2()
    with Sector(cfg, 4, 4, stored=False, direct=True, real=True, options=("no_persist",)) as D:
        assert not D.stored_whole
        _tridiag_batch(D, _random((2, D.dim), False, 6), 10, True, 1e-13, lockstep=True)
        assert lockstep_only == [2]                             # 3 seeds: a group of 2, the tail through the batch entry


# ------------------------------------------------------------- 4. refusals
def _refusals(S, code, cplx=False, **kw):
    import torch

    lib = _lib.load()
    dt = torch.complex128 if cplx else torch.float64
    nvec = kw.get("nvec", 4)
    cols = max(nvec, 1)
    X = torch.ones((S.dim, cols), dtype=dt, device="cuda")
    Y = torch.full((S.dim, cols), float("nan"), dtype=dt, device="cuda")
    st = torch.cuda.current_stream()
    y = X if kw.get("alias") else Y
    rc = lib.ed_sector_hxv_multi(S.handle, kw.get("vtype", 1 if cplx else 0), nvec, P(X.data_ptr()), P(y.data_ptr()),
                                 P(st.cuda_stream))
    torch.cuda.synchronize()
    assert rc == code, (kw, rc, lib.ed_gpu_last_error())
    assert np.all(np.isnan(Y.cpu().numpy())) and bool(torch.all(X == 1)), kw
    return lib.ed_gpu_last_error().decode()


def _lockstep_refusal(S, code, vtype=0):
    import torch

    lib = _lib.load()
    seeds = torch.ones((2, S.dim), dtype=torch.complex128 if vtype else torch.float64, device="cuda")
    a, b = np.full((2, 6), np.nan), np.full((2, 6), np.nan)
    n = np.full(2, -7, dtype=np.int32)
    torch.cuda.synchronize()
    rc = lib.ed_sector_lanc_tridiag_lockstep(S.handle, vtype, 2, P(seeds.data_ptr()), 6, 1e-13, P(a.ctypes.data),
                                             P(b.ctypes.data), P(n.ctypes.data))
    assert rc == code, (rc, lib.ed_gpu_last_error())
    assert np.all(np.isnan(a)) and np.all(np.isnan(b)) and np.all(n == -7)
    return lib.ed_gpu_last_error().decode()


def test_refusals_leave_the_outputs_untouched():
    cfg = cases.c2()
    with Sector(cfg, 4, 4, stored=True, real=True) as S:
        for nvec in (3, 0):
            assert "nvec" in _refusals(S, ERR_ARG, nvec=nvec)
        assert "overlaps" in _refusals(S, ERR_ARG, alias=True)
        assert "vtype" in _refusals(S, ERR_ARG, vtype=2)
    with Sector(cfg, 4, 4, stored=False, direct=True, real=True) as D:
        assert "no stored matrix" in _refusals(D, ERR_UNSUPPORTED)
        assert "no stored matrix" in _lockstep_refusal(D, ERR_UNSUPPORTED)
    with Sector(cfg, 4, 4, stored=True, real=True, rows=(1000, 1500)) as R:
        assert "row-split" in _refusals(R, ERR_UNSUPPORTED)
        assert "row-split" in _lockstep_refusal(R, ERR_UNSUPPORTED)
    ccfg = cases.replica_cplx()
    with Sector(ccfg, 3, 3, stored=True, real=False) as C:
        assert "complex H" in _refusals(C, ERR_ARG, vtype=0)
        assert "complex H" in _lockstep_refusal(C, ERR_ARG, vtype=0)
        assert "nvec" in _refusals(C, ERR_ARG, cplx=True, nvec=3)
