"""Spin and density susceptibilities on the MI355X: the diagonal-operator seed
kernel (ed_sector_seed_diag, k_seed_diag) against numpy seeds, the pole sum
(ed_chi_add_poles, k_chi_poles) against chi_host.chi_poles_host, and
edgpu.chi.build_chi against the dense Lehmann sums of chi_truth.

Bars.  Seeds: the unnormalised values exact — the device row is the numpy
row (the same additions and one product, in the same order) times the one
scale factor 1/sqrt(norm2) of its seed, where that factor may be the
correctly rounded one or a neighbour (the device's sqrt and divide are not
promised to round correctly); norm2 1e-13 relative (a sum of up to 273,273
squares in another order); the same bits from two calls.  Pole sum: 1e-13 of
the sum of |terms| per grid point (the device's exp against numpy's on the
tau grid; everything else is the same arithmetic).  build_chi: chi(iv) and
chi(tau) 1e-10 of each array's maximum, chi(w) 1e-5 at eps = 0.01, the
broadening fixed by the table in test_chi_cpu's docstring.

Measured on the MI355X.  Seeds: every non-zero one of the 902 seeds over all
shapes exact with the correctly rounded scale factor (no neighbour needed), norm2
within 4.4e-16, 273,273 rows: 2.2e-16 (real), 3.2e-16 (complex).  Pole sum:
iv 2.0e-17, tau 1.9e-16, w 2.3e-16 of the sum of |terms|.  build_chi against
the truth (iv / tau / w): C1 4.6e-15 / 4.7e-15 / 4.4e-15, C2 (3 states)
4.7e-15 / 5.5e-15 / 2.5e-14, CN 4.4e-15 / 4.7e-15 / 7.2e-08, thermal C1 (7
states, 2 twin entries) 1.7e-15 / 2.9e-15 / 2.0e-14.
"""
import ctypes

import numpy as np
import pytest

import chi_truth as ct
from chi_host import chi_poles_host, numpy_seeds
from edgpu import _lib, chi
from edgpu.diag import DiagOptions, ed_diag, post_diag
from edgpu.hamiltonian import Sector
from edgpu.params import make_config

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = 1, 5
_DIAG = {}


# ------------------------------------------------------------ the seed kernel
def _seed_diag(S, levels, weights, x, nlev=None, nseed=None, vtype=None, out=None):
    """(rc, seeds, norm2) of one ed_sector_seed_diag call; the output starts as NaN."""
    import torch

    lev = np.ascontiguousarray(levels, dtype=np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    ns = (w.size // max(len(lev), 1)) if nseed is None else nseed
    if out is None:
        out = torch.full((max(ns, 1), S.dim), float("nan"), dtype=x.dtype, device=x.device)      # written whole
    n2 = np.full(max(ns, 1), np.nan)
    stream = torch.cuda.current_stream()
    rc = _lib.load().ed_sector_seed_diag(S.handle, len(lev) if nlev is None else nlev, P(lev.ctypes.data), ns,
                                         P(w.ctypes.data), (1 if x.is_complex() else 0) if vtype is None else vtype,
                                         P(x.data_ptr()), P(out.data_ptr()), P(n2.ctypes.data), P(stream.cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), n2


def _random(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0.0)
    return v / np.linalg.norm(v)


def _tables(Ns, rng):
    """(levels, weights) for nlev = 1 and 6 with nseed = 1, 11 and 32; some weights zero, some negative."""
    six = [0, 2, 1, Ns + 1, Ns, 2 * Ns - 1]              # not in ascending order: the sum runs in table order
    out = []
    for lev in ([Ns], six):
        for nseed in (1, 11, 32):
            w = rng.normal(size=(nseed, len(lev)))
            w[rng.random(w.shape) < 0.25] = 0.0
            w[0] = 0.5 * (-1.0) ** np.arange(len(lev))
            out.append((lev, w))
    return out


def _check_seeds(hmap, levels, w, xh, seeds, n2):
    """Returns (norm2 distance, number of seeds scaled by a neighbour of 1/sqrt(norm2), zero seeds)."""
    ref = numpy_seeds(hmap, levels, w, xh)
    worst_n, off, zero = 0.0, 0, 0
    for q in range(len(w)):
        r2 = float(np.vdot(ref[q], ref[q]).real)
        if r2 == 0.0:
            assert n2[q] == 0.0 and not np.any(seeds[q])
            zero += 1
            continue
        worst_n = max(worst_n, abs(n2[q] - r2) / r2)
        inv = 1.0 / np.sqrt(n2[q])
        hit = [c for c in (inv, np.nextafter(inv, 0.0), np.nextafter(inv, 2.0 * inv)) if np.array_equal(seeds[q], c * ref[q])]
        assert hit, (q, np.max(np.abs(seeds[q] - inv * ref[q])))
        off += hit[0] != inv
    return worst_n, off, zero


SECTORS = {
    # name: (config, (q1, q2), dim, stored)
    "dim1": (lambda: make_config(Norb=2, Nbath=2, bath="random", seed=3), (0, 0), 1, False),
    "dim36": (lambda: make_config(Norb=2, Nbath=2, bath="random", seed=3), (1, 1), 36, False),        # below one wave
    "dim400": (lambda: make_config(Norb=2, Nbath=2, bath="random", seed=3), (3, 3), 400, False),      # 6.25 waves, 2 blocks
    "stored": (lambda: ct.config("C2"), (2, 2), 36, True),
    "nonsu2": (lambda: ct.config("CN"), (3, 0), 20, True),
    # more rows than the launcher's 1,024 blocks x 256 threads = 262,144: the strided loop runs twice.  Of
    # the Ns = 12 .. 16 normal sectors the smallest above that (Ns = 12: 392,040; 13: 368,082; 14: 273,273)
    "stride": (lambda: make_config(Norb=2, Nbath=6), (2, 6), 273273, False),
}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", list(SECTORS))
def test_seed_diag_matches_numpy_seeds(name, cplx):
    import torch

    mk, (q1, q2), dim, stored = SECTORS[name]
    cfg = mk()
    real = cfg.is_real()
    with Sector(cfg, q1, q2, stored=stored, direct=not stored, real=real) as S:
        assert S.dim == dim
        hmap = S.map()
        xh = _random(S.dim, cplx, 17)
        x = torch.from_numpy(xh).cuda()
        rng = np.random.default_rng(23)
        tables = _tables(cfg.Ns, rng)
        if name == "stride":
            tables = [tables[4]]                         # nlev = 6, nseed = 11
        worst, off, zero, nseeds = 0.0, 0, 0, 0
        for lev, w in tables:
            rc, seeds, n2 = _seed_diag(S, lev, w, x)
            assert rc == 0, _lib.load().ed_gpu_last_error()
            rc2, seeds2, n22 = _seed_diag(S, lev, w, x)
            assert rc2 == 0 and seeds.tobytes() == seeds2.tobytes() and n2.tobytes() == n22.tobytes()
            assert seeds.dtype == (np.complex128 if cplx else np.float64)
            a, b, c = _check_seeds(hmap, lev, w, xh, seeds, n2)
            worst, off, zero, nseeds = max(worst, a), off + b, zero + c, nseeds + len(w)
    print(f"{name} dim {dim} cplx={cplx}: {nseeds} seeds exact ({off} with a neighbouring scale factor, {zero} zero), "
          f"norm2 {worst:.2e}")
    assert worst <= 1e-13


def test_seed_diag_sz_of_the_empty_sector_is_zero():
    """dim 1, the (0,0) sector: Sz and n give norm2 = 0 and an all-zero seed."""
    import torch

    cfg = ct.config("C2")
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S:
        assert S.dim == 1
        lev, w = chi.seed_levels(cfg), np.array([t[2] for t in chi.seed_table(cfg)])
        rc, seeds, n2 = _seed_diag(S, lev, w, torch.ones(1, dtype=torch.float64, device="cuda"))
        assert rc == 0 and not np.any(n2) and not np.any(seeds) and seeds.shape == (7, 1)
    with Sector(cfg, 4, 4, stored=False, direct=True, real=True) as S:      # the full sector: n_a = 2, Sz = 0
        rc, seeds, n2 = _seed_diag(S, lev, w, torch.ones(1, dtype=torch.float64, device="cuda"))
        assert rc == 0 and list(n2) == [0.0, 0.0, 0.0, 4.0, 4.0, 16.0, 16.0]
        assert list(seeds[:, 0]) == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]


def test_sector_method_and_out_argument():
    import torch

    cfg = ct.config("C2")
    lev, w = chi.seed_levels(cfg), np.array([t[2] for t in chi.seed_table(cfg)])
    with Sector(cfg, 2, 2, stored=True, real=True) as S:
        xh = _random(S.dim, False, 4)
        seeds, n2 = S.seed_diag(xh, lev, w)
        assert seeds.shape == (7, 36) and seeds.is_cuda and n2.shape == (7,)
        out = torch.empty((7, 36), dtype=torch.float64, device="cuda")
        seeds2, n22 = S.seed_diag(torch.from_numpy(xh).cuda(), lev, w, out=out)
        assert seeds2 is out and torch.equal(seeds, out) and np.array_equal(n2, n22)
        a, _, _ = _check_seeds(S.map(), lev, w, xh, seeds.cpu().numpy(), n2)
        assert a < 1e-13
        with pytest.raises(ValueError):
            S.seed_diag(xh, lev, w, out=torch.empty((6, 36), dtype=torch.float64, device="cuda"))


def test_seed_diag_refusals_leave_the_output_untouched():
    import torch

    cfg = ct.config("C2")
    Ns = cfg.Ns
    with Sector(cfg, 2, 2, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 2, 2, stored=True, real=True, rows=(0, 20)) as Srow:
        xh = _random(S.dim, False, 1)
        x = torch.from_numpy(xh).cuda()
        ok = dict(levels=[0, Ns], weights=[[0.5, -0.5], [1.0, 1.0]])

        def refused(code=ERR_ARG, sec=S, **kw):
            a = dict(ok, **kw)
            extra = {k: a.pop(k) for k in ("nlev", "nseed", "vtype") if k in a}
            rc, seeds, n2 = _seed_diag(sec, a["levels"], a["weights"], x, **extra)
            assert rc == code, (kw, rc)
            assert np.all(np.isnan(seeds)) and np.all(np.isnan(n2)), kw      # nothing was launched

        rc, seeds, n2 = _seed_diag(S, ok["levels"], ok["weights"], x)
        assert rc == 0 and not np.any(np.isnan(seeds)) and not np.any(np.isnan(n2))
        refused(levels=[], weights=[], nlev=0, nseed=1)                      # nlev = 0
        refused(levels=list(range(7)), weights=[[1.0] * 7])                  # nlev = 7
        refused(levels=[0, 0])                                               # duplicate level
        refused(levels=[0, 2 * Ns])                                          # level = 2*Ns
        refused(levels=[-1, Ns])                                             # level < 0
        refused(nseed=0)                                                     # nseed = 0
        refused(weights=[[1.0, 1.0]] * 33)                                   # nseed = 33
        refused(vtype=2)                                                     # vtype outside {0, 1}
        refused(vtype=-1)
        refused(code=ERR_UNSUPPORTED, sec=Srow)                              # whole sectors only
        # seeds overlapping src_vec: the vector is the first row of the output buffer
        dim = S.dim
        buf = torch.full((3 * dim,), float("nan"), dtype=torch.float64, device="cuda")
        buf[:dim] = x
        rc, after, n2 = _seed_diag(S, ok["levels"], ok["weights"], buf[:dim], out=buf)
        assert rc == ERR_ARG and np.array_equal(after[:dim], xh) and np.all(np.isnan(after[dim:])) and np.all(np.isnan(n2))
        # ... and its last element the first of the output
        rc, after, n2 = _seed_diag(S, ok["levels"], ok["weights"], buf[:dim], out=buf[dim - 1:])
        assert rc == ERR_ARG and np.all(np.isnan(after[1:]))
        # the output right behind the vector is accepted
        rc, after, n2 = _seed_diag(S, ok["levels"], ok["weights"], buf[:dim], out=buf[dim:])
        assert rc == 0 and not np.any(np.isnan(after)) and not np.any(np.isnan(n2))
        # nlev = 6 and nseed = 32 are accepted
        rc, _, _ = _seed_diag(S, [0, 1, 2, 3, Ns, Ns + 1], np.ones((32, 6)), x)
        assert rc == 0


# ------------------------------------------------------------ the pole sum
def _fractions(rng, beta):
    """Fractions that switch component back and forth, a one-pole fraction, a
    pole with D == 0 exactly and poles with D < 0."""
    out = []
    for comp, npole in ((0, 5), (2, 7), (0, 1), (1, 4), (2, 3), (2, 6), (0, 9)):
        ei = float(rng.normal())
        D = np.sort(rng.uniform(0.05, 3.0, size=npole))
        if npole >= 2:
            D[0] = -rng.uniform(0.1, 0.7)               # a downward transition
        if npole >= 4:
            D[1] = 0.0                                  # D == 0 exactly
        E = ei + D
        z = rng.normal(size=npole)
        z /= np.linalg.norm(z)
        out.append((comp, float(rng.uniform(0.1, 2.0)), ei, E, z))
    assert any(np.any(E == ei) for _, _, ei, E, _ in out)
    return out


def test_chi_add_poles_matches_the_host_restatement():
    beta, eps, ncomp = 8.0, 0.05, 3
    Lmats, Ltau, Lreal = 37, 11, 65                     # 38 + 12 + 65 grid points: both inner boundaries fall inside waves
    vm, tg, wr = chi.bosonic_matsubara(beta, Lmats), chi.tau_grid(beta, Ltau), np.linspace(-4.0, 4.0, Lreal)
    assert (len(vm) % 64, (len(vm) + len(tg)) % 64) == (38, 50)
    rng = np.random.default_rng(41)
    first, second = _fractions(rng, beta), _fractions(rng, beta)
    ps = chi.ChiPoleSums(ncomp, vm, tg, wr, beta, eps, 0)
    for fr in first:
        ps.add(*fr)
    ps.flush()
    got1 = ps.to_host()
    ref1 = chi_poles_host(first, beta, vm, tg, wr, eps, ncomp)
    for fr in second:                                   # a second flush accumulates onto the first
        ps.add(*fr)
    ps.flush()
    got2 = ps.to_host()
    ref2 = chi_poles_host(second, beta, vm, tg, wr, eps, ncomp, start=ref1[:3])
    mag2 = [m1 + (m2 - np.abs(s)) for m1, m2, s in zip(ref1[3], ref2[3], ref1[:3])]      # sum |terms| of both flushes
    worst = []
    for got, ref, mag in ((got1, ref1[:3], ref1[3]), (got2, ref2[:3], mag2)):
        for g, r, m in zip(got, ref, mag):
            assert g.shape == r.shape and np.all(m > 0)
            worst.append(np.max(np.abs(g - r) / m))
    print("first flush iv %.2e tau %.2e w %.2e; second %.2e %.2e %.2e (of sum |terms| per grid point)" % tuple(worst))
    assert got1[1].dtype == np.float64 and got1[0].dtype == np.complex128
    assert np.max(np.abs(got2[0] - got1[0])) > 0
    assert max(worst) <= 1e-13
    ps.flush()                                          # nothing queued: nothing changes
    assert all(np.array_equal(a, b) for a, b in zip(ps.to_host(), got2))


# ------------------------------------------------------------ build_chi
def states(name):
    if name not in _DIAG:
        _DIAG[name] = ed_diag(ct.truth(name).cfg, DiagOptions())[1]
    return _DIAG[name]


@pytest.mark.parametrize("name", ["C1", "C2", "CN"])
def test_build_chi_matches_the_dense_truth(name):
    T, copt, sl = ct.truth(name), ct.options(name), states(name)
    cfg = T.cfg
    rec = []
    got = chi.build_chi(cfg, sl, copt, record=rec)
    d = ct.distances(T.chi_of_list(sl, copt), got, cfg.Norb)
    print(f"{name}: {sl.size} state(s) in sectors {sl.sectors}, eps {copt.eps}: iv {d[0]:.2e}, tau {d[1]:.2e}, w {d[2]:.2e}")
    assert [(r["state"], r["name"]) for r in rec] == [(k, n) for k, _, n, _ in chi.chi_jobs(cfg, sl)]
    No = cfg.Norb
    assert got.spin_iv.shape == (No + 1, ct.LMATS + 1) and got.spin_tau.shape == (No + 1, ct.LTAU + 1)
    assert got.dens_w.shape == (No, No, ct.LREAL) and got.dens_tot_tau.shape == (ct.LTAU + 1,)
    if No == 1:
        assert not np.any(got.spin_iv[1]) and not np.any(got.dens_tot_w)
    else:
        assert np.array_equal(got.dens_iv[0, 1], got.dens_iv[1, 0])
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5
    s_only, d_only = chi.build_chi(cfg, sl, copt, dens=False), chi.build_chi(cfg, sl, copt, spin=False)
    assert s_only.dens_iv is None and s_only.dens_tot_w is None and d_only.spin_tau is None
    for a, b in ((s_only.spin_iv, got.spin_iv), (s_only.spin_tau, got.spin_tau), (s_only.spin_w, got.spin_w),
                 (d_only.dens_iv, got.dens_iv), (d_only.dens_tau, got.dens_tau), (d_only.dens_w, got.dens_w),
                 (d_only.dens_tot_iv, got.dens_tot_iv), (d_only.dens_tot_tau, got.dens_tot_tau)):
        assert np.array_equal(a, b)


def test_build_chi_thermal_list_with_twin_vectors():
    T, copt = ct.truth("C1"), ct.options("C1")
    opt = DiagOptions(lanc_nstates_total=ct.NTOTAL, beta=ct.BETA, cutoff=ct.CUTOFF, ed_twin=True)
    _, sl = ed_diag(T.cfg, opt)
    sl2, _ = post_diag(sl, opt, T.cfg)
    kept = T.thermal_states()
    assert sl2.size == len(kept) and sum(p is not None for p in sl2.twin_of) >= 1
    assert np.max(np.abs(np.sort(sl2.energies) - np.array([t[0] for t in kept]))) < 1e-10
    got = chi.build_chi(T.cfg, sl2, copt)
    d = ct.distances(T.chi_thermal(copt), got, 1)
    print(f"thermal C1: {sl2.size} states, {sum(p is not None for p in sl2.twin_of)} twin entries: iv {d[0]:.2e}, "
          f"tau {d[1]:.2e}, w {d[2]:.2e}")
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5
    with pytest.raises(ValueError, match="beta"):
        chi.build_chi(T.cfg, sl2, chi.ChiOptions(Lmats=4, Ltau=4, Lreal=4))      # ChiOptions.beta = 1000


def test_build_chi_refuses_superc_and_a_rank_split(monkeypatch):
    import superc_truth as st

    scfg = st.config("S1")
    with pytest.raises(NotImplementedError, match="superc"):
        chi.build_chi(scfg, states("C1"), ct.options("C1"))

    class World:
        @staticmethod
        def get_world_size():
            return 2

    monkeypatch.setattr(chi, "_dist", lambda: World)
    with pytest.raises(NotImplementedError, match="rank split"):
        chi.build_chi(ct.truth("C1").cfg, states("C1"), ct.options("C1"))
