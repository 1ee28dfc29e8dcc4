"""Orbital off-diagonal Green's function (lanc_build_gf_normal_mix_c,
ED_GF_NORMAL.f90:279-553) and the fused seed kernel (ed_sector_seed_batch) on
the MI355X: against the dense direct Lehmann sum of orbmix_truth and the
oracle pipeline of oracle_gf_orbmix.

Bars: G(iw) 1e-10 of max|G|; G(w) 1e-8 at the per-model broadening
orbmix_truth.EPS (test_orbmix_cpu's docstring has the sensitivity table that
fixes it); fused against unfused seeds 1e-12 on G(iw), where only the
summation order of norm2 differs.

Measured on the MI355X.  Against the dense truth, G(iw) / G(w): H2 2.3e-14 /
1.8e-14, H3 3.9e-15 / 9.3e-10, RC 1.9e-14 / 5.6e-13; against the oracle
pipeline: H2 1.6e-14 / 4.4e-14, H3 2.4e-14 / 3.6e-10, RC 4.0e-14 / 1.8e-12;
thermal H2 (27 states, twin vectors) G_01(iw) 8.4e-15.  ed_sector_seed_batch
against the numpy seeds: normalised seeds <= 4.2e-17, norm2 <= 4.0e-16, the
unnormalised seed within 2.0 ulp of the apply_op chain (scale and back).
Fused against unfused: H3 G(iw) 1.4e-15, G(w) 4.9e-10; nonSU2 2.8e-13, 6.9e-14.
"""
import ctypes

import numpy as np
import pytest

import cases
import orbmix_truth as ot
from edgpu import _lib
from edgpu.diag import DiagOptions, ed_diag, post_diag
from edgpu.gf import GFOptions, build_gf, matsubara, orbital_pairs, realaxis
from edgpu.hamiltonian import Sector
from edgpu.params import make_config
from edgpu.sectors import get_sector

pytestmark = pytest.mark.gpu

MODELS = ["H2", "H3", "RC"]
_DIAG, _GF = {}, {}
P = ctypes.c_void_p


def gopt(name, **kw):
    return GFOptions(Lmats=32, Lreal=32, eps=ot.EPS[name], **kw)


def states(name):
    if name not in _DIAG:
        _DIAG[name] = ed_diag(ot.truth(name).cfg, DiagOptions())[1]
    return _DIAG[name]


def gf(name):
    """ed_diag + build_gf with the default host path, once per model."""
    if name not in _GF:
        _GF[name] = build_gf(ot.truth(name).cfg, states(name), gopt(name))
    return _GF[name]


def _offdiag_dist(cfg, G, G0):
    """max over the pairs of |G[s,s,a,b] - G0[s,a,b]| / max|G| (G0 indexed [s,a,b] or [s,s,a,b])."""
    scale = np.max(np.abs(G))
    return max(np.max(np.abs(G[s, s, a, b] - (G0[s, a, b] if G0.ndim == 4 else G0[s, s, a, b])))
               for s, a, b in orbital_pairs(cfg)) / scale


@pytest.mark.parametrize("name", MODELS)
def test_offdiagonal_g_matches_dense_truth_and_oracle(name):
    from oracle_gf_orbmix import build_gf_orbmix_oracle

    T, sl = ot.truth(name), states(name)
    cfg, g = T.cfg, gopt(name)
    if name == "H2":
        assert sl.size == 2
    Gm, Gr = gf(name)
    Tm, Tr = T.gf(matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal), g.eps)
    Om, Or = build_gf_orbmix_oracle(cfg, sl, g)
    dm, dr = _offdiag_dist(cfg, Gm, Tm), _offdiag_dist(cfg, Gr, Tr)
    om, orr = _offdiag_dist(cfg, Gm, Om), _offdiag_dist(cfg, Gr, Or)
    big = max(np.max(np.abs(Gm[s, s, a, b])) for s, a, b in orbital_pairs(cfg)) / np.max(np.abs(Gm))
    print(f"{name}: vs truth G(iw) {dm:.2e} G(w) {dr:.2e}; vs oracle G(iw) {om:.2e} G(w) {orr:.2e}; "
          f"max|G_ab|/max|G| {big:.2f}")
    assert dm < 1e-10 and dr < 1e-8
    assert om < 1e-10 and orr < 1e-8
    assert big > 0.1
    for s, a, b in orbital_pairs(cfg):
        assert np.array_equal(Gm[s, s, b, a], Gm[s, s, a, b]) and np.array_equal(Gr[s, s, b, a], Gr[s, s, a, b])


def test_host_paths_bit_identical():
    cfg, sl = ot.truth("H3").cfg, states("H3")
    Gb = gf("H3")                                            # batch=True
    G1 = build_gf(cfg, sl, gopt("H3", batch=False, workers=1))
    G4 = build_gf(cfg, sl, gopt("H3", batch=False, workers=4))
    for a, b, c in zip(Gb, G1, G4):
        assert np.any(a[0, 0, 0, 1] != 0)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def test_orbital_mix_off_is_the_diagonal_alone():
    cfg, sl = ot.truth("H3").cfg, states("H3")
    for G, G1 in zip(build_gf(cfg, sl, gopt("H3", orbital_mix=False)), gf("H3")):
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                if a == b:
                    assert np.any(G[:, :, a, a] != 0) and np.array_equal(G[:, :, a, a], G1[:, :, a, a])
                else:
                    assert not np.any(G[:, :, a, b])


def test_finite_temperature_with_twin_vectors():
    """Thermal state list of H2 with ed_twin: twin entries' vectors (rebuilt on
    the device) feed the mixed seeds; G_01(iw) against the Boltzmann-weighted
    direct Lehmann sum over the dense thermal set."""
    T = ot.truth("H2")
    opt = DiagOptions(lanc_nstates_total=40, beta=ot.BETA, cutoff=ot.CUTOFF, ed_twin=True)
    _, sl = ed_diag(T.cfg, opt)
    sl2, _ = post_diag(sl, opt, T.cfg)
    kept = T.thermal_states()
    assert sl2.size == len(kept) and sum(p is not None for p in sl2.twin_of) > 0
    assert np.max(np.abs(np.sort(sl2.energies) - np.array([t[0] for t in kept]))) < 1e-10
    g = gopt("H2", beta=ot.BETA)
    Gm, _ = build_gf(T.cfg, sl2, g)
    Tm, _ = T.gf(matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal), g.eps, beta=ot.BETA)
    d = np.max(np.abs(Gm[0, 0, 0, 1] - Tm[0, 0, 1])) / np.max(np.abs(Gm))
    print(f"thermal H2, {sl2.size} states: |G_01(iw) - truth| / max|G| = {d:.2e}")
    assert d < 1e-10


# ------------------------------------------------------------ the kernel alone
def _seed_batch(src, dst, op, levels, coef, x, nseed=None, nlev=None, out=None):
    """(rc, seeds, norm2) of one ed_sector_seed_batch call; coef: (nseed, nlev) complex.  out: the device
    tensor to write into (default: a NaN-filled one, written whole)."""
    import torch

    coef = np.ascontiguousarray(coef, dtype=np.complex128)
    nseed = coef.shape[0] if nseed is None else nseed
    lev = np.ascontiguousarray(levels, dtype=np.int32)
    if out is None:
        out = torch.full((max(nseed, 1), dst.dim), float("nan"), dtype=x.dtype, device=x.device)
    n2 = np.full(max(nseed, 1), np.nan)
    st = torch.cuda.current_stream()
    rc = _lib.load().ed_sector_seed_batch(src.handle, dst.handle, op, len(lev) if nlev is None else nlev,
                                          P(lev.ctypes.data), nseed, P(coef.ctypes.data),
                                          1 if x.is_complex() else 0, P(x.data_ptr()), P(out.data_ptr()),
                                          P(n2.ctypes.data), P(st.cuda_stream))
    return rc, out.cpu().numpy(), n2


def _chain(src, dst, op, terms, x):
    """ed_sector_apply_op + ed_sector_apply_op_acc: the unfused seed, unnormalised."""
    import torch

    L, st = _lib.load(), torch.cuda.current_stream()
    vt = 1 if x.is_complex() else 0
    y = torch.empty(dst.dim, dtype=x.dtype, device=x.device)
    _lib.check(L.ed_sector_apply_op(src.handle, dst.handle, op, terms[0][0], vt, P(x.data_ptr()), P(y.data_ptr()),
                                    P(st.cuda_stream)), "apply_op")
    for lv, c in terms[1:]:
        c = complex(c)
        _lib.check(L.ed_sector_apply_op_acc(src.handle, dst.handle, op, lv, c.real, c.imag, vt, P(x.data_ptr()),
                                            P(y.data_ptr()), P(st.cuda_stream)), "apply_op_acc")
    return y.cpu().numpy()


def _random(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0.0)
    return v / np.linalg.norm(v)


def _check_against_numpy(cfg, orc, srcq, dstq, op, levels, coef, x_host, S, D):
    import torch

    from oracle_gf import seed_combo

    x = torch.from_numpy(x_host).cuda()
    rc, seeds, n2 = _seed_batch(S, D, op, levels, coef, x)
    assert rc == 0, _lib.load().ed_gpu_last_error()
    rc2, seeds2, n22 = _seed_batch(S, D, op, levels, coef, x)
    assert rc2 == 0 and seeds.tobytes() == seeds2.tobytes() and n2.tobytes() == n22.tobytes()
    hmap_i = orc.build_sector(*srcq)
    assert np.array_equal(hmap_i, S.map())
    jsec = get_sector(cfg)[dstq]
    worst_v = worst_n = worst_ulp = 0.0
    for q in range(len(coef)):
        terms = [(lv, coef[q][l]) for l, lv in enumerate(levels) if coef[q][l] != 0]
        _, ref = seed_combo(orc, hmap_i, jsec, op, terms, x_host.astype(np.complex128))
        r2 = float(np.vdot(ref, ref).real)
        assert r2 > 0
        worst_n = max(worst_n, abs(n2[q] - r2) / r2)
        worst_v = max(worst_v, np.max(np.abs(seeds[q] - ref / np.sqrt(r2))))
        if len(terms) <= 2 and terms[0][1] == 1:
            ch = _chain(S, D, op, terms, x)
            un = seeds[q] * np.sqrt(n2[q])
            for a, b in ((un.real, ch.real), (un.imag, ch.imag)):
                nz = b != 0
                assert np.all(a[~nz] == 0)
                if np.any(nz):
                    worst_ulp = max(worst_ulp, np.max(np.abs(a[nz] - b[nz]) / np.spacing(np.abs(b[nz]))))
    print(f"{srcq}->{dstq} op={op} nseed={len(coef)} nlev={len(levels)} cplx={np.iscomplexobj(x_host)}: "
          f"seed {worst_v:.2e}, norm2 {worst_n:.2e}, chain {worst_ulp:.1f} ulp")
    assert worst_v <= 1e-14 and worst_n <= 1e-13 and worst_ulp <= 2.0


def _coefs9(cplx):
    """Norb^2 = 9 seeds on 3 levels: the singles, the (1, 1) pairs and the (1, i) or (1, -1) pairs."""
    second = 1j if cplx else -1.0
    rows = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for c in (1.0, second):
            r = [0, 0, 0]
            r[a], r[b] = 1, c
            rows.append(r)
    return np.array(rows, dtype=np.complex128)


@pytest.mark.parametrize("cplx", [False, True])
def test_seed_batch_matches_numpy_seeds(cplx):
    from oracle.oracle import Oracle

    cfg = make_config(Norb=2, Nbath=5, Nspin=1, bath_type="hybrid", bath="random", seed=3)
    Ns = cfg.Ns
    assert Ns == 7
    orc = Oracle(cfg)
    rng = np.random.default_rng(4)
    c32 = rng.normal(size=(32, 2)) + (1j * rng.normal(size=(32, 2)) if cplx else 0.0)
    c32[0] = (1, 1)
    if cplx:
        c32[1], c32[2] = (1, 1j), (1, -1j)
    shapes = [
        ((3, 3), (4, 3), 1, [0, 1, 2], _coefs9(cplx)),                 # 1225 rows: 5 blocks, ragged tail
        ((3, 3), (2, 3), 0, [0, 1], np.array([[1, 1]])),               # 735 rows, nseed = 1
        ((3, 3), (3, 4), 1, [Ns, Ns + 1], c32),                        # spin down: the sign carries nup
        ((3, 3), (3, 2), 0, [Ns, Ns + 2], np.array([[1, 1], [1, -1j if cplx else -1], [0, 1], [1, 0]])),
        ((6, 0), (7, 0), 1, [0, 1, 2], np.array([[1, 1, 0], [0, 1, 1]])),   # dim 7 into dim 1
    ]
    secs = {}
    try:
        for srcq, dstq, op, levels, coef in shapes:
            for q in (srcq, dstq):
                if q not in secs:
                    secs[q] = Sector(cfg, q[0], q[1], stored=False, direct=True, real=True)
            x = _random(secs[srcq].dim, cplx, 17)
            _check_against_numpy(cfg, orc, srcq, dstq, op, levels, np.asarray(coef, dtype=np.complex128), x,
                                 secs[srcq], secs[dstq])
    finally:
        for S in secs.values():
            S.close()


def test_seed_batch_zero_norm_seed_and_nonsu2():
    import torch

    from oracle.oracle import Oracle

    cfg = make_config(Norb=2, Nbath=5, Nspin=1, bath_type="hybrid", bath="random", seed=3)
    with Sector(cfg, 3, 3, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 4, 3, stored=False, direct=True, real=True) as D:
        hmap = S.map()
        m = 600
        occ = [lv for lv in range(cfg.Ns) if (hmap[m] >> lv) & 1]
        free = [lv for lv in range(cfg.Ns) if not (hmap[m] >> lv) & 1]
        e = np.zeros(S.dim)
        e[m] = 1.0
        # c+ on an occupied level of the only populated state: nothing; on a free one: one element
        rc, seeds, n2 = _seed_batch(S, D, 1, [occ[0], free[0]], np.array([[1, 0], [0, 1]]), torch.from_numpy(e).cuda())
        assert rc == 0
        assert n2[0] == 0.0 and not np.any(seeds[0])
        assert n2[1] == 1.0 and np.count_nonzero(seeds[1]) == 1 and np.max(np.abs(seeds[1])) == 1.0

    cfg = cases.nonsu2_rand()
    Ns = cfg.Ns
    orc = Oracle(cfg)
    with Sector(cfg, 6, 0, stored=False, direct=True, real=False) as S, \
            Sector(cfg, 7, 0, stored=False, direct=True, real=False) as D:
        assert (S.dim, D.dim) == (924, 792)
        coef = np.array([[1, 1, 0, 0], [1, 1j, 0, 0], [0, 0, 1, -1j], [1, 0, 0, 1]], dtype=np.complex128)
        _check_against_numpy(cfg, orc, (6, 0), (7, 0), 1, [0, Ns, 1, Ns + 1], coef, _random(S.dim, True, 23), S, D)


def test_seed_batch_argument_errors():
    import torch

    cfg = make_config(Norb=2, Nbath=5, Nspin=1, bath_type="hybrid", bath="random", seed=3)
    Ns = cfg.Ns
    with Sector(cfg, 3, 3, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 4, 3, stored=False, direct=True, real=True) as D:
        x = torch.from_numpy(_random(S.dim, False, 1)).cuda()
        one = np.ones((1, 2))
        assert _seed_batch(S, D, 1, [0, 1], one, x)[0] == 0
        assert _seed_batch(S, D, 1, [0, Ns], one, x)[0] == 1                      # levels reach different sectors
        assert _seed_batch(S, D, 1, [0, 1], np.array([[1, 1j]]), x)[0] == 1       # imaginary coefficient, vtype 0
        assert _seed_batch(S, D, 1, [0, 1], np.ones((33, 2)), x)[0] == 1          # nseed = 33
        assert _seed_batch(S, D, 1, list(range(7)), np.ones((1, 7)), x)[0] == 1   # nlev = 7
        assert _seed_batch(S, D, 1, [0, 0], one, x)[0] == 1                       # repeated level


def test_seed_batch_refuses_seeds_overlapping_the_vector():
    """Norb = 1, Nbath = 1, (1, 1) -> (2, 1), one seed: the gather reads the vector while other threads store
    output rows, so an output that shares one element with it is refused before any launch."""
    import torch

    cfg = make_config(Norb=1, Nbath=1)
    with Sector(cfg, 1, 1, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 2, 1, stored=False, direct=True, real=True) as D:
        ds, dd = S.dim, D.dim
        assert (ds, dd) == (4, 2)
        xh = _random(ds, False, 1)
        levels, coef = [0, 1], np.ones((1, 2))
        rc, ref, ref2 = _seed_batch(S, D, 1, levels, coef, torch.from_numpy(xh).cuda())
        assert rc == 0 and not np.any(np.isnan(ref)) and ref2[0] > 0
        # the vector's last element is the first of the output
        buf = torch.full((ds + dd,), float("nan"), dtype=torch.float64, device="cuda")
        buf[:ds] = torch.from_numpy(xh)
        rc, after, n2 = _seed_batch(S, D, 1, levels, coef, buf[:ds], out=buf[ds - 1:ds - 1 + dd])
        assert rc == 1 and after[0] == xh[-1] and np.all(np.isnan(after[1:])) and np.all(np.isnan(n2))
        # the output's last element is the first of the vector
        buf2 = torch.full((dd - 1 + ds,), float("nan"), dtype=torch.float64, device="cuda")
        buf2[dd - 1:] = torch.from_numpy(xh)
        rc, after, n2 = _seed_batch(S, D, 1, levels, coef, buf2[dd - 1:], out=buf2[:dd])
        assert rc == 1 and after[-1] == xh[0] and np.all(np.isnan(after[:-1])) and np.all(np.isnan(n2))
        assert np.array_equal(buf[:ds].cpu().numpy(), xh) and np.array_equal(buf2[dd - 1:].cpu().numpy(), xh)
        # the output right behind the vector is accepted
        rc, after, n2 = _seed_batch(S, D, 1, levels, coef, buf[:ds], out=buf[ds:])
        assert rc == 0 and np.array_equal(after, ref[0]) and np.array_equal(n2, ref2)


def test_sector_method_and_out_argument():
    import torch

    cfg = make_config(Norb=2, Nbath=5, Nspin=1, bath_type="hybrid", bath="random", seed=3)
    with Sector(cfg, 3, 3, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 4, 3, stored=False, direct=True, real=True) as D:
        xh, coef = _random(S.dim, False, 4), _coefs9(False)
        rc, ref, ref2 = _seed_batch(S, D, 1, [0, 1, 2], coef, torch.from_numpy(xh).cuda())
        assert rc == 0
        seeds, n2 = S.seed_batch(xh, D, 1, [0, 1, 2], coef)
        assert seeds.shape == (9, D.dim) and seeds.is_cuda and seeds.dtype == torch.float64 and n2.shape == (9,)
        assert np.array_equal(seeds.cpu().numpy(), ref) and np.array_equal(n2, ref2)      # the raw call's bits
        out = torch.full((9, D.dim), float("nan"), dtype=torch.float64, device="cuda")
        seeds2, n22 = S.seed_batch(torch.from_numpy(xh).cuda(), D, 1, [0, 1, 2], coef, out=out)
        assert seeds2 is out and torch.equal(seeds, out) and np.array_equal(n2, n22)
        rows = torch.full((12, D.dim), float("nan"), dtype=torch.float64, device="cuda")
        S.seed_batch(xh, D, 1, [0, 1, 2], coef, out=rows[2:11])                           # rows of a larger tensor
        assert torch.equal(rows[2:11], seeds) and bool(torch.isnan(rows[:2]).all()) and bool(torch.isnan(rows[11:]).all())
        for bad in (torch.empty((8, D.dim), dtype=torch.float64, device="cuda"),             # shape
                    torch.empty((9, D.dim), dtype=torch.complex128, device="cuda"),          # dtype
                    torch.empty((D.dim, 9), dtype=torch.float64, device="cuda").T):          # not contiguous
            with pytest.raises(ValueError):
                S.seed_batch(xh, D, 1, [0, 1, 2], coef, out=bad)


# ------------------------------------------------------------ fused seeds in build_gf
@pytest.mark.parametrize("name", ["H3", "nonsu2"])
def test_fused_seeds_match_the_unfused_path(name):
    """eps: orbmix_truth.EPS for H3; 0.1 for the nonSU2 model (sectors of at
    most 252 rows, as H2's)."""
    if name == "H3":
        cfg, sl, eps = ot.truth("H3").cfg, states("H3"), ot.EPS["H3"]
    else:
        cfg = make_config(Norb=1, Nbath=4, Nspin=2, ed_mode="nonsu2", bath="random", seed=5)
        sl, eps = ed_diag(cfg, DiagOptions())[1], 0.1
    r0, r1 = [], []
    G0 = build_gf(cfg, sl, GFOptions(Lmats=32, Lreal=32, eps=eps), record=r0)
    G1 = build_gf(cfg, sl, GFOptions(Lmats=32, Lreal=32, eps=eps, fused_seeds=True), record=r1)
    dm = np.max(np.abs(G0[0] - G1[0])) / np.max(np.abs(G0[0]))
    dr = np.max(np.abs(G0[1] - G1[1])) / np.max(np.abs(G0[1]))
    dn = max(abs(a["norm2"] - b["norm2"]) / a["norm2"] for a, b in zip(r0, r1))
    print(f"{name}: fused vs unfused G(iw) {dm:.2e}, G(w) {dr:.2e}, norm2 {dn:.2e}, {len(r0)} seeds")
    assert len(r0) == len(r1) > 0
    assert [(a["channel"], a["isector"], a["op"], a["nlanc"]) for a in r0] == \
        [(b["channel"], b["isector"], b["op"], b["nlanc"]) for b in r1]
    assert dm < 1e-12 and dr < 1e-8


def test_seed_buffer_chunking_gives_the_same_arrays(monkeypatch):
    """SEED_BUFFER_BYTES below one seed: gf.seed_fractions builds and tridiagonalises the fused seeds of H3
    one row at a time."""
    from edgpu import gf as gfmod

    cfg, sl = ot.truth("H3").cfg, states("H3")
    rec_w, rec_s = [], []
    whole = build_gf(cfg, sl, gopt("H3", fused_seeds=True), record=rec_w)
    monkeypatch.setattr(gfmod, "SEED_BUFFER_BYTES", 1)
    split = build_gf(cfg, sl, gopt("H3", fused_seeds=True), record=rec_s)
    assert len(rec_w) == len(rec_s) > 0
    assert [(r["channel"], r["isector"], r["op"], r["norm2"]) for r in rec_w] == \
        [(r["channel"], r["isector"], r["op"], r["norm2"]) for r in rec_s]
    for a, b in zip(whole, split):
        print(f"whole against split: {np.max(np.abs(a - b)) / np.max(np.abs(a)):.1e}")
    for a, b in zip(whole, split):
        assert np.any(a != 0) and np.array_equal(a, b)
