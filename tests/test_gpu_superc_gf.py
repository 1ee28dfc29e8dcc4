"""Superconducting Green's function (build_gf_superc, ED_GF_SUPERC.f90:18-77,
88-446) and the mixed-operator fused seed kernel (ed_sector_seed_plan,
k_seed_plan) on the MI355X, against the dense direct sum of superc_truth.

Bars: G(iw), F(iw) 1e-10 of max(|G|, |F|); G(w), F(w) 1e-5 at the per-model
broadening superc_truth.EPS (test_superc_gf_cpu's docstring has the table
that fixes it); fused against unfused seeds 1e-12 of max|G| on the Matsubara
axis; ed_sector_seed_plan against numpy seeds: the bars test_gpu_orbmix holds
ed_sector_seed_batch to (normalised seeds 1e-14, norm2 1e-13, the unnormalised
seed within 2 ulp of the apply_op chain).

Measured on the MI355X, (iw) / (w) against the dense truth: S1 (2 states)
6.7e-15 / 4.3e-14, S2 (3 states) 2.9e-14 / 7.4e-06, SH (2 states, eps 0.1)
7.9e-15 / 3.3e-07; thermal S1 (7 states, 2 twin entries) 4.7e-15 / 3.4e-14.
S2 fused against unfused: G(iw) 1.1e-14, F(iw) 7.0e-15, norm2 3.2e-16 (36
seeds).  ed_sector_seed_plan against the numpy seeds over all ten shapes:
normalised seeds <= 1.2e-16, norm2 <= 3.4e-16, the unnormalised seed within
2.0 ulp of the apply_op chain (scale and back); 646,646 target rows (the
grid-stride loop): 1.8e-18, 2.3e-16, 2.0 ulp.
"""
import ctypes

import numpy as np
import pytest

import superc_truth as st
from edgpu import _lib
from edgpu.diag import DiagOptions, ed_diag, post_diag
from edgpu.gf import GFOptions, build_gf_superc, matsubara, realaxis
from edgpu.hamiltonian import Sector
from edgpu.params import make_config

pytestmark = pytest.mark.gpu

MODELS = ["S1", "S2", "SH"]
_DIAG, _GF = {}, {}
P = ctypes.c_void_p


def gopt(name, **kw):
    return GFOptions(Lmats=32, Lreal=32, eps=st.EPS[name], **kw)


def states(name):
    if name not in _DIAG:
        _DIAG[name] = ed_diag(st.truth(name).cfg, DiagOptions())[1]
    return _DIAG[name]


def gf(name):
    """ed_diag + build_gf_superc with the default host path, once per model."""
    if name not in _GF:
        _GF[name] = build_gf_superc(st.truth(name).cfg, states(name), gopt(name))
    return _GF[name]


@pytest.mark.parametrize("name", MODELS)
def test_g_and_f_match_the_dense_truth(name):
    T, g, sl = st.truth(name), gopt(name), states(name)
    cfg = T.cfg
    wm, wr = matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal)
    got = gf(name)
    dm, dr, ratio = st.distances(T.gf_of_list(sl, wm, wr, g.eps), got, wm, wr, g.eps)
    print(f"{name}: {sl.size} state(s), eps {g.eps}: (iw) {dm:.2e}, (w) {dr:.2e}; truth max|F|/max|G| {ratio:.3f}")
    assert ratio > 0.05
    assert dm < 1e-10 and dr < 1e-5
    for arr in got:
        assert arr.shape == (1, 1, cfg.Norb, cfg.Norb, 32)
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                assert np.any(arr[0, 0, a, b]) == (a == b)      # [a, b != a] is not built: exactly zero


def test_thermal_list_with_twin_vectors():
    """Thermal list of S1 with ed_twin: the twin entries' vectors are rebuilt
    on the device (with superc_twin_sign) and feed all six seeds."""
    T = st.truth("S1")
    opt = DiagOptions(lanc_nstates_total=st.NTOTAL, beta=st.BETA, cutoff=st.CUTOFF, ed_twin=True)
    _, sl = ed_diag(T.cfg, opt)
    sl2, _ = post_diag(sl, opt, T.cfg)
    kept = T.thermal_states()
    assert sl2.size == len(kept) and sum(p is not None for p in sl2.twin_of) >= 1
    assert np.max(np.abs(np.sort(sl2.energies) - np.array([t[0] for t in kept]))) < 1e-10
    g = gopt("S1", beta=st.BETA)
    wm, wr = matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal)
    got = build_gf_superc(T.cfg, sl2, g)
    dm, dr, ratio = st.distances(T.gf_thermal(wm, wr, g.eps), got, wm, wr, g.eps)
    print(f"thermal S1: {sl2.size} states, {sum(p is not None for p in sl2.twin_of)} twin entries: (iw) {dm:.2e}, "
          f"(w) {dr:.2e}; truth max|F|/max|G| {ratio:.3f}")
    assert ratio > 0.05 and dm < 1e-10 and dr < 1e-5


def test_host_paths_bit_identical_and_fused_seeds():
    cfg, sl = st.truth("S2").cfg, states("S2")
    rb, rf = [], []
    Gb = build_gf_superc(cfg, sl, gopt("S2"), record=rb)                         # batch=True
    G1 = build_gf_superc(cfg, sl, gopt("S2", batch=False, workers=1))
    G4 = build_gf_superc(cfg, sl, gopt("S2", batch=False, workers=4))
    for a, b, c, d in zip(Gb, G1, G4, gf("S2")):
        assert np.any(a != 0)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a, d)
    Gf = build_gf_superc(cfg, sl, gopt("S2", fused_seeds=True), record=rf)
    scale = np.max(np.abs(Gb[0]))
    dg, df = np.max(np.abs(Gf[0] - Gb[0])) / scale, np.max(np.abs(Gf[2] - Gb[2])) / scale
    dn = max(abs(x["norm2"] - y["norm2"]) / x["norm2"] for x, y in zip(rb, rf))
    print(f"S2 fused vs unfused: G(iw) {dg:.2e}, F(iw) {df:.2e}, norm2 {dn:.2e}, {len(rb)} seeds")
    assert len(rb) == len(rf) > 0
    assert [(x["channel"], x["isector"], x["op"], x["nlanc"]) for x in rb] == \
        [(y["channel"], y["isector"], y["op"], y["nlanc"]) for y in rf]
    assert dg < 1e-12 and df < 1e-12


# ------------------------------------------------------------ the kernel alone
def _seed_plan(src, dst, levels, ops, terms, x, nlev=None, nseed=None, vtype=None, out=None):
    """(rc, seeds, norm2) of one ed_sector_seed_plan call; the output (`out`, or a tensor of its own) starts as NaN."""
    import torch

    lev = np.ascontiguousarray(levels, dtype=np.int32)
    op = np.ascontiguousarray(ops, dtype=np.int32)
    tt = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1, 2)
    ns = len(tt) if nseed is None else nseed
    if out is None:
        out = torch.full((max(len(tt), 1), dst.dim), float("nan"), dtype=x.dtype, device=x.device)    # written whole
    n2 = np.full(max(len(tt), 1), np.nan)
    stream = torch.cuda.current_stream()
    rc = _lib.load().ed_sector_seed_plan(src.handle, dst.handle, len(lev) if nlev is None else nlev,
                                         P(lev.ctypes.data), P(op.ctypes.data), ns, P(tt.ctypes.data),
                                         (1 if x.is_complex() else 0) if vtype is None else vtype,
                                         P(x.data_ptr()), P(out.data_ptr()), P(n2.ctypes.data), P(stream.cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), n2


def _chain(src, dst, terms, x):
    """ed_sector_apply_op + ed_sector_apply_op_acc(coef = 1): the unfused seed, unnormalised."""
    import torch

    L, stream = _lib.load(), torch.cuda.current_stream()
    vt = 1 if x.is_complex() else 0
    y = torch.empty(dst.dim, dtype=x.dtype, device=x.device)
    (lv, o), rest = terms[0], terms[1:]
    _lib.check(L.ed_sector_apply_op(src.handle, dst.handle, o, lv, vt, P(x.data_ptr()), P(y.data_ptr()),
                                    P(stream.cuda_stream)), "apply_op")
    for lv, o in rest:
        _lib.check(L.ed_sector_apply_op_acc(src.handle, dst.handle, o, lv, 1.0, 0.0, vt, P(x.data_ptr()),
                                            P(y.data_ptr()), P(stream.cuda_stream)), "apply_op_acc")
    return y.cpu().numpy()


def _numpy_image(map_src, map_dst, level, op, x):
    """op on `level` of x (rows of map_src) in the rows of map_dst, as the vvinit loops build it."""
    occ = (map_src >> np.uint32(level)) & np.uint32(1)
    sel = occ == (0 if op == 1 else 1)
    s = map_src[sel]
    below = s & np.uint32((1 << level) - 1)
    par = np.zeros(len(s), dtype=np.int64)
    for b in range(level):
        par += (below >> np.uint32(b)) & np.uint32(1)
    j = np.searchsorted(map_dst, s ^ np.uint32(1 << level))
    assert np.array_equal(map_dst[j], s ^ np.uint32(1 << level))
    v = np.zeros(len(map_dst), dtype=x.dtype)
    v[j] = (1.0 - 2.0 * (par % 2)) * x[sel]
    return v


def _random(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0.0)
    return v / np.linalg.norm(v)


def _plan_for(cfg, dsz):
    """The images and seeds of one target sector, every orbital: (levels, ops, terms)."""
    Ns, ops = cfg.Ns, ((1, 0) if dsz > 0 else (0, 1))          # raise: c+_up, c_dw; lower: c_up, c+_dw
    levels, lops, terms = [], [], []
    for a in range(cfg.Norb):
        p = len(levels)
        levels += [a, a + Ns]
        lops += list(ops)
        terms += [(p, -1), (p + 1, -1), (p, p + 1)]
    return levels, lops, terms


SHAPES = {
    "S2": (lambda: st.config("S2"), (70, 56)),
    "Ns6": (lambda: make_config(Norb=2, Nbath=2, ed_mode="superc", deltasc=0.2, bath="random", seed=3), (924, 792)),
    # the target has more rows than 1,024 blocks x 256 threads: the grid-stride loop runs
    "Ns11": (lambda: make_config(Norb=1, Nbath=10, ed_mode="superc", deltasc=0.2), (705432, 646646)),
}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape,dsz", [("S2", +1), ("S2", -1), ("Ns6", +1), ("Ns6", -1), ("Ns11", +1)])
def test_seed_plan_matches_numpy_seeds(shape, dsz, cplx):
    import torch

    mk, dims = SHAPES[shape]
    cfg = mk()
    levels, ops, terms = _plan_for(cfg, dsz)
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, dsz, 0, stored=False, direct=True, real=True) as D:
        assert (S.dim, D.dim) == dims and D.dim == dims[1]
        ms, md = S.map(), D.map()
        if shape != "Ns11":
            from oracle.oracle import Oracle

            assert np.array_equal(ms, Oracle(cfg).build_sector(0, 0))
        xh = _random(S.dim, cplx, 17)
        x = torch.from_numpy(xh).cuda()
        rc, seeds, n2 = _seed_plan(S, D, levels, ops, terms, x)
        assert rc == 0, _lib.load().ed_gpu_last_error()
        rc2, seeds2, n22 = _seed_plan(S, D, levels, ops, terms, x)
        assert rc2 == 0 and seeds.tobytes() == seeds2.tobytes() and n2.tobytes() == n22.tobytes()
        img = [_numpy_image(ms, md, lv, o, xh) for lv, o in zip(levels, ops)]
        worst_v = worst_n = worst_ulp = 0.0
        for s, (p, q) in enumerate(terms):
            ref = img[p] + img[q] if q >= 0 else img[p]
            r2 = float(np.vdot(ref, ref).real)
            assert r2 > 0
            worst_n = max(worst_n, abs(n2[s] - r2) / r2)
            worst_v = max(worst_v, np.max(np.abs(seeds[s] - ref / np.sqrt(r2))))
            if not cplx:
                assert seeds.dtype == np.float64          # unit coefficients: a real vector gives real seeds
            ch = _chain(S, D, [(levels[p], ops[p])] + ([(levels[q], ops[q])] if q >= 0 else []), x)
            un = seeds[s] * np.sqrt(n2[s])
            for a, b in ((un.real, ch.real), (un.imag, ch.imag)):
                nz = b != 0
                assert np.all(a[~nz] == 0)
                if np.any(nz):
                    worst_ulp = max(worst_ulp, np.max(np.abs(a[nz] - b[nz]) / np.spacing(np.abs(b[nz]))))
    print(f"{shape} sz 0->{dsz:+d} dims {dims} cplx={cplx} nseed={len(terms)} nlev={len(levels)}: "
          f"seed {worst_v:.2e}, norm2 {worst_n:.2e}, chain {worst_ulp:.1f} ulp")
    assert worst_v <= 1e-14 and worst_n <= 1e-13 and worst_ulp <= 2.0


def test_seed_plan_zero_seed():
    """A seed no row contributes to comes back all zero with norm2 = 0; its neighbour is untouched by that."""
    import torch

    cfg = st.config("S2")
    Ns = cfg.Ns
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 0, stored=False, direct=True, real=True) as D:
        hmap = S.map()
        m = 33
        up_occ = [lv for lv in range(Ns) if (hmap[m] >> lv) & 1]
        up_free = [lv for lv in range(Ns) if not (hmap[m] >> lv) & 1]
        assert up_occ and up_free
        e = np.zeros(S.dim)
        e[m] = 1.0
        # c+ on an occupied up level of the only populated state: nothing; on a free one: one element
        rc, seeds, n2 = _seed_plan(S, D, [up_occ[0], up_free[0]], [1, 1], [(0, -1), (1, -1), (0, 1)],
                                   torch.from_numpy(e).cuda())
        assert rc == 0
        assert n2[0] == 0.0 and not np.any(seeds[0])
        assert n2[1] == 1.0 and np.count_nonzero(seeds[1]) == 1 and np.max(np.abs(seeds[1])) == 1.0
        assert n2[2] == 1.0 and np.array_equal(seeds[2], seeds[1])


def test_seed_plan_refusals_leave_the_output_untouched():
    import torch

    cfg = st.config("S2")
    Ns = cfg.Ns
    ERR_ARG, ERR_UNSUPPORTED = 1, 5
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 0, stored=False, direct=True, real=True) as D, \
            Sector(cfg, -1, 0, stored=False, direct=True, real=True) as Dm, \
            Sector(cfg, 1, 0, stored=True, real=True, rows=(0, 20)) as Drow:
        x = torch.from_numpy(_random(S.dim, False, 1)).cuda()
        ok = dict(levels=[0, Ns], ops=[1, 0], terms=[(0, 1)])

        def refused(code=ERR_ARG, src=S, dst=D, **kw):
            a = dict(ok, **kw)
            extra = {k: a.pop(k) for k in ("nlev", "nseed", "vtype") if k in a}
            rc, seeds, n2 = _seed_plan(src, dst, a["levels"], a["ops"], a["terms"], x, **extra)
            assert rc == code, (kw, rc)
            assert np.all(np.isnan(seeds)) and np.all(np.isnan(n2)), kw      # nothing was launched

        rc, seeds, n2 = _seed_plan(S, D, ok["levels"], ok["ops"], ok["terms"], x)
        assert rc == 0 and not np.any(np.isnan(seeds)) and not np.any(np.isnan(n2))
        refused(dst=Dm)                                        # every image reaches the other sector
        refused(ops=[1, 1])                                    # c+_dw lowers sz: check_op_target of the second image
        refused(levels=[0, 2 * Ns])                            # level outside the 2*Ns Fock levels
        refused(ops=[1, 2])                                    # op outside {0, 1}
        refused(levels=[0, Ns, 0], ops=[1, 0, 1])              # duplicate (level, op)
        refused(levels=[], ops=[], nlev=0)                     # nlev = 0
        refused(levels=[0, 1, 2, 3, Ns, Ns + 1, Ns + 2], ops=[1, 1, 1, 1, 0, 0, 0])     # nlev = 7
        refused(terms=[(0, 1)], nseed=0)                       # nseed = 0
        refused(terms=[(0, -1)] * 33)                          # nseed = 33
        refused(terms=[(0, 2)])                                # q >= nlev
        refused(terms=[(2, -1)])                               # p >= nlev
        refused(terms=[(-1, 0)])                               # p < 0
        refused(terms=[(1, 1)])                                # p = q
        refused(vtype=2)                                       # vtype outside {0, 1}
        refused(code=ERR_UNSUPPORTED, dst=Drow)                # whole sectors only, as ed_sector_seed_batch
        # the six images of Norb = 2 plus two bath levels are accepted: nlev = kSeedMaxLev
        rc, _, _ = _seed_plan(S, D, [0, 1, 2, Ns, Ns + 1, Ns + 2], [1, 1, 1, 0, 0, 0], [(0, 5), (2, 3)], x)
        assert rc == 0


def test_seed_plan_refuses_seeds_overlapping_the_vector():
    """S2, sz 0 -> +1, one seed: an output that shares one element with the vector is refused before any
    launch (the gather reads the vector while other threads store output rows)."""
    import torch

    cfg = st.config("S2")
    levels, ops, terms = [0, cfg.Ns], [1, 0], [(0, 1)]
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 0, stored=False, direct=True, real=True) as D:
        ds, dd = S.dim, D.dim
        xh = _random(ds, False, 1)
        rc, ref, ref2 = _seed_plan(S, D, levels, ops, terms, torch.from_numpy(xh).cuda())
        assert rc == 0 and not np.any(np.isnan(ref)) and ref2[0] > 0
        # the vector's last element is the first of the output
        buf = torch.full((ds + dd,), float("nan"), dtype=torch.float64, device="cuda")
        buf[:ds] = torch.from_numpy(xh)
        rc, after, n2 = _seed_plan(S, D, levels, ops, terms, buf[:ds], out=buf[ds - 1:ds - 1 + dd])
        assert rc == 1 and after[0] == xh[-1] and np.all(np.isnan(after[1:])) and np.all(np.isnan(n2))
        # the output's last element is the first of the vector
        buf2 = torch.full((dd - 1 + ds,), float("nan"), dtype=torch.float64, device="cuda")
        buf2[dd - 1:] = torch.from_numpy(xh)
        rc, after, n2 = _seed_plan(S, D, levels, ops, terms, buf2[dd - 1:], out=buf2[:dd])
        assert rc == 1 and after[-1] == xh[0] and np.all(np.isnan(after[:-1])) and np.all(np.isnan(n2))
        assert np.array_equal(buf[:ds].cpu().numpy(), xh) and np.array_equal(buf2[dd - 1:].cpu().numpy(), xh)
        # the output right behind the vector is accepted
        rc, after, n2 = _seed_plan(S, D, levels, ops, terms, buf[:ds], out=buf[ds:])
        assert rc == 0 and np.array_equal(after, ref[0]) and np.array_equal(n2, ref2)


def test_sector_method_and_out_argument():
    import torch

    cfg = st.config("S2")
    levels, ops, terms = _plan_for(cfg, +1)
    ns = len(terms)
    with Sector(cfg, 0, 0, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 0, stored=False, direct=True, real=True) as D:
        xh = _random(S.dim, False, 4)
        rc, ref, ref2 = _seed_plan(S, D, levels, ops, terms, torch.from_numpy(xh).cuda())
        assert rc == 0
        seeds, n2 = S.seed_plan(xh, D, levels, ops, terms)
        assert seeds.shape == (ns, D.dim) and seeds.is_cuda and seeds.dtype == torch.float64 and n2.shape == (ns,)
        assert np.array_equal(seeds.cpu().numpy(), ref) and np.array_equal(n2, ref2)      # the raw call's bits
        out = torch.full((ns, D.dim), float("nan"), dtype=torch.float64, device="cuda")
        seeds2, n22 = S.seed_plan(torch.from_numpy(xh).cuda(), D, levels, ops, terms, out=out)
        assert seeds2 is out and torch.equal(seeds, out) and np.array_equal(n2, n22)
        for bad in (torch.empty((ns + 1, D.dim), dtype=torch.float64, device="cuda"),        # shape
                    torch.empty((ns, D.dim), dtype=torch.complex128, device="cuda"),         # dtype
                    torch.empty((D.dim, ns), dtype=torch.float64, device="cuda").T):         # not contiguous
            with pytest.raises(ValueError):
                S.seed_plan(xh, D, levels, ops, terms, out=bad)
        with pytest.raises(ValueError):
            S.seed_plan(xh, D, levels, ops[:-1], terms)                                      # one op per level


def test_seed_buffer_chunking_gives_the_same_arrays(monkeypatch):
    """SEED_BUFFER_BYTES below one seed: gf.seed_fractions builds and tridiagonalises the fused seeds of S2
    one row at a time."""
    from edgpu import gf as gfmod

    cfg, sl = st.truth("S2").cfg, states("S2")
    rec_w, rec_s = [], []
    whole = build_gf_superc(cfg, sl, gopt("S2", fused_seeds=True), record=rec_w)
    monkeypatch.setattr(gfmod, "SEED_BUFFER_BYTES", 1)
    split = build_gf_superc(cfg, sl, gopt("S2", fused_seeds=True), record=rec_s)
    assert len(rec_w) == len(rec_s) > 0
    assert [(r["channel"], r["isector"], r["op"], r["norm2"]) for r in rec_w] == \
        [(r["channel"], r["isector"], r["op"], r["norm2"]) for r in rec_s]
    for a, b in zip(whole, split):
        print(f"whole against split: {np.max(np.abs(a - b)) / np.max(np.abs(a)):.1e}")
    for a, b in zip(whole, split):
        assert np.any(a != 0) and np.array_equal(a, b)
