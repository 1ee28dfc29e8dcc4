"""Pair and inter-orbital density susceptibilities on the MI355X: the
two-operator seed kernel (ed_sector_seed_pair, k_seed_pair) against
forward-form numpy seeds and against the unfused apply_op chain, the signed
pole sum (ed_chi_add_poles_signed) against chi_pair_host.chi_poles_host_signed,
and edgpu.chi.build_chi(pair=True, exc=True) against the dense Lehmann sums of
chi_pair_truth.

Bars (those of test_gpu_chi).  Seeds: the unnormalised values exact — the
device row is the numpy row (one exact sign product, one product and at most
one addition, in the same order) times the one scale factor 1/sqrt(norm2) of
its seed, where that factor may be the correctly rounded one or a neighbour;
norm2 1e-13 relative; the same bits from two calls; against the chain the
same rule with the chain's unnormalised values in the numpy row's place.  Pole
sum: 1e-13 of the sum of |terms| per grid point.  build_chi: chi(iv) and
chi(tau) 1e-10 of each array's maximum, chi(w) 1e-5 at eps = 0.01
(chi_pair_truth.EPS, the table in test_chi_pair_cpu's docstring).

Measured on the MI355X.  Seeds: every one of the 216 seeds over all shapes
exact with the correctly rounded scale factor (no neighbour needed), norm2
within 2.5e-16, 273,273 target rows: 1.9e-16 (real and complex); the 12 seeds
of the chain test bit-equal to the unfused chain, real and complex.  Pole sum:
iv 2.4e-16, tau 1.9e-16, w 1.9e-16 of the sum of |terms|.  build_chi against
the truth (iv / tau / w): C1 (2 states) 5.9e-16 / 5.5e-16 / 7.4e-15, C2 (3
states) 9.4e-16 / 8.5e-16 / 3.5e-14, CN 2.2e-16 / 5.7e-16 / 5.6e-16, thermal
C1 (7 states, 2 twin entries) 4.0e-15 / 1.1e-15 / 2.7e-14.  One-seed calls
against whole calls on C2: the same arrays bit for bit.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import chi_pair_truth as pt
import chi_truth as ct
from chi_pair_host import chi_poles_host_signed, numpy_pair_seeds
from edgpu import _lib, chi, gf
from edgpu.diag import DiagOptions, ed_diag, post_diag
from edgpu.hamiltonian import Sector
from edgpu.params import make_config

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = 1, 5
_DIAG = {}


# ------------------------------------------------------------ the seed kernel
def _seed_pair(S, D, images, terms, x, nimg=None, nseed=None, vtype=None, out=None):
    """(rc, seeds, norm2) of one ed_sector_seed_pair call; the output starts as NaN."""
    import torch

    im = np.ascontiguousarray(images, dtype=np.int32).reshape(-1)
    tm = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1)
    ns = tm.size // 2 if nseed is None else nseed
    if out is None:
        out = torch.full((max(ns, 1), D.dim), float("nan"), dtype=x.dtype, device=x.device)      # written whole
    n2 = np.full(max(ns, 1), np.nan)
    stream = torch.cuda.current_stream()
    rc = _lib.load().ed_sector_seed_pair(S.handle, D.handle, im.size // 4 if nimg is None else nimg, P(im.ctypes.data),
                                         ns, P(tm.ctypes.data), (1 if x.is_complex() else 0) if vtype is None else vtype,
                                         P(x.data_ptr()), P(out.data_ptr()), P(n2.ctypes.data), P(stream.cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), n2


def _random(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0.0)
    return v / np.linalg.norm(v)


def _images(kind, Ns, nonsu2):
    """Twelve distinct images of one kind: "down" (two electrons fewer: one up and one down in normal mode),
    "up" (two more) or "same" (c^+ c within one spin species / any two levels in nonsu2); lev2 < lev1 and
    lev2 > lev1 alternate."""
    if kind == "same":
        if nonsu2:
            pairs = [(i, j) for i in range(2 * Ns) for j in range(2 * Ns) if i != j][:12]
        else:
            pairs = [(i, j) for i in range(3) for j in range(3) if i != j]
            pairs += [(Ns + i, Ns + j) for i, j in pairs]
        return [(i, 0, j, 1) for i, j in pairs]
    op = 1 if kind == "up" else 0
    if nonsu2:
        pairs = [(i, j) for i in range(2 * Ns) for j in range(i + 1, 2 * Ns)][:12]
    else:
        pairs = [(i, Ns + j) for i in range(3) for j in range(4)]
    return [(i, op, j, op) if n % 2 else (j, op, i, op) for n, (i, j) in enumerate(pairs)]


def _tables(kind, Ns, nonsu2):
    """(images, terms, never): nimg = 1 with one seed; nimg = 12 with 12 seeds, one-image and two-image ones
    mixed; two images that no row has both of, alone and summed."""
    im = _images(kind, Ns, nonsu2)
    assert len(im) == 12 and len(set(im)) == 12
    twelve = [(s, -1) if s % 2 == 0 else (s, (s + 5) % 12) for s in range(12)]
    if kind == "same":
        a, b = (im[0][0], im[0][2])
        never = [(a, 0, b, 1), (b, 0, a, 1)]            # the first needs b occupied and a empty in the row, the second the reverse
    elif kind == "up":
        never = [(0, 1, Ns, 1), (Ns + 1, 1, 0, 1)]      # these two can meet: the flag below stays off
    else:
        never = [(0, 0, Ns, 0), (Ns + 1, 0, 0, 0)]
    return [([im[3]], [(0, -1)], False), (im, twelve, False), (never, [(0, -1), (1, -1), (0, 1)], kind == "same")]


def _check_seeds(ref, seeds, n2):
    """Returns (norm2 distance, number of seeds scaled by a neighbour of 1/sqrt(norm2), zero seeds)."""
    worst_n, off, zero = 0.0, 0, 0
    for q in range(len(ref)):
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


N22 = lambda: make_config(Norb=2, Nbath=2, bath="random", seed=3)      # noqa: E731   Ns = 6
SHAPES = {
    # name: (config, src, dst, dim of dst, kind)
    "to_dim1": (N22, (1, 1), (0, 0), 1, "down"),                       # a dim-1 target
    "from_dim1": (N22, (0, 0), (1, 1), 36, "up"),                      # a dim-1 source, 36 rows: below one wave
    "two_blocks": (N22, (2, 2), (3, 3), 400, "up"),                    # 6.25 waves, 2 blocks
    "same": (N22, (3, 3), (3, 3), 400, "same"),                        # src == dst: the exc images
    "nonsu2_up": (lambda: ct.config("CN"), (3, 0), (5, 0), 6, "up"),
    "nonsu2_down": (lambda: ct.config("CN"), (3, 0), (1, 0), 6, "down"),
    # more rows than the launcher's 1,024 blocks x 256 threads = 262,144: the strided loop runs twice
    "stride": (lambda: make_config(Norb=2, Nbath=6), (1, 5), (2, 6), 273273, "up"),
}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_seed_pair_matches_forward_numpy_seeds(name, cplx):
    import torch

    mk, sq, dq, dim, kind = SHAPES[name]
    cfg = mk()
    real, nonsu2 = cfg.is_real(), cfg.ed_mode == "nonsu2"
    with contextlib.ExitStack() as stack:
        S = stack.enter_context(Sector(cfg, *sq, stored=False, direct=True, real=real))
        D = S if dq == sq else stack.enter_context(Sector(cfg, *dq, stored=False, direct=True, real=real))   # src == dst: one handle
        assert D.dim == dim
        ms, md = S.map(), D.map()
        xh = _random(S.dim, cplx, 17)
        x = torch.from_numpy(xh).cuda()
        tables = _tables(kind, cfg.Ns, nonsu2)
        if name == "stride":
            tables = [tables[1]]                         # nimg = 12, nseed = 12
        if name == "from_dim1":
            # a dim-1 source has one up and one down electron to add: two images on different up levels never meet
            tables[2] = ([(0, 1, cfg.Ns, 1), (1, 1, cfg.Ns, 1)], [(0, -1), (1, -1), (0, 1)], True)
        worst, off, zero, nseeds = 0.0, 0, 0, 0
        for images, terms, never in tables:
            rc, seeds, n2 = _seed_pair(S, D, images, terms, x)
            assert rc == 0, _lib.load().ed_gpu_last_error()
            rc2, seeds2, n22 = _seed_pair(S, D, images, terms, x)
            assert rc2 == 0 and seeds.tobytes() == seeds2.tobytes() and n2.tobytes() == n22.tobytes()
            assert seeds.dtype == (np.complex128 if cplx else np.float64)
            ref = numpy_pair_seeds(ms, md, images, terms, xh)
            if never:
                assert np.any(ref[0]) and np.any(ref[1]) and not np.any((ref[0] != 0) & (ref[1] != 0))
            a, b, c = _check_seeds(ref, seeds, n2)
            worst, off, zero, nseeds = max(worst, a), off + b, zero + c, nseeds + len(terms)
    print(f"{name} {sq}->{dq} dim {dim} cplx={cplx}: {nseeds} seeds exact ({off} with a neighbouring scale factor, "
          f"{zero} zero), norm2 {worst:.2e}")
    assert worst <= 1e-13


def _chain(S, M, D, image, x, y):
    """y += op2 op1 x through the intermediate sector M: apply_op, then apply_op_acc(coef = 1)."""
    import torch

    L, stream = _lib.load(), torch.cuda.current_stream()
    vt = 1 if x.is_complex() else 0
    lev1, op1, lev2, op2 = image
    mid = torch.empty(M.dim, dtype=x.dtype, device=x.device)
    _lib.check(L.ed_sector_apply_op(S.handle, M.handle, op1, lev1, vt, P(x.data_ptr()), P(mid.data_ptr()),
                                    P(stream.cuda_stream)), "apply_op")
    _lib.check(L.ed_sector_apply_op_acc(M.handle, D.handle, op2, lev2, 1.0, 0.0, vt, P(mid.data_ptr()), P(y.data_ptr()),
                                        P(stream.cuda_stream)), "apply_op_acc")
    torch.cuda.synchronize()


@pytest.mark.parametrize("cplx", [False, True])
def test_seed_pair_matches_the_unfused_chain(cplx):
    """(2, 2) -> (3, 3), the nimg = 12 table: every seed against ed_sector_apply_op into (3, 2) or (2, 3) and
    ed_sector_apply_op_acc from there, summed image by image into a zeroed vector."""
    import torch

    cfg = N22()
    Ns = cfg.Ns
    with Sector(cfg, 2, 2, stored=False, direct=True, real=True) as S, Sector(cfg, 3, 3, stored=False, direct=True, real=True) as D, \
            Sector(cfg, 3, 2, stored=False, direct=True, real=True) as Mu, Sector(cfg, 2, 3, stored=False, direct=True, real=True) as Md:
        images, terms, _ = _tables("up", Ns, False)[1]
        assert any(im[0] < Ns for im in images) and any(im[0] >= Ns for im in images)       # both intermediate sectors
        xh = _random(S.dim, cplx, 29)
        x = torch.from_numpy(xh).cuda()
        rc, seeds, n2 = _seed_pair(S, D, images, terms, x)
        assert rc == 0
        ref = []
        for p, q in terms:
            y = torch.zeros(D.dim, dtype=x.dtype, device=x.device)
            for l in (p,) + ((q,) if q >= 0 else ()):
                _chain(S, Mu if images[l][0] < Ns else Md, D, images[l], x, y)
            ref.append(y.cpu().numpy())
        ref = np.array(ref)
        assert np.array_equal(ref, numpy_pair_seeds(S.map(), D.map(), images, terms, xh))    # the chain is the forward form
        worst, off, zero = _check_seeds(ref, seeds, n2)
    print(f"chain cplx={cplx}: 12 seeds bit-equal to the unfused chain ({off} with a neighbouring scale factor, {zero} "
          f"zero), norm2 {worst:.2e}")
    assert zero == 0 and worst <= 1e-13


def test_sector_method_and_out_argument():
    import torch

    cfg = ct.config("C2")
    calls = chi.seed_pair_calls(cfg, True, True)
    with Sector(cfg, 2, 2, stored=True, real=True) as S, Sector(cfg, 1, 1, stored=True, real=True) as D:
        xh = _random(S.dim, False, 4)
        _, images, terms, _ = calls[0]
        seeds, n2 = S.seed_pair(xh, D, images, terms)
        assert seeds.shape == (2, D.dim) and seeds.is_cuda and n2.shape == (2,)
        out = torch.empty((2, D.dim), dtype=torch.float64, device="cuda")
        seeds2, n22 = S.seed_pair(torch.from_numpy(xh).cuda(), D, images, terms, out=out)
        assert seeds2 is out and torch.equal(seeds, out) and np.array_equal(n2, n22)
        a, _, _ = _check_seeds(numpy_pair_seeds(S.map(), D.map(), images, terms, xh), seeds.cpu().numpy(), n2)
        assert a < 1e-13
        with pytest.raises(ValueError):
            S.seed_pair(xh, D, images, terms, out=torch.empty((3, D.dim), dtype=torch.float64, device="cuda"))
        _, images, terms, _ = calls[2]                    # the exc seeds stay in the sector
        seeds, n2 = S.seed_pair(xh, S, images, terms)
        assert seeds.shape == (2, S.dim)
        a, _, _ = _check_seeds(numpy_pair_seeds(S.map(), S.map(), images, terms, xh), seeds.cpu().numpy(), n2)
        assert a < 1e-13


def test_seed_pair_refusals_leave_the_output_untouched():
    import torch

    cfg = ct.config("C2")
    Ns = cfg.Ns
    with Sector(cfg, 2, 2, stored=False, direct=True, real=True) as S, \
            Sector(cfg, 1, 1, stored=False, direct=True, real=True) as D, \
            Sector(cfg, 3, 3, stored=False, direct=True, real=True) as Dup, \
            Sector(cfg, 1, 1, stored=True, real=True, rows=(0, 8)) as Drow:
        xh = _random(S.dim, False, 1)
        x = torch.from_numpy(xh).cuda()
        ok = dict(images=[(Ns, 0, 0, 0), (Ns + 1, 0, 1, 0)], terms=[(0, -1), (0, 1)])
        thirteen = [(Ns + j, 0, i, 0) for i in range(4) for j in range(4)][:13]

        def refused(code=ERR_ARG, dst=D, **kw):
            a = dict(ok, **kw)
            extra = {k: a.pop(k) for k in ("nimg", "nseed", "vtype") if k in a}
            rc, seeds, n2 = _seed_pair(S, dst, a["images"], a["terms"], x, **extra)
            assert rc == code, (kw, rc)
            assert np.all(np.isnan(seeds)) and np.all(np.isnan(n2)), kw      # nothing was launched

        rc, seeds, n2 = _seed_pair(S, D, ok["images"], ok["terms"], x)
        assert rc == 0 and not np.any(np.isnan(seeds)) and not np.any(np.isnan(n2))
        refused(images=[(0, 0, 0, 0), (Ns + 1, 0, 1, 0)])                    # lev1 == lev2
        refused(dst=Dup)                                                     # a wrong dst
        refused(dst=S)                                                       # ... the source itself
        refused(images=ok["images"] + [ok["images"][0]])                     # duplicate images
        refused(terms=[(1, 1)])                                              # p == q
        refused(terms=[(0, 2)])                                              # q = nimg
        refused(images=thirteen, terms=[(0, -1)])                            # nimg = 13
        refused(terms=[(0, -1)] * 13)                                        # nseed = 13
        refused(images=[], terms=[(0, -1)], nimg=0)                          # nimg = 0
        refused(nseed=0)                                                     # nseed = 0
        refused(vtype=2)                                                     # vtype outside {0, 1}
        refused(code=ERR_UNSUPPORTED, dst=Drow)                              # whole sectors only
        # seeds overlapping src_vec: the vector's last element is the first of the output
        ds, dd = S.dim, D.dim
        buf = torch.full((ds + 2 * dd,), float("nan"), dtype=torch.float64, device="cuda")
        buf[:ds] = x
        rc, after, n2 = _seed_pair(S, D, ok["images"], ok["terms"], buf[:ds], out=buf[ds - 1:ds - 1 + 2 * dd])
        assert rc == ERR_ARG and after[0] == xh[-1] and np.all(np.isnan(after[1:])) and np.all(np.isnan(n2))
        # the output right behind the vector is accepted
        rc, after, n2 = _seed_pair(S, D, ok["images"], ok["terms"], buf[:ds], out=buf[ds:])
        assert rc == 0 and not np.any(np.isnan(after)) and not np.any(np.isnan(n2))
        # nimg = 12 and nseed = 12 are accepted
        rc, _, _ = _seed_pair(S, D, thirteen[:12], [(k, -1) for k in range(12)], x)
        assert rc == 0


# ------------------------------------------------------------ the signed pole sum
def _fractions(rng, signs):
    """Fractions that switch component back and forth, with a D == 0 pole and downward transitions; the sign
    selector cycles through `signs` so every component takes both-sign, +1-only and -1-only fractions."""
    out = []
    for n, (comp, npole) in enumerate(((0, 5), (2, 7), (0, 1), (1, 4), (2, 3), (2, 6), (0, 9), (1, 2), (1, 5))):
        ei = float(rng.normal())
        D = np.sort(rng.uniform(0.05, 3.0, size=npole))
        if npole >= 2:
            D[0] = -rng.uniform(0.1, 0.7)
        if npole >= 4:
            D[1] = 0.0
        z = rng.normal(size=npole)
        z /= np.linalg.norm(z)
        out.append((comp, float(rng.uniform(0.1, 2.0)), ei, ei + D, z, signs[n % len(signs)]))
    return out


def test_chi_add_poles_signed_matches_the_host_restatement():
    beta, eps, ncomp = 8.0, 0.05, 3
    Lmats, Ltau, Lreal = 37, 11, 65                     # 38 + 12 + 65 grid points: both inner boundaries fall inside waves
    vm, tg, wr = chi.bosonic_matsubara(beta, Lmats), chi.tau_grid(beta, Ltau), np.linspace(-4.0, 4.0, Lreal)
    rng = np.random.default_rng(43)
    first, second = _fractions(rng, (0, +1, -1, -1)), _fractions(rng, (+1, 0, -1))
    for comp in range(ncomp):
        assert {f[5] for f in first + second if f[0] == comp} == {0, 1, -1}
    ps = chi.ChiPoleSums(ncomp, vm, tg, wr, beta, eps, 0)
    for fr in first:
        ps.add(*fr)
    ps.flush()
    got1 = ps.to_host()
    ref1 = chi_poles_host_signed(first, beta, vm, tg, wr, eps, ncomp)
    for fr in second:
        ps.add(*fr)
    ps.flush()
    got2 = ps.to_host()
    ref2 = chi_poles_host_signed(second, beta, vm, tg, wr, eps, ncomp, start=ref1[:3])
    mag2 = [m1 + (m2 - np.abs(s)) for m1, m2, s in zip(ref1[3], ref2[3], ref1[:3])]      # sum |terms| of both flushes
    worst = []
    for got, ref, mag in ((got1, ref1[:3], ref1[3]), (got2, ref2[:3], mag2)):
        for g, r, m in zip(got, ref, mag):
            assert g.shape == r.shape and np.all(m > 0)
            worst.append(np.max(np.abs(g - r) / m))
    print("first flush iv %.2e tau %.2e w %.2e; second %.2e %.2e %.2e (of sum |terms| per grid point)" % tuple(worst))
    assert max(worst) <= 1e-13
    # a +1-only fraction differs from the both-sign one: the selector is not ignored
    one = chi_poles_host_signed([f[:5] + (0,) for f in first], beta, vm, tg, wr, eps, ncomp)
    assert np.max(np.abs(one[1] - ref1[1])) > 1e-3 * np.max(np.abs(ref1[1]))
    # a selector outside {0, +1, -1} is refused and nothing is added
    L = _lib.load()
    npole, E, z = np.array([1], dtype=np.int32), np.array([0.5]), np.array([1.0])
    peso, ei, comp, bad = np.array([1.0]), np.array([0.0]), np.array([0], dtype=np.int32), np.array([2], dtype=np.int32)
    rc = L.ed_chi_add_poles_signed(1, P(npole.ctypes.data), P(E.ctypes.data), P(z.ctypes.data), P(peso.ctypes.data),
                                   P(ei.ctypes.data), P(comp.ctypes.data), P(bad.ctypes.data), beta, P(ps.vm.data_ptr()),
                                   Lmats, P(ps.tg.data_ptr()), Ltau, P(ps.wr.data_ptr()), Lreal, eps, P(ps.iv.data_ptr()),
                                   P(ps.tau.data_ptr()), P(ps.w.data_ptr()), None)
    assert rc == ERR_ARG and all(np.array_equal(a, b) for a, b in zip(ps.to_host(), got2))


# ------------------------------------------------------------ build_chi
def states(name):
    if name not in _DIAG:
        _DIAG[name] = ed_diag(ct.truth(name).cfg, DiagOptions())[1]
    return _DIAG[name]


def _old_fields(c):
    return (c.spin_iv, c.spin_tau, c.spin_w, c.dens_iv, c.dens_tau, c.dens_w, c.dens_tot_iv, c.dens_tot_tau, c.dens_tot_w)


@pytest.mark.parametrize("name", ["C1", "C2", "CN"])
def test_build_chi_pair_and_exc_match_the_dense_truth(name):
    T, copt, sl = pt.truth(name), pt.options(name), states(name)
    cfg, No = T.cfg, T.cfg.Norb
    rec = []
    got = chi.build_chi(cfg, sl, copt, record=rec, pair=True, exc=True)
    d = pt.distances(T.pair_exc_of_list(sl, copt), got, No)
    print(f"{name}: {sl.size} state(s) in sectors {sl.sectors}, eps {copt.eps}: iv {d[0]:.2e}, tau {d[1]:.2e}, w {d[2]:.2e}; "
          f"smallest dynamic share {min(T.shares.values()):.2e}, smallest norm2 {T.min_amp2:.2e}")
    # queue order: kept state, its spin and density seeds, pair -1 by orbital, pair +1, every exc seed with +1 and -1
    old = [(n, 0) for n, _, _ in chi.seed_table(cfg)]
    new = ([(("pair", a), -1) for a in range(No)] + [(("pair", a), +1) for a in range(No)]
           + [x for a, b in chi.exc_pairs(cfg) for x in ((("exc", a, b), +1), (("exc", b, a), -1))])
    assert [(r["state"], r["name"], r["isign"]) for r in rec] == [(k,) + x for k in range(sl.size) for x in old + new]
    assert got.pair_iv.shape == (No, ct.LMATS + 1) and got.pair_tau.shape == (No, ct.LTAU + 1)
    assert got.exc_w.shape == (No, No, ct.LREAL) and got.exc_tau.dtype == np.float64
    for a in range(No):
        assert not np.any(got.exc_iv[a, a]) and not np.any(got.exc_tau[a, a]) and not np.any(got.exc_w[a, a])
    for a, b in chi.exc_pairs(cfg):
        assert np.max(np.abs(got.exc_tau[a, b] - got.exc_tau[b, a][::-1])) <= 1e-12 * np.max(np.abs(got.exc_tau[a, b]))
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5
    # pair and exc left off: the fields of before, bit for bit, and no new one
    plain = chi.build_chi(cfg, sl, copt)
    assert all(np.array_equal(a, b) for a, b in zip(_old_fields(plain), _old_fields(got)))
    assert plain.pair_iv is None and plain.pair_tau is None and plain.exc_iv is None and plain.exc_w is None
    # each new part alone, without the old ones
    p_only = chi.build_chi(cfg, sl, copt, spin=False, dens=False, pair=True)
    e_only = chi.build_chi(cfg, sl, copt, spin=False, dens=False, exc=True)
    assert p_only.spin_iv is None and p_only.dens_w is None and p_only.exc_iv is None and e_only.pair_iv is None
    for a, b in ((p_only.pair_iv, got.pair_iv), (p_only.pair_tau, got.pair_tau), (p_only.pair_w, got.pair_w),
                 (e_only.exc_iv, got.exc_iv), (e_only.exc_tau, got.exc_tau), (e_only.exc_w, got.exc_w)):
        assert np.array_equal(a, b)


def test_build_chi_pair_thermal_list_with_twin_vectors():
    T, copt = pt.truth("C1"), pt.options("C1")
    opt = DiagOptions(lanc_nstates_total=ct.NTOTAL, beta=ct.BETA, cutoff=ct.CUTOFF, ed_twin=True)
    _, sl = ed_diag(T.cfg, opt)
    sl2, _ = post_diag(sl, opt, T.cfg)
    kept = T.thermal_states()
    assert sl2.size == len(kept) and sum(p is not None for p in sl2.twin_of) >= 1
    got = chi.build_chi(T.cfg, sl2, copt, pair=True, exc=True)
    d = pt.distances(T.pair_exc_thermal(copt), got, 1)
    print(f"thermal C1: {sl2.size} states, {sum(p is not None for p in sl2.twin_of)} twin entries: iv {d[0]:.2e}, "
          f"tau {d[1]:.2e}, w {d[2]:.2e}")
    assert got.exc_iv.shape == (1, 1, ct.LMATS + 1) and not np.any(got.exc_iv)      # Norb = 1: no exc seed
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5


def test_seed_buffer_chunking_gives_the_same_arrays(monkeypatch):
    """SEED_BUFFER_BYTES below one seed: every call is split into one-seed calls and one-row Lanczos
    batches.  The seeds are the same bits; a batch of one may take another recurrence kernel than a batch
    of two, so the arrays are held to the bars of the truth test against each other."""
    T, copt, sl = pt.truth("C2"), pt.options("C2"), states("C2")
    rec_w, rec_s = [], []
    whole = chi.build_chi(T.cfg, sl, copt, spin=False, dens=False, pair=True, exc=True, record=rec_w)
    monkeypatch.setattr(gf, "SEED_BUFFER_BYTES", 1)           # the one knob: gf.seed_fractions reads it
    split = chi.build_chi(T.cfg, sl, copt, spin=False, dens=False, pair=True, exc=True, record=rec_s)
    assert [(r["state"], r["name"], r["isign"], r["norm2"]) for r in rec_w] == \
        [(r["state"], r["name"], r["isign"], r["norm2"]) for r in rec_s]
    worst = {}
    for f, bar in (("pair_iv", 1e-10), ("pair_tau", 1e-10), ("pair_w", 1e-5), ("exc_iv", 1e-10), ("exc_tau", 1e-10), ("exc_w", 1e-5)):
        a, b = getattr(whole, f), getattr(split, f)
        worst[f] = np.max(np.abs(a - b)) / np.max(np.abs(a))
        assert worst[f] < bar, (f, worst[f])
    print("whole against split: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
