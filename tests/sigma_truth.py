"""Dense truths of the self-energy tests (test infrastructure only).

Nothing here shares code with the bath functions under test (csrc/
ed_sigma_host.hpp): no pole table, no Delta formula.

One-particle truth.  The one-body matrix of a config is read off the full-Fock
Jordan-Wigner Hamiltonian of oracle.jw_dense with the interactions set to zero,
  h[i, j] = H[1 << i, 1 << j] - H[0, 0] delta_ij,
and G0(z) = [(z - h)^-1] on the impurity levels.

superc.  With Psi = (c_{i,up}, c+_{i,dw}) over all Ns levels the vacuum is "no
up level, every down level filled"; the states psi+_i |vac> are built with the
Jordan-Wigner matrices themselves (their signs are the true ones) and
  h_BdG = B+ H B - E_vac
on their span.  The Nambu block of orbital a is [(z - h_BdG)^-1] on the indices
(a, Ns + a).

Interacting truth.  Sigma = G0_truth^-1 - G_Lehmann^-1 with the Lehmann sums of
orbmix_truth (H2), superc_truth (S1) and `Lehmann1` below (N1, a single-orbital
normal model), block by block with numpy.linalg.inv.

Everything is computed once per model and shared (never modified) by the CPU
and GPU tests.
"""
import copy
from functools import lru_cache

import numpy as np

BETA, EPS, WINI, WFIN = 50.0, 0.05, -5.0, 5.0     # the grids of the U = 0 checks


def noninteracting(cfg):
    c = copy.deepcopy(cfg)
    c.Uloc, c.Ust, c.Jh, c.Jx, c.Jp = (0.0, 0.0, 0.0), 0.0, 0.0, 0.0, 0.0
    return c


def u0_config(name):
    """The models of the U = 0 identity: five normal / nonsu2 ones and two superc."""
    import cases
    from edgpu.params import EDConfig, init_dmft_bath, make_config

    if name == "normal_diag":       # normal bath, diagonal impHloc
        cfg = make_config(Norb=2, Nbath=3, Nspin=2, xmu=0.2, bath="random", seed=7)
        cfg.impHloc = cases._hloc(2, 2, 1, offdiag=False)
    elif name == "hybrid":
        cfg = cases.hybrid()
    elif name == "replica_real":    # real impHloc, real replica blocks
        cfg = EDConfig(Norb=2, Nbath=2, Nspin=1, bath_type="replica", xmu=0.1)
        cfg.impHloc = cases._hloc(1, 2, 8)
        b = init_dmft_bath(cfg)
        rng = np.random.default_rng(9)
        for k in range(cfg.Nbath):
            a = rng.normal(size=(2, 2))
            b.h[0, 0, :, :, k] = 0.5 * (a + a.T)
            b.vr[k] = 0.4 + 0.1 * (k + 1)
        cfg.bath = b
    elif name == "nonsu2_normal":   # Norb = 1, real spin-flip impHloc
        cfg = make_config(Norb=1, Nbath=3, Nspin=2, ed_mode="nonsu2", xmu=0.15, ed_vsf_ratio=0.4, bath="random",
                          seed=23)
        cfg.impHloc = cases._hloc(2, 1, 12, spinflip=True)
    elif name == "nonsu2_replica":  # Norb = 1, real replica blocks with a spin flip
        cfg = EDConfig(Norb=1, Nbath=2, Nspin=2, ed_mode="nonsu2", bath_type="replica")
        cfg.impHloc = cases._hloc(2, 1, 12, spinflip=True)
        b = init_dmft_bath(cfg)
        rng = np.random.default_rng(14)
        for k in range(cfg.Nbath):
            a = rng.normal(size=(2, 2))
            b.h[:, :, 0, 0, k] = 0.5 * (a + a.T)
            b.vr[k] = 0.3 + 0.05 * k
        cfg.bath = b
    elif name == "superc_1":
        cfg = make_config(Norb=1, Nbath=2, ed_mode="superc", deltasc=0.3, bath="random", xmu=0.2, seed=8)
    elif name == "superc_2":
        cfg = make_config(Norb=2, Nbath=1, ed_mode="superc", deltasc=0.3, bath="random", xmu=0.1, seed=19)
        cfg.impHloc = cases._hloc(1, 2, 20, offdiag=False)
    else:
        raise KeyError(name)
    cfg = noninteracting(cfg)
    cfg.check()
    return cfg


U0_MODELS = ["normal_diag", "hybrid", "replica_real", "nonsu2_normal", "nonsu2_replica"]
U0_SUPERC = ["superc_1", "superc_2"]
# one sector per model for the device pipeline: it and every sector its seeds
# reach have at most 924 rows; at U = 0 the G of any eigenstate is G0
U0_SECTOR = {"normal_diag": (2, 1), "hybrid": (3, 3), "replica_real": (3, 3), "nonsu2_normal": (4, 0),
             "nonsu2_replica": (3, 0), "superc_1": (0, 0), "superc_2": (0, 0)}


def one_body(cfg):
    """h (2Ns x 2Ns) of the quadratic part of H."""
    from oracle.jw_dense import full_hamiltonian

    H = full_hamiltonian(noninteracting(cfg)).tocsr()
    n = 2 * cfg.Ns
    h = np.zeros((n, n), dtype=np.complex128)
    e0 = H[0, 0]
    for i in range(n):
        for j in range(n):
            h[i, j] = H[1 << i, 1 << j] - (e0 if i == j else 0.0)
    assert np.max(np.abs(h - h.conj().T)) < 1e-14
    return h


def imp_levels(cfg):
    """The level of layout index s * Norb + o."""
    return [o + s * cfg.Ns for s in range(cfg.Nspin) for o in range(cfg.Norb)]


def h_bdg(cfg):
    """(h_BdG, residual of the invariant subspace) of a superc config."""
    from oracle.jw_dense import _ops, full_hamiltonian

    Ns = cfg.Ns
    H = full_hamiltonian(noninteracting(cfg)).tocsr()
    c = [m.tocsr() for m in _ops(2 * Ns)]
    vac = np.zeros(H.shape[0], dtype=np.complex128)
    vac[((1 << Ns) - 1) << Ns] = 1.0
    cols = [np.asarray(c[i].getH() @ vac).ravel() for i in range(Ns)] + [np.asarray(c[Ns + i] @ vac).ravel()
                                                                         for i in range(Ns)]
    B = np.array(cols).T
    assert np.allclose(B.conj().T @ B, np.eye(2 * Ns))
    HB = H @ B
    evac = np.vdot(vac, H @ vac)
    M = B.conj().T @ HB
    resid = np.max(np.abs(HB - B @ M))
    return M - evac * np.eye(2 * Ns), resid


class Dense:
    """G0 of one config on given points: `g0` (Nspin, Nspin, Norb, Norb, L)
    (superc: g0 and f0 (1, 1, Norb, Norb, L), entries (a, a) only, and `nambu`
    (Norb, 2, 2, L)); `bar` (L,) = kappa_2(z - h) max|(z - h)^-1| per point,
    the factor of the G0 bar 1e-13 kappa_2(z - h) max|G0|."""

    def __init__(self, cfg, z):
        self.cfg = cfg
        z = np.asarray(z, dtype=np.complex128)
        No, Nsp = cfg.Norb, cfg.Nspin
        superc = cfg.ed_mode == "superc"
        h = h_bdg(cfg)[0] if superc else one_body(cfg)
        n = h.shape[0]
        R = np.linalg.inv(z[:, None, None] * np.eye(n)[None] - h[None])            # (L, n, n)
        self.bar = np.linalg.cond(z[:, None, None] * np.eye(n)[None] - h[None], 2) * np.max(np.abs(R), axis=(1, 2))
        self.g0 = np.zeros((Nsp, Nsp, No, No, len(z)), dtype=np.complex128)
        if superc:
            self.f0 = np.zeros_like(self.g0)
            self.nambu = np.zeros((No, 2, 2, len(z)), dtype=np.complex128)
            for a in range(No):
                ix = [a, cfg.Ns + a]
                self.nambu[a] = np.moveaxis(R[:, ix][:, :, ix], 0, -1)
                self.g0[0, 0, a, a] = self.nambu[a, 0, 0]
                self.f0[0, 0, a, a] = self.nambu[a, 0, 1]
        else:
            lev = imp_levels(cfg)
            full = np.moveaxis(R[:, lev][:, :, lev], 0, -1)                        # (nso, nso, L)
            for i in range(Nsp * No):
                for j in range(Nsp * No):
                    self.g0[i // No, j // No, i % No, j % No] = full[i, j]


def block_indices(cfg):
    """The blocks as lists of layout indices s * Norb + o (the table of DESIGN
    section 14, restated); superc: one list [a] per orbital."""
    No, Nsp = cfg.Norb, cfg.Nspin
    if cfg.ed_mode == "superc":
        return [[a] for a in range(No)]
    if cfg.ed_mode == "normal":
        if cfg.bath_type == "normal":
            return [[s * No + o] for s in range(Nsp) for o in range(No)]
        return [[s * No + o for o in range(No)] for s in range(Nsp)]
    if cfg.bath_type == "normal":
        return [[o, No + o] for o in range(No)]
    return [list(range(2 * No))]


def gather(A, idx, No):
    """The (n, n, L) block of a (Nspin, Nspin, Norb, Norb, L) array."""
    return np.array([[A[i // No, j // No, i % No, j % No] for j in idx] for i in idx])


def scatter(cfg, blocks, mats, L):
    out = np.zeros((cfg.Nspin, cfg.Nspin, cfg.Norb, cfg.Norb, L), dtype=np.complex128)
    No = cfg.Norb
    for idx, M in zip(blocks, mats):
        for a, i in enumerate(idx):
            for b, j in enumerate(idx):
                out[i // No, j // No, i % No, j % No] = M[a, b]
    return out


def inv_pointwise(M):
    """numpy.linalg.inv of an (n, n, L) array at every point."""
    return np.moveaxis(np.linalg.inv(np.moveaxis(M, -1, 0)), 0, -1)


def nambu_of(G, F, a, real_axis):
    """[[G, F], [F, -conj(G)]] of orbital a, (2, 2, L); the last entry at the
    mirrored index on the real axis."""
    g, f = G[0, 0, a, a], F[0, 0, a, a]
    gb = -np.conj(g[::-1] if real_axis else g)
    return np.array([[g, f], [f, gb]])


def sigma_from(cfg, G0, G, F0=None, F=None, real_axis=False):
    """numpy Sigma = G0^-1 - G^-1 block by block.  Returns (S, SA, norm2) with
    norm2 (nblocks, L) the 2-norm of every block's G0^-1 per point."""
    No = cfg.Norb
    L = G.shape[-1]
    blocks = block_indices(cfg)
    S, SA, norms = [], [], []
    for idx in blocks:
        if cfg.ed_mode == "superc":
            a = idx[0]
            i0 = inv_pointwise(nambu_of(G0, F0, a, real_axis))
            s = i0 - inv_pointwise(nambu_of(G, F, a, real_axis))
            S.append(s[:1, :1])
            SA.append(s[:1, 1:])
        else:
            i0 = inv_pointwise(gather(G0, idx, No))
            S.append(i0 - inv_pointwise(gather(G, idx, No)))
        norms.append(np.linalg.norm(np.moveaxis(i0, -1, 0), 2, axis=(1, 2)))
    out = scatter(cfg, blocks, S, L)
    outa = scatter(cfg, blocks, SA, L) if SA else None
    return out, outa, np.array(norms)


# ------------------------------------------------------------ interacting N1
def n1_config():
    from edgpu.params import make_config

    return make_config(Norb=1, Nbath=3, Nspin=1, Uloc=(2.0, 0.0, 0.0), xmu=0.3, bath="random", seed=41)


class Lehmann1:
    """G_aa of a small normal-mode model by the direct Lehmann sum over the
    whole Fock space (dense eigh of the full Hamiltonian), T = 0 with equal
    weights on the ground-state set {E - E0 < 1e-9}."""

    def __init__(self, cfg):
        from oracle.jw_dense import _ops, full_hamiltonian

        self.cfg = cfg
        H = full_hamiltonian(cfg).toarray()
        assert np.max(np.abs(H - H.conj().T)) < 1e-14
        self.w, self.v = np.linalg.eigh(H)
        self.c = [m.toarray() for m in _ops(2 * cfg.Ns)]

    def gf(self, z):
        cfg = self.cfg
        No, Nsp, Ns = cfg.Norb, cfg.Nspin, cfg.Ns
        z = np.asarray(z, dtype=np.complex128)
        G = np.zeros((Nsp, Nsp, No, No, len(z)), dtype=np.complex128)
        gs = [k for k, e in enumerate(self.w) if e - self.w[0] < 1e-9]
        for k in gs:
            de = self.w - self.w[k]
            for s in range(Nsp):
                for a in range(No):
                    c = self.c[a + s * Ns]
                    p = np.abs(self.v.conj().T @ (c.conj().T @ self.v[:, k])) ** 2
                    h = np.abs(self.v.conj().T @ (c @ self.v[:, k])) ** 2
                    G[s, s, a, a] += (np.sum(p[None, :] / (z[:, None] - de[None, :]), axis=1)
                                      + np.sum(h[None, :] / (z[:, None] + de[None, :]), axis=1)) / len(gs)
        return G


@lru_cache(maxsize=None)
def lehmann1():
    return Lehmann1(n1_config())


# ------------------------------------------------- random blocks against numpy
# Every block size on one (Nspin, Nspin, Norb, Norb) = (2, 2, 3, 3) layout (the
# Nambu case on (1, 1, 3, 3)); the indices left out must stay exactly zero.
LM, LR = 67, 65        # a partial last wave; an odd real grid: the mirror has a centre point
CASE_LAYOUT = (2, 3)
CASE_IDX = {1: [[0], [4]], 2: [[0, 3], [5, 2]], 3: [[0, 1, 2]], 4: [[3, 0, 4, 1]], 6: [[0, 1, 2, 3, 4, 5]]}
CASE_POLES = (1, 7, 64)
# (N, poles, Nambu): every block size at every pole count, and the Nambu form of n = 2
CASES = [(N, p, False) for N in CASE_IDX for p in CASE_POLES] + [(2, p, True) for p in CASE_POLES]


def _herm(rng, n, real=False):
    a = rng.normal(size=(n, n)) + (0 if real else 1j * rng.normal(size=(n, n)))
    return 0.5 * (a + a.conj().T)


def case_grids():
    from edgpu.gf import matsubara, realaxis

    return 1j * matsubara(BETA, LM), realaxis(WINI, WFIN, LR) + 1j * EPS


@lru_cache(maxsize=None)
def random_case(N, npole, nambu=False):
    """Blocks (edgpu.sigma.Block) with random Hermitian h and random poles, and
    a physical G: the block's corner of [(z - A)^-1] for a random Hermitian A
    of twice its size (Nambu: A real, of the Bogoliubov-de Gennes form
    [[a, b], [b, -a]], G and F its (particle, particle) and (particle, hole)
    entries, so that [[G, F], [F, -conj(G(-w))]] is its resolvent)."""
    from edgpu.sigma import Block

    rng = np.random.default_rng(1000 * N + npole + (500 if nambu else 0))
    nspin, norb = (1, 3) if nambu else CASE_LAYOUT
    lists = [[0, 0], [2, 2]] if nambu else CASE_IDX[N]
    zs = case_grids()
    G = [np.zeros((nspin, nspin, norb, norb, len(z)), dtype=np.complex128) for z in zs]
    F = [np.zeros_like(g) for g in G] if nambu else None
    blocks = []
    for idx in lists:
        n = len(idx)
        if nambu:
            x = rng.normal()
            h = np.diag([x, -x])                 # diag(h - mu, -(h - mu))
        else:
            h = 0.4 * _herm(rng, n)
        e = rng.uniform(-2.0, 2.0, size=npole)
        w = (rng.normal(size=(npole, n)) + (0 if nambu else 1j * rng.normal(size=(npole, n)))) / np.sqrt(npole)
        blocks.append(Block(np.array(idx), nambu, h.astype(np.complex128), e, np.ones(npole, dtype=np.complex128), w))
        if nambu:
            m = 3
            a, b = _herm(rng, m, True), _herm(rng, m, True)
            A = np.block([[a, b], [b, -a]])
            for g, f, z in zip(G, F, zs):
                R = np.linalg.inv(z[:, None, None] * np.eye(2 * m)[None] - A[None])
                g[0, 0, idx[0], idx[0]] = R[:, 0, 0]
                f[0, 0, idx[0], idx[0]] = R[:, 0, m]
        else:
            A = _herm(rng, 2 * n)
            for g, z in zip(G, zs):
                R = np.linalg.inv(z[:, None, None] * np.eye(2 * n)[None] - A[None])
                for ia, i in enumerate(idx):
                    for ja, j in enumerate(idx):
                        g[i // norb, j // norb, i % norb, j % norb] = R[:, ia, ja]
    return dict(blocks=blocks, nspin=nspin, norb=norb, G=G, F=F, nambu=nambu)


def numpy_case(case):
    """Sigma, G0, Delta (and Sigma_A, F0) of a random case with numpy.linalg.inv,
    and per axis the bars, (nblocks, L):
      s:  1e-12 (|invG0|_max + kappa_2(G) |G^-1|_max)    the forward error of pivoted elimination, n <= 6
      g0: 1e-12 kappa_2(invG0) |G0|_max                   the same for the one inverse
      d:  1e-13 sum_p |term_p|_max                        the pole sum's additions."""
    nspin, norb, nambu = case["nspin"], case["norb"], case["nambu"]
    out = {k: [None, None] for k in ("s", "g0", "d", "sa", "f0")}
    bars = {k: [None, None] for k in ("s", "g0", "d")}
    for ax, z in enumerate(case_grids()):
        L = len(z)
        arr = {k: np.zeros((nspin, nspin, norb, norb, L), dtype=np.complex128) for k in out}
        bs, bg, bd = [], [], []
        for B in case["blocks"]:
            n = len(B.idx)
            terms = B.c[:, None, None, None] * B.w[:, :, None, None] * np.conj(B.w)[:, None, :, None] / (
                z[None, None, None, :] - B.e[:, None, None, None])
            D = terms.sum(axis=0)
            i0 = z[None, None, :] * np.eye(n)[:, :, None] - B.h[:, :, None] - D
            g0 = inv_pointwise(i0)
            Gb = nambu_of(case["G"][ax], case["F"][ax], B.idx[0], ax == 1) if nambu else gather(case["G"][ax], B.idx,
                                                                                                norb)
            gi = inv_pointwise(Gb)
            S = i0 - gi
            mx = lambda M: np.max(np.abs(M), axis=(0, 1))                       # noqa: E731
            cond = lambda M: np.linalg.cond(np.moveaxis(M, -1, 0), 2)           # noqa: E731
            bs.append(1e-12 * (mx(i0) + cond(Gb) * mx(gi)))
            bg.append(1e-12 * cond(i0) * mx(g0))
            bd.append(1e-13 * np.max(np.abs(terms).sum(axis=0), axis=(0, 1)))
            if nambu:
                a = B.idx[0]
                arr["s"][0, 0, a, a], arr["sa"][0, 0, a, a] = S[0, 0], S[0, 1]
                arr["g0"][0, 0, a, a], arr["f0"][0, 0, a, a] = g0[0, 0], g0[0, 1]
                arr["d"][0, 0, a, a] = D[0, 0]
            else:
                for ia, i in enumerate(B.idx):
                    for ja, j in enumerate(B.idx):
                        at = (i // norb, j // norb, i % norb, j % norb)
                        arr["s"][at], arr["g0"][at], arr["d"][at] = S[ia, ja], g0[ia, ja], D[ia, ja]
        for k in out:
            out[k][ax] = arr[k]
        bars["s"][ax], bars["g0"][ax], bars["d"][ax] = np.array(bs), np.array(bg), np.array(bd)
    return out, bars


def case_errors(case, got, ref, bars):
    """Largest ratio |got - ref| / bar per key over blocks, axes and points, and
    whether every entry outside the blocks is exactly zero."""
    norb, nambu = case["norb"], case["nambu"]
    worst = {"s": 0.0, "g0": 0.0, "d": 0.0}
    zeros = True
    for ax in range(2):
        mask = np.zeros(got["g0"][ax].shape[:4], dtype=bool)
        for b, B in enumerate(case["blocks"]):
            for i in (B.idx[:1] if nambu else B.idx):
                for j in (B.idx[:1] if nambu else B.idx):
                    mask[i // norb, j // norb, i % norb, j % norb] = True
            for k, extra in (("s", "sa"), ("g0", "f0"), ("d", None)):
                if nambu:
                    a = B.idx[0]
                    e = np.abs(got[k][ax][0, 0, a, a] - ref[k][ax][0, 0, a, a])
                    if extra:
                        e = np.maximum(e, np.abs(got[extra][ax][0, 0, a, a] - ref[extra][ax][0, 0, a, a]))
                else:
                    e = np.max(np.abs(gather(got[k][ax], B.idx, norb) - gather(ref[k][ax], B.idx, norb)), axis=(0, 1))
                worst[k] = max(worst[k], float(np.max(e / bars[k][ax][b])))
        for k in ("s", "g0", "d") + (("sa", "f0") if nambu else ()):
            zeros = zeros and not np.any(got[k][ax][~mask])
    return worst, zeros


# ------------------------------------------------------------ U = 0 identity
def u0_ratio(cfg, G, F, out, zs, scale=1e-10):
    """max over blocks and points of |Sigma| (and |Sigma_A|) / (scale max(|G|, |F|) |G0^-1|_2^2)."""
    worst = 0.0
    for ax, z in enumerate(zs):
        D = Dense(cfg, z)
        _, _, norms = sigma_from(cfg, D.g0, D.g0, getattr(D, "f0", None), getattr(D, "f0", None), ax == 1)
        gmax = max(np.max(np.abs(G[ax])), np.max(np.abs(F[ax])) if F is not None else 0.0)
        for b, idx in enumerate(block_indices(cfg)):
            if cfg.ed_mode == "superc":
                a = idx[0]
                e = np.maximum(np.abs(out["s"][ax][0, 0, a, a]), np.abs(out["sa"][ax][0, 0, a, a]))
            else:
                e = np.max(np.abs(gather(out["s"][ax], idx, cfg.Norb)), axis=(0, 1))
            worst = max(worst, float(np.max(e / (scale * gmax * norms[b] ** 2))))
    return worst


# ------------------------------------------------------- interacting models
INTERACTING = ["H2", "S1", "N1"]


def interacting_config(name):
    """(cfg, eps): orbmix_truth H2 (real impHloc), superc_truth S1, and N1."""
    import orbmix_truth as ot
    import superc_truth as st

    if name == "H2":
        return ot.truth("H2").cfg, ot.EPS["H2"]
    if name == "S1":
        return st.truth("S1").cfg, st.EPS["S1"]
    assert name == "N1"
    return n1_config(), EPS


def interacting_truth(name, states, wm, wr, eps):
    """((Gm, Gr), (Fm, Fr) or None) of the dense Lehmann sums, in the layout
    (Nspin, Nspin, Norb, Norb, L); S1 sums over the list under test (its
    ground state may be degenerate)."""
    import orbmix_truth as ot
    import superc_truth as st

    cfg, _ = interacting_config(name)
    No, Nsp = cfg.Norb, cfg.Nspin
    if name == "N1":
        T = lehmann1()
        return (T.gf(1j * np.asarray(wm)), T.gf(np.asarray(wr) + 1j * eps)), None
    if name == "H2":
        out = []
        for g in ot.truth("H2").gf(wm, wr, eps):
            G = np.zeros((Nsp, Nsp, No, No, g.shape[-1]), dtype=np.complex128)
            for s in range(Nsp):
                G[s, s] = g[s]
            out.append(G)
        return tuple(out), None
    tr = st.truth("S1").gf_of_list(states, wm, wr, eps)
    G, F = [], []
    for ax in range(2):
        g = np.zeros((1, 1, No, No, tr["G"][ax].shape[-1]), dtype=np.complex128)
        f = np.zeros_like(g)
        for a in range(No):
            g[0, 0, a, a], f[0, 0, a, a] = tr["G"][ax][a], tr["F"][ax][a]
        G.append(g)
        F.append(f)
    return tuple(G), tuple(F)


def interacting_ratios(cfg, Gt, Ft, S, SA, zs):
    """Per axis: max over blocks and points of |Sigma - Sigma_truth| (and the
    anomalous part) / (scale max(|G|, |F|) |G0(z)^-1|_2^2), scale 1e-10 on the
    Matsubara axis and 1e-5 on the real axis (G's own bars carried through the
    inverse); and max Im Sigma_aa(i w_n) over the diagonal."""
    out = []
    for ax, (z, scale) in enumerate(zip(zs, (1e-10, 1e-5))):
        D = Dense(cfg, z)
        St, SAt, norms = sigma_from(cfg, D.g0, Gt[ax], getattr(D, "f0", None), Ft[ax] if Ft else None, ax == 1)
        gmax = max(np.max(np.abs(Gt[ax])), np.max(np.abs(Ft[ax])) if Ft else 0.0)
        worst = 0.0
        for b, idx in enumerate(block_indices(cfg)):
            if cfg.ed_mode == "superc":
                a = idx[0]
                e = np.maximum(np.abs(S[ax][0, 0, a, a] - St[0, 0, a, a]), np.abs(SA[ax][0, 0, a, a] - SAt[0, 0, a, a]))
            else:
                e = np.max(np.abs(gather(S[ax], idx, cfg.Norb) - gather(St, idx, cfg.Norb)), axis=(0, 1))
            worst = max(worst, float(np.max(e / (scale * gmax * norms[b] ** 2))))
        out.append(worst)
    No = cfg.Norb
    im = max(float(np.max(S[0][s, s, a, a].imag)) for s in range(cfg.Nspin) for a in range(No))
    return out[0], out[1], im, float(np.max(np.abs(St)))
