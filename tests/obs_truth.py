"""Truth functions of the observables tests (test infrastructure only).

Two independent restatements of <v|T|v> for an operator string T (a list of
(level, op), op 1 = c^+, 0 = c, applied right to left):

  * dense_expect: the full-Fock Jordan-Wigner matrices of oracle.jw_dense._ops
    multiplied in string order and restricted to the sector's states — no
    popcount sign logic at all (tiny systems only);
  * numpy_expect / numpy_moments: a vectorised walk over the sector map that
    applies the operators one after the other, each with its own sign, and
    finds the target rows by searchsorted.  It serves as the `evaluator` of
    edgpu.observables on the CPU and as the host route the device calls are
    timed against.
"""
import numpy as np

from oracle.jw_dense import _ops

_OPS = {}


def fock_ops(nlev):
    if nlev not in _OPS:
        _OPS[nlev] = _ops(nlev)
    return _OPS[nlev]


def dense_term(nlev, term):
    c = fock_ops(nlev)
    m = None
    for lev, op in term:
        f = c[lev].getH() if op else c[lev]
        m = f if m is None else m @ f
    return m.tocsr()


def dense_restricted(nlev, hmap, term):
    idx = np.asarray(hmap, dtype=np.int64)
    return dense_term(nlev, term)[idx][:, idx]


def dense_expect(nlev, hmap, vec, term):
    return complex(np.vdot(vec, dense_restricted(nlev, hmap, term) @ vec))


def dense_conserves(cfg, term):
    """[T, Q] = 0 for the quantum numbers of cfg's sectors, as full-Fock
    matrices (T must not vanish identically)."""
    import scipy.sparse as sp

    from edgpu.sectors import LZDIAG

    Ns = cfg.Ns
    nlev = 2 * Ns
    T = dense_term(nlev, term)
    assert T.nnz > 0
    occ = (np.arange(1 << nlev)[:, None] >> np.arange(nlev)) & 1
    nup, ndw = occ[:, :Ns].sum(1), occ[:, Ns:].sum(1)
    if cfg.ed_mode == "normal":
        qs = [nup, ndw]
    elif cfg.ed_mode == "superc":
        qs = [nup - ndw]
    else:
        qs = [nup + ndw]
        if cfg.Jz_basis:
            wgt = np.array([2 * LZDIAG[(l % Ns) % cfg.Norb] + (1 if l < Ns else -1) for l in range(nlev)])
            qs.append(occ @ wgt)
    for q in qs:
        Q = sp.diags(q.astype(np.float64))
        if abs(Q @ T - T @ Q).max() != 0:
            return False
    return True


def _parity(x):
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> s
    return x & 1


def apply_string(states, term):
    """(alive, target state, sign) per source state, operator by operator."""
    st = np.asarray(states, dtype=np.int64).copy()
    sign = np.ones(len(st))
    alive = np.ones(len(st), dtype=bool)
    for lev, op in reversed(list(term)):
        occ = (st >> lev) & 1
        alive &= occ == (0 if op else 1)
        sign *= 1.0 - 2.0 * _parity(st & ((1 << lev) - 1))
        st ^= 1 << lev
    return alive, st, sign


def numpy_expect(hmap, vec, term):
    hmap = np.asarray(hmap, dtype=np.int64)
    alive, tg, sg = apply_string(hmap, term)
    i = np.nonzero(alive)[0]
    j = np.searchsorted(hmap, tg[i])
    assert np.array_equal(hmap[j], tg[i]), "string leaves the sector"
    return complex(np.sum(np.conj(vec[j]) * sg[i] * vec[i]))


def numpy_moments(hmap, vec, levels):
    w = np.abs(vec) ** 2
    bits = ((np.asarray(hmap, dtype=np.int64)[:, None] >> np.asarray(levels)) & 1).astype(np.float64)
    return bits.T @ (bits * w[:, None]), float(w.sum())


def numpy_evaluator(map_of):
    """An `evaluator` for edgpu.observables; map_of(cfg, sec) -> sector map."""
    def ev(cfg, sec, vec, levels, terms):
        hmap = map_of(cfg, sec)
        v = np.asarray(vec)
        M, norm = numpy_moments(hmap, v, levels)
        return M, norm, np.array([numpy_expect(hmap, v, t) for t in terms], dtype=np.complex128)
    return ev


def oracle_map(cfg, sec):
    from oracle.oracle import Oracle

    return Oracle(cfg).build_sector(sec.q1, sec.q2)


# ------------------------------------------------------------------ strings
CDG, C = 1, 0


def imp_levels(cfg):
    return [a + s * cfg.Ns for s in (0, 1) for a in range(cfg.Norb)]


def hop_terms(cfg):
    lv = imp_levels(cfg)
    return [[(p, CDG), (q, C)] for p in lv for q in lv if p != q]


def exchange_terms(cfg):
    """The Dse and Dph strings (ED_OBSERVABLES.f90:882-927), reference order."""
    Ns, out = cfg.Ns, []
    for a in range(cfg.Norb):
        for b in range(cfg.Norb):
            if a != b:
                out.append([(a, CDG), (b + Ns, CDG), (a + Ns, C), (b, C)])
                out.append([(a, CDG), (a + Ns, CDG), (b + Ns, C), (b, C)])
    return out


def number_terms(cfg):
    lv = imp_levels(cfg)
    out = [[(p, CDG), (p, C)] for p in lv] + [[(p, C), (p, CDG)] for p in lv]
    p, q = lv[0], lv[-1]
    out.append([(p, CDG), (p, C), (q, CDG), (q, C)])       # n_p n_q
    out.append([(p, CDG), (q, C), (q, CDG), (p, C)])       # c+_p (1 - n_q) c_p = n_p (1 - n_q)
    out.append([(p, CDG), (p, CDG), (p, C), (p, C)])       # vanishes identically
    return out


def pair_terms(cfg):
    return [[(a, C), (a + cfg.Ns, C)] for a in range(cfg.Norb)]


def random_state(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0.0)
    return v / np.linalg.norm(v)


# ------------------------------------------------- dense ground multiplet
def dense_ground_states(cfg, tol=1e-9):
    """StateList of the degenerate ground multiplet from the dense eigh of
    oracle.jw_dense.sector_matrix over every sector ed_diag visits."""
    from edgpu.diag import StateList
    from edgpu.sectors import diag_sectors
    from oracle.jw_dense import full_hamiltonian

    H = full_hamiltonian(cfg)
    found = []
    for sec in diag_sectors(cfg):
        idx = oracle_map(cfg, sec).astype(np.int64)
        w, v = np.linalg.eigh(H[idx][:, idx].toarray())
        found += [(w[k], sec.isector, v[:, k]) for k in range(len(w))]
    e0 = min(f[0] for f in found)
    keep = [f for f in found if f[0] - e0 <= tol]
    return StateList([float(f[0]) for f in keep], [f[1] for f in keep], [f[2] for f in keep])


def embed(cfg, states):
    """The kept vectors in the full Fock space of 2*Ns levels."""
    from edgpu.sectors import setup_pointers

    secs = setup_pointers(cfg)
    out = []
    for isec, v in zip(states.sectors, states.vectors):
        full = np.zeros(1 << (2 * cfg.Ns), dtype=np.complex128)
        full[oracle_map(cfg, secs[isec - 1]).astype(np.int64)] = v
        out.append(full)
    return out


def dense_observables(cfg, states):
    """observables_impurity and local_energy_impurity from full-Fock operator
    matrices, the seed-norm quantities by the reference's own route
    (ED_OBSERVABLES.f90:166-337: 0.5*(|seed|^2 - ...))."""
    Ns, No, Nsp = cfg.Ns, cfg.Norb, cfg.Nspin
    S = Nsp - 1
    c = fock_ops(2 * Ns)
    cd = [m.getH() for m in c]
    n = [cd[p] @ c[p] for p in range(2 * Ns)]
    psis = embed(cfg, states)
    wgt = 1.0 / len(psis)

    def ev(O):
        return wgt * sum(np.vdot(p, O @ p) for p in psis)

    def norm2(O):
        return wgt * sum(np.vdot(O @ p, O @ p).real for p in psis)

    up = [n[a] for a in range(No)]
    dw = [n[a + Ns] for a in range(No)]
    o = {}
    o["dens_up"] = np.array([ev(up[a]).real for a in range(No)])
    o["dens_dw"] = np.array([ev(dw[a]).real for a in range(No)])
    o["dens"] = o["dens_up"] + o["dens_dw"]
    o["docc"] = np.array([ev(up[a] @ dw[a]).real for a in range(No)])
    o["magz"] = o["dens_up"] - o["dens_dw"]
    sz = [0.5 * (up[a] - dw[a]) for a in range(No)]
    nt = [up[a] + dw[a] for a in range(No)]
    o["sz2"] = np.array([[ev(sz[a] @ sz[b]).real for b in range(No)] for a in range(No)])
    o["n2"] = np.array([[ev(nt[a] @ nt[b]).real for b in range(No)] for a in range(No)])
    o["s2tot"] = ev(sum(sz) @ sum(sz)).real
    o["magx"], o["magy"], o["phisc"] = np.zeros(No), np.zeros(No), np.zeros(No)
    for a in range(No):
        if cfg.ed_mode == "nonsu2":
            o["magx"][a] = 0.5 * (norm2(c[a] + c[a + Ns]) - o["dens_up"][a] - o["dens_dw"][a])
            o["magy"][a] = 0.5 * (norm2(1j * c[a] + c[a + Ns]) - o["dens_up"][a] - o["dens_dw"][a])
        if cfg.ed_mode == "superc":
            o["phisc"][a] = 0.5 * (norm2(cd[a] + c[a + Ns]) - o["dens_up"][a] - (1.0 - o["dens_dw"][a]))
    dm = np.zeros((Nsp, Nsp, No, No), dtype=np.complex128)
    for i in range(Nsp):
        for j in range(Nsp):
            for a in range(No):
                for b in range(No):
                    if (cfg.ed_mode == "normal" and i != j) or (cfg.bath_type == "normal" and a != b):
                        continue
                    dm[i, j, a, b] = ev(cd[a + i * Ns] @ c[b + j * Ns])
    o["imp_density_matrix"] = dm
    # local energy
    h = cfg.impHloc
    ek = 0.0
    for a in range(No):
        for b in range(No):
            ek += (h[0, 0, a, b] * ev(cd[a] @ c[b])).real + (h[S, S, a, b] * ev(cd[a + Ns] @ c[b + Ns])).real
            if cfg.ed_mode == "nonsu2":
                ek += (h[0, 1, a, b] * ev(cd[a] @ c[b + Ns])).real + (h[1, 0, a, b] * ev(cd[a + Ns] @ c[b])).real
    o["eknot"] = ek
    U, Ust, Jh = cfg.Uloc, cfg.Ust, cfg.Jh
    dust = sum(ev(up[a] @ dw[b] + up[b] @ dw[a]).real for a in range(No) for b in range(a + 1, No))
    dund = sum(ev(up[a] @ up[b] + dw[a] @ dw[b]).real for a in range(No) for b in range(a + 1, No))
    dse = dph = 0.0
    if No > 1 and cfg.jhflag:
        for a in range(No):
            for b in range(No):
                if a != b:
                    dse += ev(cd[a] @ cd[b + Ns] @ c[a + Ns] @ c[b]).real
                    dph += ev(cd[a] @ cd[a + Ns] @ c[b + Ns] @ c[b]).real
    eh = 0.0
    if cfg.hfmode:
        eh += sum(-0.5 * U[a] * o["dens"][a] + 0.25 * U[a] for a in range(No))
        for a in range(No):
            for b in range(a + 1, No):
                eh += -0.5 * (2 * Ust - Jh) * (o["dens"][a] + o["dens"][b]) + 0.25 * (2 * Ust - Jh)
    o["epot"] = (sum(U[a] * o["docc"][a] for a in range(No)) + Ust * dust + (Ust - Jh) * dund
                 + cfg.Jx * dse + cfg.Jp * dph + eh)
    o.update(ehartree=eh, dust=dust, dund=dund, dse=dse, dph=dph, egs=min(states.energies))
    return o


OBS_FIELDS = ("dens", "dens_up", "dens_dw", "docc", "magz", "magx", "magy", "phisc", "sz2", "n2", "s2tot",
              "egs", "imp_density_matrix")
ENE_FIELDS = ("epot", "eknot", "ehartree", "dust", "dund", "dse", "dph")


def max_deviation(obs, ene, truth):
    """Largest absolute difference between (Observables, LocalEnergy) and dense_observables' dict."""
    d = 0.0
    for f in OBS_FIELDS:
        d = max(d, float(np.max(np.abs(np.asarray(getattr(obs, f)) - np.asarray(truth[f])))))
    for f in ENE_FIELDS:
        d = max(d, abs(getattr(ene, f) - truth[f]))
    return d
