"""Impurity observables and local energies of the kept states, on the device.

Mirrors observables_impurity (ED_OBSERVABLES.f90:48-715) and
local_energy_impurity (ED_OBSERVABLES.f90:726-980).  The reference copies
every kept vector to its master rank and walks it element by element with a
bdecomp and a binary_search per hit; here a kept state stays in HBM and costs

  * one ``Sector.nn_moments`` call on the 2*Norb impurity levels: the pair
    moments <n_p n_q> give every quantity of the diagonal loops (:127-158,
    :797-878, :929-943): dens, dens_up, dens_dw, docc, magz, sz2, n2, s2tot,
    the density-density part of <H_int>, Dust, Dund and the Hartree shift;
  * one ``Sector.expect`` call with every off-diagonal operator string of that
    state: the density matrices (:556-581, :631-654), magX / magY / phisc, the
    hopping part of Eknot (:802-846) and the Dse / Dph strings (:882-927).

Operator strings are lists of (level, op), op 1 = c^+, 0 = c, applied right to
left; level is the 0-based bit: impurity orbital a of spin s is a + s*Ns
(impIndex), replica bath level (a, k, s) is a + (k+1)*Norb + s*Ns (:621).

Multi-rank use follows build_gf: a rank evaluates the states whose vectors it
holds (``owners``; without owners the states are dealt round-robin), then one
all_reduce runs over the flat list of output numbers.  ``evaluator(cfg, sec,
vec, levels, terms) -> (M, norm, values)`` replaces the two device calls (the
CPU tests pass a numpy one); the package itself has no host fallback.

Not here: the exciton combinations (:341-515), which are linear in the
impurity density matrix, and the file output (write_observables).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .diag import StateList, state_vector
from .hamiltonian import Sector
from .params import EDConfig
from .sectors import LZDIAG, setup_pointers

Term = List[Tuple[int, int]]
CDG, C = 1, 0


@dataclass
class Observables:
    """observables_impurity's module variables (ED_OBSERVABLES.f90:75-102)."""

    dens: np.ndarray
    dens_up: np.ndarray
    dens_dw: np.ndarray
    docc: np.ndarray
    magz: np.ndarray
    magx: np.ndarray                 # nonsu2, else zeros
    magy: np.ndarray
    phisc: np.ndarray                # superc, else zeros
    sz2: np.ndarray                  # (Norb, Norb)
    n2: np.ndarray                   # (Norb, Norb)
    s2tot: float
    egs: float
    imp_density_matrix: np.ndarray   # (Nspin, Nspin, Norb, Norb) complex
    bth_density_matrix: Optional[np.ndarray] = None   # replica: (Nspin, Nspin, Norb, Norb, Nbath)


@dataclass
class LocalEnergy:
    """ed_Epot, ed_Eknot, ed_Ehartree, ed_Dust, ed_Dund, ed_Dse, ed_Dph
    (ED_OBSERVABLES.f90:747-753; epot includes ehartree, :962)."""

    epot: float
    eknot: float
    ehartree: float
    dust: float
    dund: float
    dse: float
    dph: float


# ------------------------------------------------------------------ strings
def imp_site(cfg: EDConfig, iorb: int, ispin: int) -> int:
    return iorb + ispin * cfg.Ns


def bath_site(cfg: EDConfig, iorb: int, ibath: int, ispin: int) -> int:
    """Replica bath level (ED_OBSERVABLES.f90:621), 0-based."""
    return iorb + (ibath + 1) * cfg.Norb + ispin * cfg.Ns


def term_conserves(cfg: EDConfig, term: Term) -> bool:
    """Does the string map every sector into itself (the library's compile
    rule; getCsector / getCDGsector summed over the string)?  In the Jz basis
    the reference drops the other strings row by row (``if(Jz_basis.and.j==0)
    cycle``, ED_OBSERVABLES.f90:809), here they are not sent at all."""
    Ns = cfg.Ns
    dup = ddw = djz = 0
    for lev, op in term:
        d = 1 if op else -1
        up = lev < Ns
        if up:
            dup += d
        else:
            ddw += d
        djz += d * (2 * LZDIAG[(lev % Ns) % cfg.Norb] + (1 if up else -1))
    if cfg.ed_mode == "normal":
        return dup == 0 and ddw == 0
    if cfg.ed_mode == "superc":
        return dup == ddw
    return dup + ddw == 0 and (not cfg.Jz_basis or djz == 0)


def _mask(cfg: EDConfig, ispin: int, jspin: int, iorb: int, jorb: int) -> bool:
    """dmft_bath%mask(ispin,jspin,iorb,jorb,1) .or. (...,2): |Re| or |Im| of
    impHloc above 1e-6 (init_dmft_bath_mask, ED_BATH/dmft_aux.f90:261-302)."""
    h = 0j if cfg.impHloc is None else complex(cfg.impHloc[ispin, jspin, iorb, jorb])
    return abs(h.real) > 1e-6 or abs(h.imag) > 1e-6


def density_matrix_entries(cfg: EDConfig, bath: Optional[int] = None):
    """(ispin, jspin, iorb, jorb) of the off-diagonal loop that are kept
    (ED_OBSERVABLES.f90:556-564 impurity, :631-637 bath level `bath`): no
    spin-off-diagonal entry in normal mode, no orbital-off-diagonal one for
    bath_type normal, the Jz mask rule (replica only for the impurity matrix).
    ispin == jspin, iorb == jorb never hits there (the diagonal is the density)."""
    out = []
    for ispin in range(cfg.Nspin):
        for jspin in range(cfg.Nspin):
            for iorb in range(cfg.Norb):
                for jorb in range(cfg.Norb):
                    if ispin == jspin and iorb == jorb:
                        continue
                    if cfg.ed_mode == "normal" and ispin != jspin:
                        continue
                    if cfg.bath_type == "normal" and iorb != jorb:
                        continue
                    jzrule = cfg.Jz_basis and (bath is not None or cfg.bath_type == "replica")
                    if jzrule and not _mask(cfg, ispin, jspin, iorb, jorb):
                        continue
                    out.append((ispin, jspin, iorb, jorb))
    return out


def observable_terms(cfg: EDConfig):
    """[(tag, string)] of observables_impurity's off-diagonal quantities."""
    out = []
    if cfg.ed_mode == "nonsu2":
        for a in range(cfg.Norb):   # magX + i magY = <c^+_{a up} c_{a dw}>
            out.append((("mag", a), [(imp_site(cfg, a, 0), CDG), (imp_site(cfg, a, 1), C)]))
    if cfg.ed_mode == "superc":
        for a in range(cfg.Norb):   # <c_{a up} c_{a dw}>
            out.append((("phi", a), [(imp_site(cfg, a, 0), C), (imp_site(cfg, a, 1), C)]))
    for (i, j, a, b) in density_matrix_entries(cfg):
        out.append((("imp", i, j, a, b), [(imp_site(cfg, a, i), CDG), (imp_site(cfg, b, j), C)]))
    if cfg.bath_type == "replica":
        for k in range(cfg.Nbath):
            for s in range(cfg.Nspin):
                for a in range(cfg.Norb):   # the bath densities as number operators c^+_p c_p
                    p = bath_site(cfg, a, k, s)
                    out.append((("bth", s, s, a, a, k), [(p, CDG), (p, C)]))
            for (i, j, a, b) in density_matrix_entries(cfg, bath=k):
                out.append((("bth", i, j, a, b, k), [(bath_site(cfg, a, k, i), CDG), (bath_site(cfg, b, k, j), C)]))
    return [(tag, t) for tag, t in out if term_conserves(cfg, t)]


def energy_terms(cfg: EDConfig):
    """[(tag, coefficient, string)] of local_energy_impurity's off-diagonal sums,
    in the reference's operator order."""
    S = cfg.Nspin - 1
    h = cfg.impHloc
    out = []
    for a in range(cfg.Norb):
        for b in range(cfg.Norb):
            if a == b:
                continue
            up = [(imp_site(cfg, a, 0), CDG), (imp_site(cfg, b, 0), C)]          # :805-812
            dw = [(imp_site(cfg, a, 1), CDG), (imp_site(cfg, b, 1), C)]          # :815-820
            out.append(("hop", 0j if h is None else complex(h[0, 0, a, b]), up))
            out.append(("hop", 0j if h is None else complex(h[S, S, a, b]), dw))
    if cfg.ed_mode == "nonsu2" and h is not None:
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                if h[0, S, a, b] != 0:                                           # :829-834
                    out.append(("hop", complex(h[0, S, a, b]), [(imp_site(cfg, a, 0), CDG), (imp_site(cfg, b, 1), C)]))
                if h[S, 0, a, b] != 0:                                           # :837-842
                    out.append(("hop", complex(h[S, 0, a, b]), [(imp_site(cfg, a, 1), CDG), (imp_site(cfg, b, 0), C)]))
    if cfg.Norb > 1 and cfg.jhflag:
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                if a == b:
                    continue
                up_a, dw_a = imp_site(cfg, a, 0), imp_site(cfg, a, 1)
                up_b, dw_b = imp_site(cfg, b, 0), imp_site(cfg, b, 1)
                # c^+_{a up} c^+_{b dw} c_{a dw} c_{b up}   (:891-894)
                out.append(("dse", cfg.Jx, [(up_a, CDG), (dw_b, CDG), (dw_a, C), (up_b, C)]))
                # c^+_{a up} c^+_{a dw} c_{b dw} c_{b up}   (:916-919)
                out.append(("dph", cfg.Jp, [(up_a, CDG), (dw_a, CDG), (dw_b, C), (up_b, C)]))
    return [(tag, c, t) for tag, c, t in out if term_conserves(cfg, t)]


# ---------------------------------------------------------------- evaluation
class _DeviceEvaluator:
    """The two device calls on a direct (matrix-free) sector handle per
    symmetry sector, kept for the states that share it."""

    def __init__(self, device: int):
        self.device, self.cache = device, {}

    def sector(self, cfg, sec) -> Sector:
        key = (sec.q1, sec.q2)
        if key not in self.cache:
            self.cache[key] = Sector(cfg, sec.q1, sec.q2, stored=False, direct=True, real=cfg.is_real(),
                                     device=self.device)
        return self.cache[key]

    def __call__(self, cfg, sec, vec, levels, terms):
        S = self.sector(cfg, sec)
        if isinstance(vec, np.ndarray):      # a dense sector's host vector: one upload for both calls
            _, vec, _ = S._state_arg(vec)
        M, norm = S.nn_moments(vec, levels)
        vals = S.expect(vec, terms) if terms else np.zeros(0, dtype=np.complex128)
        return M, norm, vals

    def close(self):
        for S in self.cache.values():
            S.close()
        self.cache.clear()


def _dist():
    try:
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _per_state(cfg: EDConfig, states: StateList, device: int, weights, owners, evaluator, terms, fold, nout: int):
    """Shared driver: for every kept state this rank evaluates, one moments
    call on the impurity levels and one expect call with `terms`;
    fold(out, weight, M, norm, values) adds the state into the flat output,
    which is summed over the ranks once."""
    dist = _dist()
    rank = dist.get_rank() if dist else 0
    world = dist.get_world_size() if dist else 1
    n = states.size
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
    elif states.finite_t:           # peso / zeta_function (ED_OBSERVABLES.f90:119-120)
        w = states.weights() / states.zeta
    else:
        w = np.full(n, 1.0 / n)
    if w.shape != (n,):
        raise ValueError("weights: one per kept state")
    levels = [imp_site(cfg, a, 0) for a in range(cfg.Norb)] + [imp_site(cfg, a, 1) for a in range(cfg.Norb)]
    secs = setup_pointers(cfg)
    out = np.zeros(nout)
    ev = evaluator if evaluator is not None else _DeviceEvaluator(device)
    try:
        for k in range(n):
            mine = (owners[k] == rank) if (owners is not None and world > 1) else (k % world == rank)
            if not mine:
                continue
            sector_of = (lambda s: ev.sector(cfg, s)) if isinstance(ev, _DeviceEvaluator) else None
            vec = state_vector(cfg, states, k, device, sector_of)
            if vec is None:
                raise ValueError("the observables need the state vectors (keep_vectors=True; multi-rank: owners)")
            M, norm, vals = ev(cfg, secs[states.sectors[k] - 1], vec, levels, terms)
            fold(out, float(w[k]), np.asarray(M), float(norm), np.asarray(vals, dtype=np.complex128))
    finally:
        if evaluator is None:
            ev.close()
    if world > 1:
        import torch

        t = torch.from_numpy(out)
        if dist.get_backend() == "nccl":
            t = t.to(torch.device("cuda", device))
            dist.all_reduce(t)
            out = t.cpu().numpy()
        else:
            dist.all_reduce(t)
    return out, w


def observables(cfg: EDConfig, states: StateList, device: int = 0, weights: Optional[Sequence[float]] = None,
                owners: Optional[List[int]] = None, evaluator=None) -> Observables:
    """observables_impurity (ED_OBSERVABLES.f90:48-715) from device-resident
    state vectors.  weights[k] is the Boltzmann factor of kept state k divided
    by the partition function (peso/zeta_function, :119-120); default:
    states.weights() / states.zeta, which at T=0 is 1/states.size.  A twin
    entry is evaluated from its partner's vector reordered on the device
    (state_vector) by the rank that owns the partner.

    magx, magy (nonsu2): Re and Im of <c^+_{a up} c_{a dw}>.  The reference
    takes them from two seed norms (:234-337): expanding
    |(c_up + c_dw) psi|^2 = n_up + n_dw + 2 Re<c^+_up c_dw> and
    |(i c_up + c_dw) psi|^2 = n_up + n_dw + 2 Im<c^+_up c_dw> shows that
    0.5*(norm - dens_up - dens_dw) are exactly these two numbers.  In the Jz
    basis the string changes Jz and both are zero.

    phisc (superc): the reference's number (:166-231).  Its seed norm is
    |(c^+_up + c_dw) psi|^2 = (1 - n_up) + n_dw + 2 Re<c_up c_dw>, from which it
    subtracts dens_up + (1 - dens_dw) — not the (1 - dens_up) + dens_dw the
    norm contains — so phisc = Re<c_up c_dw> + dens_dw - dens_up (plus
    0.5*(sum(weights) - 1), zero for normalised weights).  The quirk is kept.

    imp_density_matrix[is, js, a, b] = <c^+_{a is} c_{b js}> with the
    reference's skip rules (:556-564); bth_density_matrix likewise per replica
    bath level (:591-661), None for the other bath types."""
    No, Nsp, Nb = cfg.Norb, cfg.Nspin, cfg.Nbath
    tagged = observable_terms(cfg)
    terms = [t for _, t in tagged]
    nt = len(terms)
    nM = 2 * No
    nout = nM * nM + 1 + 2 * nt

    def fold(out, wk, M, norm, vals):
        out[: nM * nM] += wk * M.reshape(-1)
        out[nM * nM] += wk * norm
        out[nM * nM + 1: nM * nM + 1 + nt] += wk * vals.real
        out[nM * nM + 1 + nt:] += wk * vals.imag

    out, w = _per_state(cfg, states, device, weights, owners, evaluator, terms, fold, nout)
    M = out[: nM * nM].reshape(nM, nM)
    vals = out[nM * nM + 1: nM * nM + 1 + nt] + 1j * out[nM * nM + 1 + nt:]
    uu, dd, ud = M[:No, :No], M[No:, No:], M[:No, No:]
    dens_up, dens_dw = np.diag(uu).copy(), np.diag(dd).copy()
    docc = np.diag(ud).copy()
    sz2 = 0.25 * (uu - ud - ud.T + dd)
    n2 = uu + ud + ud.T + dd
    magx, magy, phisc = np.zeros(No), np.zeros(No), np.zeros(No)
    imp = np.zeros((Nsp, Nsp, No, No), dtype=np.complex128)
    bth = np.zeros((Nsp, Nsp, No, No, Nb), dtype=np.complex128) if cfg.bath_type == "replica" else None
    for a in range(No):
        imp[0, 0, a, a] += dens_up[a]
        if Nsp == 2:
            imp[1, 1, a, a] += dens_dw[a]
    if cfg.ed_mode == "superc":
        phisc += dens_dw - dens_up + 0.5 * (float(np.sum(w)) - 1.0)
    for (tag, _), v in zip(tagged, vals):
        if tag[0] == "mag":
            magx[tag[1]], magy[tag[1]] = v.real, v.imag
        elif tag[0] == "phi":
            phisc[tag[1]] += v.real
        elif tag[0] == "imp":
            imp[tag[1:]] += v
        else:
            bth[tag[1:]] += v
    return Observables(dens=dens_up + dens_dw, dens_up=dens_up, dens_dw=dens_dw, docc=docc,
                       magz=dens_up - dens_dw, magx=magx, magy=magy, phisc=phisc, sz2=sz2, n2=n2,
                       s2tot=float(np.sum(sz2)), egs=float(states.emin), imp_density_matrix=imp,
                       bth_density_matrix=bth)


def local_energy(cfg: EDConfig, states: StateList, device: int = 0, weights: Optional[Sequence[float]] = None,
                 owners: Optional[List[int]] = None, evaluator=None) -> LocalEnergy:
    """local_energy_impurity (ED_OBSERVABLES.f90:726-980): eknot = <impHloc>
    (diagonal part from the densities, :800; hopping part Re sum h_ab
    <c^+_a c_b>, :802-846, the nonSU2 spin-flip entries only where impHloc is
    non-zero, as there), epot = <H_int> (:852-927) + ehartree (:930-943, :962),
    and the correlators dust, dund, dse, dph.  The reference adds the complex
    hopping and exchange sums into real variables, i.e. keeps their real part."""
    No, S = cfg.Norb, cfg.Nspin - 1
    tagged = energy_terms(cfg)
    terms = [t for _, _, t in tagged]
    nt = len(terms)
    nM = 2 * No
    nout = nM * nM + 1 + nt

    def fold(out, wk, M, norm, vals):
        out[: nM * nM] += wk * M.reshape(-1)
        out[nM * nM] += wk * norm
        out[nM * nM + 1:] += wk * np.array([(c * v).real if tag == "hop" else v.real
                                             for (tag, c, _), v in zip(tagged, vals)])

    out, _ = _per_state(cfg, states, device, weights, owners, evaluator, terms, fold, nout)
    M = out[: nM * nM].reshape(nM, nM)
    norm = out[nM * nM]
    vals = out[nM * nM + 1:]
    uu, dd, ud = M[:No, :No], M[No:, No:], M[:No, No:]
    nup, ndw = np.diag(uu), np.diag(dd)
    h = cfg.impHloc
    eknot = 0.0
    if h is not None:
        eknot += float(np.dot(np.real(np.diag(h[0, 0])), nup) + np.dot(np.real(np.diag(h[S, S])), ndw))
    epot = float(sum(cfg.Uloc[a] * ud[a, a] for a in range(No)))
    dust = dund = dse = dph = ehartree = 0.0
    for a in range(No):
        for b in range(a + 1, No):
            dust += ud[a, b] + ud[b, a]
            dund += uu[a, b] + dd[a, b]
    epot += cfg.Ust * dust + (cfg.Ust - cfg.Jh) * dund
    for (tag, c, _), v in zip(tagged, vals):
        if tag == "hop":
            eknot += v
        elif tag == "dse":
            dse += v
        else:
            dph += v
    epot += cfg.Jx * dse + cfg.Jp * dph
    if cfg.hfmode:
        for a in range(No):
            ehartree += -0.5 * cfg.Uloc[a] * (nup[a] + ndw[a]) + 0.25 * cfg.Uloc[a] * norm
        for a in range(No):
            for b in range(a + 1, No):
                nn = nup[a] + ndw[a] + nup[b] + ndw[b]
                ehartree += -0.5 * cfg.Ust * nn + 0.25 * cfg.Ust * norm
                ehartree += -0.5 * (cfg.Ust - cfg.Jh) * nn + 0.25 * (cfg.Ust - cfg.Jh) * norm
    return LocalEnergy(epot=float(epot + ehartree), eknot=float(eknot), ehartree=float(ehartree),
                       dust=float(dust), dund=float(dund), dse=float(dse), dph=float(dph))
