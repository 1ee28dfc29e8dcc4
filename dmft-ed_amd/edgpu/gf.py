"""Impurity Green's function by Lanczos continued fraction, normal mode.

Mirrors build_gf_normal / lanc_build_gf_normal_c / add_to_lanczos_gf_normal
(ED_GF_NORMAL.f90:18-92, 116-260, 580-632) for the diagonal components
G_{aa,ss}, and lanc_build_gf_normal_mix_c (ED_GF_NORMAL.f90:279-553) for the
orbital off-diagonal G_{ab,ss} of hybrid and replica baths (`orbital_pairs`,
four two-term seeds per pair and kept state, recombined in build_gf).
Per kept state |gs> (energy E_i), orbital a, spin s:

  * seed  c+_{a s}|gs>  in sector getCDGsector(s, isector)  and
          c_{a s}|gs>   in sector getCsector(s, isector),
    built on the GPU (ed_sector_apply_op, the vvinit loop :159-174);
  * norm2 = <seed|seed>, seed /= sqrt(norm2);
  * nlanc = min(jdim, lanc_nGFiter) steps of sp_lanc_tridiag on the GPU
    (device-resident plain Lanczos from a device start vector);
  * poles: eigenvalues and squared first eigenvector components of the
    tridiagonal (diag alfa, subdiag beta(2:)) by `ed_tridiag_poles` (implicit
    QL on the first row of Z, the tql2 iteration), weight norm2/Z * Z(1,j)^2,
    G(iw_n) += w/(iw_n - isign*(E_j - E_i)), G(w) += w/(w + i eps - isign*(E_j - E_i))
    with w_n = pi/beta (2n-1) and w = linspace(wini, wfin, Lreal)
    (allocate_grids, ED_AUX_FUNX.f90:449-461).
The pole sums of all seeds run in one device kernel (ed_gf_add_poles) into
G arrays kept in HBM, in the serial job order and the reference's per-pole
addition order; the frequency grids are uploaded once per build and G is
copied to the host (or all-reduced on the device) once at the end.

ed_mode superc: build_gf_superc (ED_GF_SUPERC.f90:18-77, 88-446, 757-803),
the orbital-diagonal normal G and anomalous F from six seeds per orbital and
kept state in three aux channels, through the same machinery.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check
from .diag import StateList, is_complex_vector, state_vector
from .hamiltonian import Sector
from .params import EDConfig
from .sectors import c_sector, cdg_sector, setup_pointers


@dataclass
class GFOptions:
    """ED_INPUT_VARS defaults (ED_INPUT_VARS.f90:126-173)."""

    lanc_nGFiter: int = 200
    Lmats: int = 5000
    Lreal: int = 5000
    beta: float = 1000.0
    eps: float = 0.01
    wini: float = -5.0
    wfin: float = 5.0
    threshold: float = 1e-13      # sp_lanc_tridiag breakdown test (.repo/PLAIN_LANCZOS.f90:27)
    sparse_H: bool = True         # ed_sparse_H
    # seeds solved concurrently on one GPU (host threads, each with its own
    # device sectors); contributions are added to G in job order, so the
    # result is bit-identical to the serial loop
    workers: int = 4
    # seeds grouped by target sector: one sector build and one batched
    # persistent Lanczos launch per group (one workgroup per seed,
    # ed_sector_lanc_tridiag_batch); bit-identical to the per-seed runs
    batch: bool = True
    # hybrid / replica baths: the orbital off-diagonal G[s, s, a, b] of
    # build_gf_normal (ED_GF_NORMAL.f90:33-72).  False: orbital-diagonal only
    orbital_mix: bool = True
    # batched path: every seed of one (kept state, operator type, target
    # sector, vector type) group from one ed_sector_seed_batch call, written
    # straight into the stacked tensor of the batched Lanczos launch.  Only the
    # summation order of norm2 differs from the per-seed chain.  superc: one
    # ed_sector_seed_plan call per (kept state, target sector, vector type)
    fused_seeds: bool = False
    # the seeds of a target sector whose Lanczos runs are not persistent (the
    # large sectors) advance in lockstep groups of 8, 4, 2, 1 through one block
    # H·X per Krylov step (ed_sector_lanc_tridiag_lockstep) instead of one
    # after the other.  alfa and beta then differ from the serial runner's by
    # the summation order of the two dot products of a step
    lockstep: bool = False


# fused_seeds: a stacked seed buffer (one batched Lanczos launch) stays under
# this many bytes; larger groups are tridiagonalised in chunks (a complex seed
# of a dim 11.8 M sector is 189 MB: 11 seeds per chunk)
SEED_BUFFER_BYTES = 2 << 30
SEED_MAX_LEVELS, SEED_MAX_SEEDS = 6, 32   # kSeedMaxLev, kSeedMaxSeeds (csrc/ed_seed_plan.hpp)


def matsubara(beta: float, L: int) -> np.ndarray:
    return np.pi / beta * (2.0 * np.arange(1, L + 1) - 1.0)


def realaxis(wini: float, wfin: float, L: int) -> np.ndarray:
    return np.linspace(wini, wfin, L)


def tridiag_poles(alfa: np.ndarray, beta: np.ndarray, n: int, first_row: bool = False):
    """Eigenvalues of tridiag(alfa(1:n), beta(2:n)) and squared first components
    (tql2 / eigh of add_to_lanczos_gf_*, ED_GF_NONSU2.f90:936, ED_GF_NORMAL.f90:
    612-618): `ed_tridiag_poles`, the implicit-QL iteration carrying only the
    first row of the eigenvector matrix (O(n^2)).  first_row: return the
    components Z(1,j) themselves instead of their squares."""
    a = np.ascontiguousarray(alfa[:n], dtype=np.float64)
    b = np.zeros(n, dtype=np.float64)
    b[1:n] = beta[1:n]
    E = np.empty(n, dtype=np.float64)
    z2 = np.empty(n, dtype=np.float64)
    z1 = np.empty(n, dtype=np.float64)
    check(_lib.load().ed_tridiag_poles(n, a.ctypes.data, b.ctypes.data, E.ctypes.data, z2.ctypes.data,
                                       z1.ctypes.data), "ed_tridiag_poles")
    return (E, z1) if first_row else (E, z2)


class PoleSums:
    """Device side of add_to_lanczos_gf_normal / _nonsu2 (ED_GF_NORMAL.f90:
    620-631, ED_GF_NONSU2.f90:936-950): the frequency grids are uploaded once,
    G lives in HBM as (Nspin, Nspin, Norb, Norb, L) complex arrays, and `add`
    queues one continued fraction (its poles from ed_tridiag_poles) for
    component (ispin, jspin, iorb, jorb), or (ispin, jspin, iorb) meaning
    jorb = iorb.  `flush` sums every queued fraction in one launch of
    ed_gf_add_poles, in queue order and pole by pole (the reference's order of
    additions into G(i)).  With `ncomp` the arrays are (ncomp, L) instead and
    a component is its flat index (the aux channels of build_gf_superc)."""

    def __init__(self, nspin: int, norb: int, wm: np.ndarray, wr: np.ndarray, eps: float, device: int,
                 ncomp: Optional[int] = None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("the Green's function pole sum runs on the GPU (no host fallback)")
        self.dev = torch.device("cuda", device)
        self.nspin, self.norb, self.eps = nspin, norb, float(eps)
        self.wm = torch.from_numpy(np.ascontiguousarray(wm, dtype=np.float64)).to(self.dev)
        self.wr = torch.from_numpy(np.ascontiguousarray(wr, dtype=np.float64)).to(self.dev)
        shape = (nspin, nspin, norb, norb) if ncomp is None else (ncomp,)
        self.ncomp = ncomp
        self.Gm = torch.zeros(shape + (len(wm),), dtype=torch.complex128, device=self.dev)
        self.Gr = torch.zeros(shape + (len(wr),), dtype=torch.complex128, device=self.dev)
        self._q = []

    def add(self, comp, peso_bz, Ei: float, E: np.ndarray, z: np.ndarray, isign: int) -> None:
        if self.ncomp is not None:
            c = int(comp)
            assert 0 <= c < self.ncomp
        else:
            ispin, jspin, iorb = comp[:3]
            jorb = comp[3] if len(comp) > 3 else iorb
            c = ((ispin * self.nspin + jspin) * self.norb + iorb) * self.norb + jorb
        pb = complex(peso_bz)
        self._q.append((c, pb.real, pb.imag, float(Ei), int(isign), np.asarray(E, np.float64),
                        np.asarray(z, np.float64)))

    def flush(self) -> None:
        import torch

        if not self._q:
            return
        q, self._q = self._q, []
        npole = np.array([len(t[5]) for t in q], dtype=np.int32)
        E = np.ascontiguousarray(np.concatenate([t[5] for t in q]))
        z = np.ascontiguousarray(np.concatenate([t[6] for t in q]))
        pb = np.ascontiguousarray(np.array([[t[1], t[2]] for t in q], dtype=np.float64).reshape(-1))
        ei = np.array([t[3] for t in q], dtype=np.float64)
        sg = np.array([t[4] for t in q], dtype=np.int32)
        comp = np.array([t[0] for t in q], dtype=np.int32)
        st = torch.cuda.current_stream(self.dev)
        P = ctypes.c_void_p
        check(_lib.load().ed_gf_add_poles(len(q), P(npole.ctypes.data), P(E.ctypes.data), P(z.ctypes.data),
                                          P(pb.ctypes.data), P(ei.ctypes.data), P(sg.ctypes.data),
                                          P(comp.ctypes.data), P(self.wm.data_ptr()), self.wm.numel(),
                                          P(self.wr.data_ptr()), self.wr.numel(), self.eps,
                                          P(self.Gm.data_ptr()), P(self.Gr.data_ptr()), P(st.cuda_stream)),
              "ed_gf_add_poles")

    def to_host(self, Gm: np.ndarray, Gr: np.ndarray) -> None:
        """Add the device G into the host arrays of the same shape."""
        Gm += self.Gm.cpu().numpy()
        Gr += self.Gr.cpu().numpy()


def _seed(src: Sector, dst: Sector, op: int, terms, vec: np.ndarray, cplx: bool):
    """Seed sum_t coef_t * op_{level_t}|vec> on the device (first term assigned,
    the rest accumulated, as the vvinit loops of ED_GF_NORMAL/ED_GF_NONSU2);
    returns (normalised seed, norm2).  A term is (level, coef) with the seed's
    `op`, or (level, coef, op_t) with an operator type of its own (the superc
    seeds c+_up + c_dw, ED_GF_SUPERC.f90:332-349); the library checks per call
    that every term reaches dst."""
    import torch

    real = not cplx
    dt = torch.float64 if real else torch.complex128
    dev = f"cuda:{src.device}"
    if isinstance(vec, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(vec.astype(np.float64 if real else np.complex128))).to(dev)
    else:                                   # state vector kept in HBM by the farm
        x = vec.to(device=dev, dtype=dt).contiguous()
    y = torch.empty(dst.dim, dtype=dt, device=dev)
    st = torch.cuda.current_stream(x.device)
    L = _lib.load()
    vt = 0 if real else 1
    xp, yp, sp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(st.cuda_stream)
    ops = [t[2] if len(t) > 2 else op for t in terms]
    assert terms[0][1] == 1
    check(L.ed_sector_apply_op(src.handle, dst.handle, ops[0], terms[0][0], vt, xp, yp, sp), "ed_sector_apply_op")
    for (lvl, c, *_), o in zip(terms[1:], ops[1:]):
        check(L.ed_sector_apply_op_acc(src.handle, dst.handle, o, lvl, float(np.real(c)), float(np.imag(c)),
                                       vt, xp, yp, sp), "ed_sector_apply_op_acc")
    norm2 = float(torch.sum(y.abs() ** 2).item())
    if norm2 > 0:
        y = y / np.sqrt(norm2)
    y = y.contiguous()
    st.synchronize()   # the seed is complete for the library's stream (no device-wide sync:
    return y, norm2    # other threads may be capturing graphs)


def _tridiag_dev(S: Sector, seed, nlanc: int, real: bool, threshold: float):
    a = np.zeros(nlanc)
    b = np.zeros(nlanc)
    n = ctypes.c_int32()
    check(_lib.load().ed_sector_lanc_tridiag_dev(S.handle, 0 if real else 1,
                                                 ctypes.c_void_p(seed.data_ptr()), nlanc, threshold,
                                                 a.ctypes.data_as(ctypes.c_void_p),
                                                 b.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)),
          "ed_sector_lanc_tridiag_dev")
    return a, b, int(n.value)


def _target(cfg: EDConfig, sec, op: int, ispin: int, iorb: int = 0):
    return cdg_sector(cfg, sec, ispin, iorb) if op == 1 else c_sector(cfg, sec, ispin, iorb)


class _SectorCache:
    """Device sectors reused across the seeds of one GF build (the reference
    rebuilds them per seed with build_Hv_sector / delete_Hv_sector)."""

    def __init__(self, cfg, gopt, device):
        self.cfg, self.gopt, self.device, self.d = cfg, gopt, device, {}
        self.aux = {}      # small device tensors that live as long as the sectors

    def get(self, sec, hamiltonian: bool) -> Sector:
        key = (sec.q1, sec.q2, hamiltonian)
        if key not in self.d:
            stored = hamiltonian and self.gopt.sparse_H
            self.d[key] = Sector(self.cfg, sec.q1, sec.q2, stored=stored, direct=not stored,
                                 real=self.cfg.is_real(), device=self.device)
        return self.d[key]

    def close(self):
        for S in self.d.values():
            S.close()
        self.d.clear()
        self.aux.clear()


def mixed_pairs(cfg: EDConfig):
    """(ispin, jspin, iorb) of the spin-off-diagonal nonsu2 components
    (build_gf_nonsu2 ED_GF_NONSU2.f90:39-48 normal/hybrid: all of them;
    :203-217 replica: only where dmft_bath%mask(ispin,jspin,iorb,iorb,:) is set,
    i.e. |Re or Im impHloc(ispin,jspin,iorb,iorb)| > 1e-6, init_dmft_bath_mask
    ED_BATH/dmft_aux.f90:261-302)."""
    if cfg.ed_mode != "nonsu2":
        return []
    Nsp, No = cfg.Nspin, cfg.Norb
    out = []
    for s1 in range(Nsp):
        for s2 in range(Nsp):
            for o in range(No):
                if s1 == s2:
                    continue
                if cfg.bath_type == "replica":
                    h = 0j if cfg.impHloc is None else cfg.impHloc[s1, s2, o, o]
                    if not (abs(h.real) > 1e-6 or abs(h.imag) > 1e-6):
                        continue
                out.append((s1, s2, o))
    return out


def orbital_pairs(cfg: EDConfig):
    """(ispin, iorb, jorb), iorb < jorb, of the orbital off-diagonal components
    of build_gf_normal (ED_GF_NORMAL.f90:33-50), in the reference's loop order:
    none for bath_type normal; hybrid: all of them; replica: only where
    dmft_bath%mask(ispin,ispin,iorb,jorb,1:2) is set (ED_GF_NORMAL.f90:40-42),
    i.e. |Re or Im impHloc(ispin,ispin,iorb,jorb)| > 1e-6 (init_dmft_bath_mask,
    ED_BATH/dmft_aux.f90:261-302).  Empty for nonsu2 and superc."""
    if cfg.ed_mode != "normal" or cfg.bath_type == "normal":
        return []
    out = []
    for s in range(cfg.Nspin):
        for a in range(cfg.Norb):
            for b in range(a + 1, cfg.Norb):
                if cfg.bath_type == "replica":
                    h = 0j if cfg.impHloc is None else complex(cfg.impHloc[s, s, a, b])
                    if not (abs(h.real) > 1e-6 or abs(h.imag) > 1e-6):
                        continue
                out.append((s, a, b))
    return out


class Seed(NamedTuple):
    """A seed spec: sum_t coef_t op_t|gs> over `terms`, rows (level, coef) with
    the seed's `op` (0 c, 1 c^+) or (level, coef, op_t) with their own; `ispin`
    is the spin of the first level, `weight` multiplies norm2 in the pole sum."""

    op: int
    isign: int
    ispin: int
    terms: list
    weight: complex


class Job(NamedTuple):
    """One continued fraction: component `comp` of G, the channel `tag`, kept
    state `k`, its seed, and the sectors of the kept state and of the seed."""

    comp: object
    tag: tuple
    k: int
    seed: Seed
    src: object
    dst: object


def _job_list(cfg: EDConfig, states: StateList, orbital_mix: bool = True):
    """Every `Job` of build_gf in the serial accumulation order: diagonal
    components (ispin, iorb), then for nonSU2 the mixed seeds (ispin != jspin,
    iorb), then (normal mode, hybrid / replica bath, `orbital_mix`) the
    orbital-mixed seeds (ispin, iorb < jorb) of lanc_build_gf_normal_mix_c.  A
    component is (ispin, jspin, iorb, jorb)."""
    Ns, No, Nsp = cfg.Ns, cfg.Norb, cfg.Nspin
    site = lambda o, s: o + s * Ns          # impIndex(iorb,ispin), 0-based bit
    chans = []
    for ispin in range(Nsp):
        for iorb in range(No):
            i = site(iorb, ispin)
            chans.append(((ispin, ispin, iorb, iorb), ("diag", ispin, iorb),
                          [(1, +1, ispin, [(i, 1)], 1.0), (0, -1, ispin, [(i, 1)], 1.0)]))
    pairs = mixed_pairs(cfg)
    if pairs:
        if cfg.Jz_basis:
            # the reference builds the second term of a mixed seed in the sector
            # of (jorb,jspin) (ED_GF_NONSU2.f90:576-584), a different Jz sector
            raise NotImplementedError("mixed nonsu2 seeds in the Jz basis")
        for ispin, jspin, iorb in pairs:
            i, j = site(iorb, ispin), site(iorb, jspin)
            chans.append(((ispin, jspin, iorb, iorb), ("mix", ispin, jspin, iorb), [
                (1, +1, ispin, [(i, 1), (j, 1)], 1.0),         # (c+_i + c+_j)|gs>      :571-595
                (0, -1, ispin, [(i, 1), (j, 1)], 1.0),         # (c_i + c_j)|gs>        :654-678
                (1, +1, ispin, [(i, 1), (j, 1j)], 1j),         # (c+_i + i c+_j)|gs>    :739-763, cnorm2=i*norm2
                (0, -1, ispin, [(i, 1), (j, -1j)], 1j),        # (c_i - i c_j)|gs>      :823-847
            ]))
    if orbital_mix:
        # lanc_build_gf_normal_mix_c: both levels have spin ispin, so the four
        # seeds of a pair live in the diagonal channels' target sectors; the
        # weight of the last two is -xi*norm2 (the nonSU2 routine's is +xi)
        for ispin, iorb, jorb in orbital_pairs(cfg):
            i, j = site(iorb, ispin), site(jorb, ispin)
            chans.append(((ispin, ispin, iorb, jorb), ("orbmix", ispin, iorb, jorb), [
                (1, +1, ispin, [(i, 1), (j, 1)], 1.0),         # (c+_i + c+_j)|gs>      ED_GF_NORMAL.f90:312-363
                (0, -1, ispin, [(i, 1), (j, 1)], 1.0),         # (c_i + c_j)|gs>        ED_GF_NORMAL.f90:371-421
                (1, +1, ispin, [(i, 1), (j, 1j)], -1j),        # (c+_i + i c+_j)|gs>    ED_GF_NORMAL.f90:429-480
                (0, -1, ispin, [(i, 1), (j, -1j)], -1j),       # (c_i - i c_j)|gs>      ED_GF_NORMAL.f90:488-539
            ]))
    secs = setup_pointers(cfg)
    jobs = []
    for comp, tag, seeds in chans:
        for k, isec in enumerate(states.sectors):
            sec = secs[isec - 1]
            for spec in seeds:
                jsec = _target(cfg, sec, spec[0], spec[2], comp[2])
                if jsec is not None:
                    jobs.append(Job(comp, tag, k, Seed(*spec), sec, jsec))
    return jobs, pairs


SUPERC_CHANNELS = 3      # auxGmats(1:3,:): G_aa, barG_aa, A_aa (ED_GF_SUPERC.f90:23-24)


def _job_list_superc(cfg: EDConfig, states: StateList):
    """Every `Job` of lanc_build_gf_superc_c (ED_GF_SUPERC.f90:88-446) in the
    order in which each aux channel accumulates: orbital, kept state, then the
    six seeds.  A component is the flat index iorb * 3 + channel (channel 0:
    G_aa, 1: barG_aa, 2: A_aa); a seed is Seed(op of the first term, isign, 0,
    [(level, 1, op)], 1.0): every term carries its own operator type.  c+_up
    and c_dw raise sz by one, c_up and c+_dw lower it; a seed whose target
    sector does not exist is left out."""
    Ns = cfg.Ns
    secs = setup_pointers(cfg)
    by_sz = {s.q1: s for s in secs}
    jobs = []
    for iorb in range(cfg.Norb):
        up, dw = iorb, iorb + Ns
        seeds = [                                               # ED_GF_SUPERC.f90
            (0, +1, +1, [(up, 1, 1)]),                          # c+_up|n>            :119-166
            (0, -1, -1, [(up, 1, 0)]),                          # c_up|n>             :168-217
            (1, +1, +1, [(dw, 1, 0)]),                          # c_dw|n>             :219-268
            (1, -1, -1, [(dw, 1, 1)]),                          # c+_dw|n>            :270-318
            (2, +1, +1, [(up, 1, 1), (dw, 1, 0)]),              # (c+_up + c_dw)|n>   :320-378
            (2, -1, -1, [(up, 1, 0), (dw, 1, 1)]),              # (c_up + c+_dw)|n>   :380-439
        ]
        for k, isec in enumerate(states.sectors):
            sec = secs[isec - 1]
            for chan, dsz, isign, terms in seeds:
                jsec = by_sz.get(sec.q1 + dsz)
                if jsec is not None:
                    jobs.append(Job(iorb * SUPERC_CHANNELS + chan, ("superc", chan, iorb), k,
                                    Seed(terms[0][2], isign, 0, terms, 1.0), sec, jsec))
    return jobs


def _peso_bz(states: StateList, k: int, weight, norm2: float, zeta: float):
    """pesoBZ of add_to_lanczos_gf_normal (ED_GF_NORMAL.f90:596-601) times the
    seed's weight: norm2 / zeta at T=0; at finite T norm2 exp(-beta (Ei - Egs))
    / zeta, and 0 once beta (Ei - Egs) reaches 200."""
    if not states.finite_t:
        return weight * norm2 / zeta
    x = states.beta * (states.energies[k] - states.emin)
    if not x < 200.0:
        return 0.0
    return weight * (norm2 * np.exp(-x) / zeta)


def _peso_superc(states: StateList, k: int, weight, norm2: float, zeta: float):
    """pesoBZ of add_to_lanczos_gf_superc (ED_GF_SUPERC.f90:781-782) times the
    seed's weight: norm2 / zeta at T=0, norm2 exp(-beta (Ei - Egs)) / zeta at
    finite T.  Unlike the normal-mode routine it has no beta (Ei - Egs) < 200
    cut (the cut is commented out there, ED_GF_SUPERC.f90:773-779)."""
    if not states.finite_t:
        return weight * norm2 / zeta
    return weight * (norm2 * np.exp(-states.beta * (states.energies[k] - states.emin)) / zeta)


def _peso(cfg: EDConfig):
    return _peso_superc if cfg.ed_mode == "superc" else _peso_bz


def superc_twin_sign(Ns: int, hmap: np.ndarray) -> np.ndarray:
    """The sign that makes a superc twin entry's vector an eigenvector.

    `state_vector` reorders the partner's vector by flip_state (the two Ns-bit
    halves exchanged) without a sign, as es_return_cvector does
    (ED_EIGENSPACE.f90:414-445).  In ed_mode superc that exchange P alone is
    no symmetry: it sends the pair term deltasc (c+_up c+_dw + h.c.) to minus
    itself, H(deltasc) -> H(-deltasc).  P followed by the gauge turn
    c -> i c is one, and in the Fock basis it is the reordering times
    i^(nup + ndw) (-1)^(nup ndw): within a sector (nup - ndw fixed) that is,
    up to one overall phase, the real sign (-1)^(ndw (1 + nup)) of the twin
    sector's row state.  Without it the reordered vector of a sz = +-1 sector
    of the Ns = 3 test model misses (H - E) v = 0 by 0.96; with it by 1e-15.
    Returns +-1.0 per row of `hmap` (the twin sector's map)."""
    m = np.asarray(hmap).astype(np.int64)
    pc = lambda v: sum((v >> b) & 1 for b in range(Ns))    # noqa: E731
    nup, ndw = pc(m & ((1 << Ns) - 1)), pc(m >> Ns)
    return 1.0 - 2.0 * ((ndw * (1 + nup)) & 1)


def _state_vec(cfg, states, k, cache):
    """Kept state k's vector; a twin entry's is rebuilt on the device from its
    partner's with the cache's (matrix-free) sector handles.  A superc twin
    vector also takes `superc_twin_sign` (kept on the device per twin sector):
    the Green's function needs eigenvectors."""
    vec = state_vector(cfg, states, k, cache.device, lambda s: cache.get(s, False))
    if cfg.ed_mode != "superc" or states.partner(k) is None or vec is None:
        return vec
    import torch

    sec = setup_pointers(cfg)[states.sectors[k] - 1]
    key = ("twin_sign", sec.q1)
    if key not in cache.aux:
        cache.aux[key] = torch.from_numpy(superc_twin_sign(cfg.Ns, cache.get(sec, False).map())).to(vec.device)
    return vec * cache.aux[key]


def _run_job(cfg, states, gopt, job, cache, poles, record, zeta):
    """One tridiagonalisation; its poles are queued on `poles` (PoleSums)."""
    comp, tag, k, (op, isign, ispin, terms, weight), sec, jsec = job
    e_i, vec = states.energies[k], _state_vec(cfg, states, k, cache)
    if vec is None:
        raise ValueError("the Green's function needs the state vectors (keep_vectors=True)")
    cplx = (not cfg.is_real()) or is_complex_vector(vec) or any(np.imag(t[1]) != 0 for t in terms)
    HI, HJ = cache.get(sec, False), cache.get(jsec, True)
    seed, norm2 = _seed(HI, HJ, op, terms, vec, cplx)
    if norm2 == 0.0:
        return
    nlanc = min(HJ.dim, gopt.lanc_nGFiter)
    a, b, n = _tridiag_dev(HJ, seed, nlanc, not cplx, gopt.threshold)
    # the reference diagonalises all nlanc entries (unset ones stay 0)
    E, z = tridiag_poles(a, b, nlanc, first_row=True)
    if record is not None:
        record.append(dict(channel=tag, isector=states.sectors[k], op=op, norm2=norm2, alfa=a, beta=b,
                           nlanc=n))
    poles.add(comp, _peso(cfg)(states, k, weight, norm2, zeta), e_i, E, z, isign)


# complex(8) vectors go in lockstep only on sectors of at most this many rows:
# the measured table of DESIGN.md §15 (profiles/lockstep/INDEX.md) has them
# faster at 853,776 rows and slower at 10,306,296; nothing between was measured
LOCKSTEP_COMPLEX_MAX_DIM = 853776


def _lockstep_seeds(S: Sector, nseed: int, real: bool) -> int:
    """How many of the nseed seeds of S, from the first, the lockstep entry
    takes; the others go through ed_sector_lanc_tridiag_batch.  None unless the
    sector holds the whole stored matrix and its Lanczos runs of this vector
    type are not persistent (those go in one batched launch, one workgroup per
    seed, already).  Then the group widths that measured faster than the
    sequential runs: 8, 4 and 2, so an odd seed count leaves
    its width-1 tail to the batch entry; complex vectors only up to
    LOCKSTEP_COMPLEX_MAX_DIM rows."""
    if not (S.stored_whole and S.lanc_mode(real=real) < 0):
        return 0
    if not real and S.dim > LOCKSTEP_COMPLEX_MAX_DIM:
        return 0
    return nseed - nseed % 2


def _tridiag_batch(S: Sector, seeds, nlanc: int, real: bool, threshold: float, lockstep: bool = False):
    """sp_lanc_tridiag of every seed (rows of the contiguous `seeds` tensor) on
    S; `lockstep`: the first _lockstep_seeds of them through
    Sector.lanc_tridiag_lockstep."""
    k = seeds.shape[0]
    head = _lockstep_seeds(S, k, real) if lockstep else 0
    if head == k:
        return S.lanc_tridiag_lockstep(seeds, nlanc, threshold)
    if head:
        first, rest = S.lanc_tridiag_lockstep(seeds[:head], nlanc, threshold), _tridiag_batch(S, seeds[head:], nlanc, real,
                                                                                              threshold)
        return tuple(np.concatenate(pair) for pair in zip(first, rest))
    a = np.zeros((k, nlanc))
    b = np.zeros((k, nlanc))
    n = np.zeros(k, dtype=np.int32)
    check(_lib.load().ed_sector_lanc_tridiag_batch(S.handle, 0 if real else 1, k,
                                                   ctypes.c_void_p(seeds.data_ptr()), nlanc, threshold,
                                                   a.ctypes.data_as(ctypes.c_void_p),
                                                   b.ctypes.data_as(ctypes.c_void_p),
                                                   n.ctypes.data_as(ctypes.c_void_p)),
          "ed_sector_lanc_tridiag_batch")
    return a, b, n


def _device_vec(vec, cplx: bool, device: int):
    import torch

    dt = torch.complex128 if cplx else torch.float64
    if isinstance(vec, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(vec.astype(np.complex128 if cplx else np.float64))).to(
            f"cuda:{device}")
    return vec.to(device=f"cuda:{device}", dtype=dt).contiguous()


def _seed_calls(jobs, members, mixed: bool):
    """Split `members` (jobs of one target sector and vector type) into fused
    seed calls of at most SEED_MAX_SEEDS seeds and SEED_MAX_LEVELS distinct
    images.  An image is a level and the calls are per (kept state, operator
    type) for ed_sector_seed_batch; `mixed` (terms with their own operator
    type, ed_sector_seed_plan): an image is (level, op) and the calls are per
    kept state.  Yields (k, op or None, images, members of the call)."""
    image = (lambda t: (t[0], t[2])) if mixed else (lambda t: t[0])
    by = {}
    for n in members:
        by.setdefault((jobs[n].k, None if mixed else jobs[n].seed.op), []).append(n)
    for (k, op), ns in by.items():
        images, call = [], []
        for n in ns:
            mine = list(dict.fromkeys(image(t) for t in jobs[n].seed.terms))
            new = [im for im in mine if im not in images]
            if call and (len(call) == SEED_MAX_SEEDS or len(images) + len(new) > SEED_MAX_LEVELS):
                yield k, op, images, call
                images, call, new = [], [], mine
            images += new
            call.append(n)
        yield k, op, images, call


def _fused_seeds(cfg, states, jobs, members, cache, cplx: bool, mixed: bool = False):
    """The normalised seeds of `members` as rows of one device tensor, and
    their norm2, one `_seed_calls` call after the other: Sector.seed_batch
    (k_seed_gather, csrc/ed_seed.hpp), or with `mixed` Sector.seed_plan
    (k_seed_plan).  Returns (members in row order, tensor, norm2)."""
    import torch

    HJ = cache.get(jobs[members[0]].dst, True)
    dt = torch.complex128 if cplx else torch.float64
    out = torch.empty((len(members), HJ.dim), dtype=dt, device=f"cuda:{cache.device}")
    rows, norms = [], []
    for k, op, images, call in _seed_calls(jobs, members, mixed):
        HI = cache.get(jobs[call[0]].src, False)
        x = _device_vec(_state_vec(cfg, states, k, cache), cplx, cache.device)
        into = out[len(rows):len(rows) + len(call)]
        if mixed:
            terms = np.full((len(call), 2), -1, dtype=np.int32)
            for s, n in enumerate(call):
                tt = jobs[n].seed.terms
                assert len(tt) <= 2 and all(c == 1 for _, c, _ in tt)     # unit coefficients: all superc needs
                for j, (lv, _, o) in enumerate(tt):
                    terms[s, j] = images.index((lv, o))
            _, n2 = HI.seed_plan(x, HJ, [lv for lv, _ in images], [o for _, o in images], terms, out=into)
        else:
            coef = np.zeros((len(call), len(images)), dtype=np.complex128)
            for q, n in enumerate(call):
                for lv, c in jobs[n].seed.terms:
                    coef[q, images.index(lv)] = c
            _, n2 = HI.seed_batch(x, HJ, op, images, coef, out=into)
        rows += call
        norms += list(n2)
    return rows, out, norms


def seed_fractions(S: Sector, make, nseed: int, cplx: bool, nlanc: int, threshold: float, chunked: bool = True,
                   lockstep: bool = False):
    """From seed calls to continued fractions, for build_gf, build_gf_superc
    and build_chi.  make(rows) -> (device tensor, norm2) builds the normalised
    seeds `rows` (a range of 0..nseed-1) of sector S as the tensor's rows;
    `chunked`: a tensor stays under SEED_BUFFER_BYTES.  Seeds with norm2 == 0
    are dropped (no fraction), the others of a tensor tridiagonalised in one
    batched launch.  Yields (seed index, norm2, alfa, beta, nlanc found, E, z)
    in seed order, E and z(1, j) from `tridiag_poles` over all `nlanc` entries
    (the reference diagonalises them all; unset ones stay 0).  `lockstep`:
    GFOptions.lockstep."""
    import torch

    step = max(1, SEED_BUFFER_BYTES // (S.dim * (16 if cplx else 8))) if chunked else max(1, nseed)
    for q0 in range(0, nseed, step):
        rows = range(q0, min(q0 + step, nseed))
        buf, n2 = make(rows)
        keep = [q for q, v in enumerate(n2) if v != 0.0]
        if not keep:
            continue
        stacked = buf if len(keep) == len(rows) else buf[torch.tensor(keep, device=buf.device)]
        # the library reads the seeds on the sector's own (non-blocking) stream:
        # what torch's stream still does to them must be complete first
        torch.cuda.current_stream(stacked.device).synchronize()
        a, b, nl = _tridiag_batch(S, stacked, nlanc, not cplx, threshold, lockstep)
        for row, q in enumerate(keep):
            E, z = tridiag_poles(a[row], b[row], nlanc, first_row=True)
            yield q0 + q, float(n2[q]), a[row], b[row], int(nl[row]), E, z


def _run_jobs_batched(cfg, states, gopt, jobs, todo, device, poles, zeta, record=None):
    """The seed loop grouped by (target sector, vector type): each group's
    seeds are built on the device and tridiagonalised in one batched launch;
    the poles are queued in job order (the serial loop's sequence of
    additions)."""
    import torch

    torch.cuda.set_device(device)
    cache = _SectorCache(cfg, gopt, device)
    groups = {}
    for n in todo:
        p = states.partner(jobs[n].k)
        vec = states.vectors[jobs[n].k if p is None else p]    # a twin's vector has its partner's type
        if vec is None:
            raise ValueError("the Green's function needs the state vectors (keep_vectors=True)")
        cplx = (not cfg.is_real()) or is_complex_vector(vec) or any(np.imag(t[1]) != 0 for t in jobs[n].seed.terms)
        groups.setdefault((jobs[n].dst.q1, jobs[n].dst.q2, cplx), []).append(n)
    fracs = {}
    try:
        for (_, _, cplx), members in groups.items():
            HJ = cache.get(jobs[members[0]].dst, True)
            held = {}                                  # row of the group -> job

            def make(rows):
                chunk = [members[i] for i in rows]
                if gopt.fused_seeds:
                    order, buf, n2 = _fused_seeds(cfg, states, jobs, chunk, cache, cplx, cfg.ed_mode == "superc")
                else:
                    order = chunk
                    made = [_seed(cache.get(jobs[n].src, False), HJ, jobs[n].seed.op, jobs[n].seed.terms,
                                  _state_vec(cfg, states, jobs[n].k, cache), cplx) for n in chunk]
                    buf, n2 = torch.stack([y for y, _ in made]).contiguous(), [v for _, v in made]
                held.update(zip(rows, order))
                return buf, n2

            nlanc = min(HJ.dim, gopt.lanc_nGFiter)
            # only the fused seeds are chunked: the others exist one by one before they are stacked
            for i, norm2, a, b, nl, E, z in seed_fractions(HJ, make, len(members), cplx, nlanc, gopt.threshold,
                                                           chunked=gopt.fused_seeds, lockstep=gopt.lockstep):
                n = held[i]
                job = jobs[n]
                if record is not None:
                    record.append((n, dict(channel=job.tag, isector=states.sectors[job.k], op=job.seed.op,
                                           norm2=norm2, alfa=a, beta=b, nlanc=nl)))
                fracs[n] = (job.comp, _peso(cfg)(states, job.k, job.seed.weight, norm2, zeta),
                            states.energies[job.k], E, z, job.seed.isign)
    finally:
        cache.close()
    for n in todo:
        if n in fracs:
            poles.add(*fracs[n])


def _run_jobs_threaded(cfg, states, gopt, jobs, todo, device, poles, zeta):
    """The seed loop on `gopt.workers` host threads (one sector cache per
    thread); each job's poles are queued in job order afterwards — the same
    sequence of additions as the serial loop."""
    import threading
    from concurrent.futures import ThreadPoolExecutor

    import torch

    local = threading.local()
    caches, lock = [], threading.Lock()

    def init():
        torch.cuda.set_device(device)   # the current device is per thread
        local.cache = _SectorCache(cfg, gopt, device)
        with lock:
            caches.append(local.cache)

    class _Rec:
        def __init__(self):
            self.q = []

        def add(self, *a):
            self.q.append(a)

    def work(n):
        r = _Rec()
        _run_job(cfg, states, gopt, jobs[n], local.cache, r, None, zeta)
        return r.q

    order = sorted(todo, key=lambda n: -jobs[n].dst.dim)   # longest first
    try:
        with ThreadPoolExecutor(max_workers=min(gopt.workers, len(todo)), initializer=init) as ex:
            futs = {n: ex.submit(work, n) for n in order}
            for n in todo:
                for fr in futs[n].result():
                    poles.add(*fr)
    finally:
        for c in caches:
            c.close()


def _dist():
    try:
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _with_broadcast_vectors(cfg, states, owners, device):
    """The state list with every ordinary entry's vector on this rank
    (farm_diag keeps them on their owner; a twin entry is rebuilt from its
    partner on every rank)."""
    dist = _dist()
    if not dist or owners is None:
        return states
    from .farm import broadcast_vector

    vecs = list(states.vectors)
    for k, isec in enumerate(states.sectors):
        if states.partner(k) is not None:     # a twin entry: every rank rebuilds it from the partner
            continue
        dim = setup_pointers(cfg)[isec - 1].dim
        cplx = not cfg.is_real() or is_complex_vector(vecs[k])
        flag = [cplx]
        dist.broadcast_object_list(flag, src=owners[k])
        vecs[k] = broadcast_vector(vecs[k], owners[k], dim, flag[0], device)
    return states.with_vectors(vecs)


def _sum_jobs(cfg, states, gopt, jobs, Gm, Gr, device, record, runner, who: str, ncomp: Optional[int] = None):
    """Run this rank's share of `jobs` and add every continued fraction into
    the host arrays Gm, Gr (indexed by a job's component), summed over the
    ranks of the process group: the part of build_gf and build_gf_superc
    between the job list and the recombination.  ncomp: the arrays are
    (ncomp, L) and a component is a flat index."""
    wm = matsubara(gopt.beta, gopt.Lmats)
    wr = realaxis(gopt.wini, gopt.wfin, gopt.Lreal)
    dist = _dist()
    rank = dist.get_rank() if dist else 0
    world = dist.get_world_size() if dist else 1
    if world > 1:
        from .farm import lpt_partition

        costs = [float(min(j.dst.dim, gopt.lanc_nGFiter)) * j.dst.dim for j in jobs]
        mine = set(lpt_partition(costs, world)[rank])
    else:
        mine = set(range(len(jobs)))
    if states.finite_t and gopt.beta != states.beta:
        raise ValueError(f"{who}: GFOptions.beta = {gopt.beta} but the state list was weighted at "
                         f"beta = {states.beta}")
    # zeta_function (ED_DIAG.f90:403-412): sum of exp(-beta (Ei - Egs)), state_list%size at T=0
    zeta = states.zeta if states.finite_t else float(states.size)
    todo = [n for n in range(len(jobs)) if n in mine]
    poles = PoleSums(cfg.Nspin, cfg.Norb, wm, wr, gopt.eps, device, ncomp) if runner is None else None
    if runner is None and gopt.batch:
        rec = [] if record is not None else None
        _run_jobs_batched(cfg, states, gopt, jobs, todo, device, poles, zeta, rec)
        if record is not None:
            record.extend(r for _, r in sorted(rec, key=lambda t: t[0]))
    elif runner is None and record is None and gopt.workers > 1 and len(todo) > 1:
        _run_jobs_threaded(cfg, states, gopt, jobs, todo, device, poles, zeta)
    else:
        cache = _SectorCache(cfg, gopt, device)
        try:
            for n in todo:
                job = jobs[n]
                if runner is None:
                    _run_job(cfg, states, gopt, job, cache, poles, record, zeta)
                else:
                    runner(cfg, states, gopt, job, wm, wr, Gm[job.comp], Gr[job.comp], zeta)
        finally:
            cache.close()
    if poles is not None:
        poles.flush()
    if world > 1:
        import torch

        if poles is not None and dist.get_backend() == "nccl":
            for t in (poles.Gm, poles.Gr):            # device G, summed over ranks in HBM
                dist.all_reduce(torch.view_as_real(t))
        elif poles is not None:
            for t in (poles.Gm, poles.Gr):
                h = torch.view_as_real(t).cpu()
                dist.all_reduce(h)
                torch.view_as_real(t).copy_(h)
        else:
            for G in (Gm, Gr):
                t = torch.view_as_real(torch.from_numpy(G))   # (re, im) pairs: plain f64 sum
                dist.all_reduce(t)
                G[...] = torch.view_as_complex(t).numpy()
    if poles is not None:
        poles.to_host(Gm, Gr)


def build_gf(cfg: EDConfig, states: StateList, gopt: Optional[GFOptions] = None, device: int = 0,
             record: Optional[list] = None, owners: Optional[List[int]] = None, runner=None):
    """impGmats, impGreal (Nspin, Nspin, Norb, Norb, L) for ed_mode normal
    (build_gf_normal, ED_GF_NORMAL.f90:18-92) and nonsu2 (build_gf_nonsu2,
    ED_GF_NONSU2.f90:18-333, bath_type normal/hybrid: diagonal components plus
    the spin-off-diagonal ones from the mixed seeds and the 0.5*(G - (1+i)G_ii -
    (1+i)G_jj) recombination).

    Normal mode: the orbital-diagonal G[s,s,a,a] for every bath; for hybrid and
    replica baths (`orbital_pairs`, gopt.orbital_mix) also G[s,s,a,b], a < b,
    from the four seeds (c+_a + c+_b), (c_a + c_b), (c+_a + i c+_b),
    (c_a - i c_b)|gs> of lanc_build_gf_normal_mix_c (ED_GF_NORMAL.f90:279-553;
    the last two weighted -i*norm2) and, after the all-reduce,
      G_ab = 0.5*(G_ab - (1-i) G_aa - (1-i) G_bb),   G_ba = G_ab
    (ED_GF_NORMAL.f90:61-68).  The copy into G_ba is the reference's choice
    and is reproduced as it stands: its own comment says the relation holds
    for a real impHloc_ab only; for a complex one G_ba is NOT the true
    <c_b (z-H)^-1 c+_a>.  With orbital_mix=False only the diagonal is built;
    its entries are bit-identical in both settings (the diagonal jobs come
    first and every component accumulates on its own).

    Seed farm: with a process group initialised, the (component, state, seed)
    jobs are split over ranks (longest first by target dimension), each rank
    sums its poles into its own G, and one all_reduce adds the G arrays
    (2 x L complex numbers per component — no collective inside a job).  State
    vectors missing on a rank (farm_diag keeps them on their owner) are
    broadcast from `owners` first.  A finite-temperature list (states.finite_t)
    weights every state by exp(-beta (Ei - Egs)) / zeta (ED_GF_NORMAL.f90:596-601)
    and needs gopt.beta == states.beta; twin entries take their vector from
    `state_vector`.  `runner(cfg, states, gopt, job, wm, wr,
    G_m, G_r, zeta)` replaces the device job (the CPU tests pass the oracle's)."""
    gopt = gopt or GFOptions()
    if cfg.ed_mode == "superc":
        raise NotImplementedError("build_gf returns (Gmats, Greal) only: the superc Green's function "
                                  "(ED_GF_SUPERC, G and the anomalous F) is build_gf_superc")
    No, Nsp = cfg.Norb, cfg.Nspin
    Gm = np.zeros((Nsp, Nsp, No, No, gopt.Lmats), dtype=np.complex128)
    Gr = np.zeros((Nsp, Nsp, No, No, gopt.Lreal), dtype=np.complex128)
    states = _with_broadcast_vectors(cfg, states, owners, device)
    jobs, pairs = _job_list(cfg, states, gopt.orbital_mix)
    opairs = orbital_pairs(cfg) if gopt.orbital_mix else []
    _sum_jobs(cfg, states, gopt, jobs, Gm, Gr, device, record, runner, "build_gf")
    for ispin, jspin, iorb in pairs:               # build_gf_nonsu2 :35-48
        for G in (Gm, Gr):
            G[ispin, jspin, iorb, iorb] = 0.5 * (G[ispin, jspin, iorb, iorb]
                                                 - (1 + 1j) * G[ispin, ispin, iorb, iorb]
                                                 - (1 + 1j) * G[jspin, jspin, iorb, iorb])
    for s, a, b in opairs:                         # build_gf_normal, ED_GF_NORMAL.f90:61-68
        for G in (Gm, Gr):
            G[s, s, a, b] = 0.5 * (G[s, s, a, b] - (1 - 1j) * G[s, s, a, a] - (1 - 1j) * G[s, s, b, b])
            G[s, s, b, a] = G[s, s, a, b]
    return Gm, Gr


def build_gf_normal(cfg: EDConfig, states: StateList, gopt: Optional[GFOptions] = None,
                    device: int = 0, record: Optional[list] = None):
    """build_gf_normal (ED_GF_NORMAL.f90:18-92).  A record entry of a diagonal
    channel ("diag", ispin, iorb) gets ispin, iorb and jorb = iorb; one of an
    orbital-mixed channel ("orbmix", ispin, iorb, jorb) its own jorb."""
    if cfg.ed_mode != "normal":
        raise ValueError("build_gf_normal needs ed_mode='normal'")
    rec = [] if record is not None else None
    Gm, Gr = build_gf(cfg, states, gopt, device, rec)
    if record is not None:
        for r in rec:
            ch = r["channel"]
            record.append(dict(r, ispin=ch[1], iorb=ch[2], jorb=ch[3] if ch[0] == "orbmix" else ch[2]))
    return Gm, Gr


def build_gf_superc(cfg: EDConfig, states: StateList, gopt: Optional[GFOptions] = None, device: int = 0,
                    record: Optional[list] = None, owners: Optional[List[int]] = None, runner=None):
    """impGmats, impGreal, impFmats, impFreal, each (1, 1, Norb, Norb, L), for
    ed_mode superc: build_gf_superc / lanc_build_gf_superc_c /
    add_to_lanczos_gf_superc (ED_GF_SUPERC.f90:18-77, 88-446, 757-803).

    Per orbital a and kept state |n> six seeds go into three aux channels
    (`_job_list_superc`): G_aa from c+_{a,up}|n> and c_{a,up}|n>, barG_aa
    from c_{a,dw}|n> and c+_{a,dw}|n>, A_aa from (c+_{a,up} + c_{a,dw})|n> and
    (c_{a,up} + c+_{a,dw})|n>; the first of each pair lives in sector sz+1 with
    isign +1, the second in sz-1 with isign -1.  The weight is `_peso_superc`
    (no beta dE < 200 cut, unlike the normal mode).  After the all-reduce over
    the aux arrays (ED_GF_SUPERC.f90:39-44)
      G[0,0,a,a] = G_aa,   F[0,0,a,a] = 0.5 * (A_aa - G_aa - barG_aa).

    Orbital off-diagonal entries [0,0,a,b], a != b, stay zero, also for a
    hybrid bath: the reference's pair loop (lanc_build_gf_superc_mix_c,
    ED_GF_SUPERC.f90:455-738) accumulates on aux arrays it does not zero
    between pairs (ED_GF_SUPERC.f90:31-33 is the only reset, ED_GF_SUPERC.f90:55-65 the pair loop), stores that raw
    sum as impGmats(a,b) and never fills (b,a), so there is no sound value to
    reproduce.

    The host paths (serial, threaded, batched, gopt.fused_seeds with
    ed_sector_seed_plan), the rank split, `owners`, `record`, finite-temperature
    and twin lists and `runner` are build_gf's; a record entry's channel is
    ("superc", aux channel 0..2, iorb)."""
    gopt = gopt or GFOptions()
    if cfg.ed_mode != "superc":
        raise ValueError("build_gf_superc needs ed_mode='superc'")
    No = cfg.Norb
    aux_m = np.zeros((SUPERC_CHANNELS * No, gopt.Lmats), dtype=np.complex128)
    aux_r = np.zeros((SUPERC_CHANNELS * No, gopt.Lreal), dtype=np.complex128)
    states = _with_broadcast_vectors(cfg, states, owners, device)
    jobs = _job_list_superc(cfg, states)
    _sum_jobs(cfg, states, gopt, jobs, aux_m, aux_r, device, record, runner, "build_gf_superc",
              ncomp=SUPERC_CHANNELS * No)
    out = []
    for aux in (aux_m, aux_r):
        G = np.zeros((1, 1, No, No, aux.shape[1]), dtype=np.complex128)
        F = np.zeros_like(G)
        for a in range(No):
            g, gbar, A = aux[SUPERC_CHANNELS * a:SUPERC_CHANNELS * (a + 1)]
            G[0, 0, a, a] = g
            F[0, 0, a, a] = 0.5 * (A - g - gbar)
        out.append((G, F))
    (Gm, Fm), (Gr, Fr) = out
    return Gm, Gr, Fm, Fr
