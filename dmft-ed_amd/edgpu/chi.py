"""Spin and density susceptibilities of the kept states by Lanczos, on device.

Mirrors buildChi_impurity (ED_GREENS_FUNCTIONS.f90:72-106) for build_chi_spin
(ED_GF_CHISPIN.f90:22-40) and build_chi_dens (ED_GF_CHIDENS.f90:21-66) with
the four departures of DESIGN.md section 12.  For a Hermitian operator O
diagonal in the Fock basis, kept states n of weight w_n (`StateList.weights`
over zeta, 1/size at T = 0), m over the eigenstates of n's sector and
D = E_m - E_n:

  tau_i : sum_n w_n sum_m |<m|O|n>|^2 [exp(-tau_i D) + exp(-(beta - tau_i) D)]
  iv_0  : sum_n w_n sum_m |<m|O|n>|^2 2 s(D),  s(D) = (1 - exp(-beta D)) / D, s(0) = beta
  iv_i  : sum_n w_n sum_m |<m|O|n>|^2 (1 - exp(-beta D)) [1/(i v_i + D) - 1/(i v_i - D)]
  w_i   : the same with i v_i -> wr_i + i eps

Per kept state |n> (a twin entry's vector through `state_vector`):

  * every seed O_q|n> of the table (`seed_table`) from one
    ed_sector_seed_diag call (k_seed_diag, csrc/ed_chi.hpp), written straight
    into the stacked tensor; norm2_q = <seed|seed>; seeds with norm2 == 0 are
    dropped;
  * one ed_sector_lanc_tridiag_batch launch on |n>'s own sector,
    nlanc = min(dim, lanc_nGFiter);
  * poles by `ed_tridiag_poles`, |<m|O|n>|^2 = norm2 Z(1,j)^2, queued in the
    order (kept state, seed) and summed by one ed_chi_add_poles launch
    (k_chi_poles) into arrays that stay in HBM.

The off-diagonal density comes from the seeds n_a + n_b:
chi[a,b] = chi[b,a] = (chi[n_a + n_b] - chi[n_a] - chi[n_b]) / 2 on all three
grids, exact because the n_a commute and are real.

With `pair` / `exc` the pair susceptibility of
Delta_a = c_{a,up} c_{a,dw} (ED_GF_CHIPAIR.f90) and the inter-orbital density
susceptibility of O_ab = sum_sigma c^+_{a,sigma} c_{b,sigma}
(lanc_ed_build_densChi_mix_c, ED_GF_CHIDENS.f90:490-673) are built as well:
chi_O(tau) = <O(tau) O^+(0)> of a non-Hermitian O is two one-sign fractions,
the seed O^+|n> with isign = +1 and the seed O|n> with isign = -1 (the two
branches above, one each).  Per kept state one ed_sector_seed_pair call
(k_seed_pair) per target sector — every Delta_a|n> into (nup-1, ndw-1), every
Delta_a^+|n> into (nup+1, ndw+1), every O_ab^+|n> into the state's own — writes
straight into the stacked tensor of one batched Lanczos launch on that sector;
O_ba = O_ab^+, so each inter-orbital tridiagonalisation is queued twice, with
+1 into [a,b] and with -1 into [b,a].
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check
from .diag import StateList, is_complex_vector, state_vector
from .gf import _device_vec, _dist, _peso_bz, _SectorCache, realaxis, seed_fractions
from .params import EDConfig
from .sectors import c_sector, cdg_sector, setup_pointers


@dataclass
class ChiOptions:
    """ED_INPUT_VARS defaults (ED_INPUT_VARS.f90:126-173)."""

    lanc_nGFiter: int = 200
    Lmats: int = 5000
    Lreal: int = 5000
    Ltau: int = 1000
    beta: float = 1000.0
    eps: float = 0.01
    wini: float = -5.0
    wfin: float = 5.0
    threshold: float = 1e-13      # sp_lanc_tridiag breakdown test
    sparse_H: bool = True         # ed_sparse_H
    lockstep: bool = False        # GFOptions.lockstep: the seeds of one sector advance together

    @property
    def ltau(self) -> int:
        """Ltau = max(int(beta), Ltau) (ED_INPUT_VARS.f90:211)."""
        return max(int(self.beta), self.Ltau)


def bosonic_matsubara(beta: float, L: int) -> np.ndarray:
    """vm(0:L) = pi/beta * 2 i (allocate_grids, ED_AUX_FUNX.f90:457)."""
    return np.pi / beta * (2.0 * np.arange(0, L + 1))


def tau_grid(beta: float, L: int) -> np.ndarray:
    """tau(0:L) = linspace(0, beta, L+1) (ED_AUX_FUNX.f90:460)."""
    return np.linspace(0.0, beta, L + 1)


# ------------------------------------------------------------ seeds and components
def seed_levels(cfg: EDConfig) -> List[int]:
    """The impurity levels of one ed_sector_seed_diag call: (orbital a, up) is
    bit a, (orbital a, down) bit a + Ns — ib(iorb), ib(iorb+Ns) of the
    reference's vvinit loops (ED_GF_CHISPIN.f90:98-103)."""
    return list(range(cfg.Norb)) + [a + cfg.Ns for a in range(cfg.Norb)]


def dens_pairs(cfg: EDConfig) -> List[Tuple[int, int]]:
    return [(a, b) for a in range(cfg.Norb) for b in range(a + 1, cfg.Norb)]


def n_components(cfg: EDConfig, pair: bool = False, exc: bool = False) -> int:
    """Flat components: spin a (Norb), spin total, density a (Norb), density
    pair sums n_a + n_b (a < b), density total; behind them, with `pair`, Norb
    pair components and, with `exc`, the Norb x Norb block of inter-orbital
    ones (its diagonal is never written)."""
    No = cfg.Norb
    return 2 * No + 2 + len(dens_pairs(cfg)) + (No if pair else 0) + (No * No if exc else 0)


def seed_table(cfg: EDConfig, spin: bool = True, dens: bool = True):
    """The seeds of one kept state in the order their fractions are queued:
    a list of (name, flat component, weights over `seed_levels`).

      ("spin", a)         (n_a,up - n_a,dw) / 2     ED_GF_CHISPIN.f90:61-141
      ("spin_tot",)       sum_a of those            ED_GF_CHISPIN.f90:158-237   Norb > 1
      ("dens", a)         n_a,up + n_a,dw           ED_GF_CHIDENS.f90:90-169
      ("dens_pair", a, b) n_a + n_b, a < b          ED_GF_CHIDENS.f90:291-468   Norb > 1
      ("dens_tot",)       sum_a n_a                 ED_GF_CHIDENS.f90:191-269   Norb > 1
    """
    No = cfg.Norb
    up, dw = (lambda a: a), (lambda a: No + a)      # positions in seed_levels
    out = []

    def row(name, comp, terms):
        w = np.zeros(2 * No)
        for pos, c in terms:
            w[pos] = c
        out.append((name, comp, w))

    if spin:
        for a in range(No):
            row(("spin", a), a, [(up(a), 0.5), (dw(a), -0.5)])
        if No > 1:
            row(("spin_tot",), No, [(up(a), 0.5) for a in range(No)] + [(dw(a), -0.5) for a in range(No)])
    if dens:
        d0 = No + 1
        for a in range(No):
            row(("dens", a), d0 + a, [(up(a), 1.0), (dw(a), 1.0)])
        if No > 1:
            for p, (a, b) in enumerate(dens_pairs(cfg)):
                row(("dens_pair", a, b), d0 + No + p, [(up(a), 1.0), (dw(a), 1.0), (up(b), 1.0), (dw(b), 1.0)])
            row(("dens_tot",), d0 + No + len(dens_pairs(cfg)), [(up(a), 1.0) for a in range(No)]
                + [(dw(a), 1.0) for a in range(No)])
    return out


def chi_jobs(cfg: EDConfig, states: StateList, spin: bool = True, dens: bool = True):
    """(kept state k, seed index in the table, name, component) of every
    fraction in queue order: kept state in `states.sectors` order, then seed."""
    table = seed_table(cfg, spin, dens)
    return [(k, q, name, comp) for k in range(states.size) for q, (name, comp, _) in enumerate(table)]


@dataclass
class Chi:
    """spin_*: leading shape (Norb+1,), row Norb the total (zero for Norb = 1);
    dens_*: (Norb, Norb), symmetric; dens_tot_*: the total density (zero for
    Norb = 1, where the reference builds no total seed either).  *_iv:
    complex (.., Lmats+1) on `vm`; *_tau: real (.., Ltau+1) on `tau`; *_w:
    complex (.., Lreal) on `wr`.  A part that was not requested is None."""

    vm: np.ndarray
    tau: np.ndarray
    wr: np.ndarray
    spin_iv: Optional[np.ndarray] = None
    spin_tau: Optional[np.ndarray] = None
    spin_w: Optional[np.ndarray] = None
    dens_iv: Optional[np.ndarray] = None
    dens_tau: Optional[np.ndarray] = None
    dens_w: Optional[np.ndarray] = None
    dens_tot_iv: Optional[np.ndarray] = None
    dens_tot_tau: Optional[np.ndarray] = None
    dens_tot_w: Optional[np.ndarray] = None
    # pair_*: (Norb,), chi of Delta_a = c_{a,up} c_{a,dw}; exc_*: (Norb, Norb), chi of
    # O_ab = sum_sigma c^+_{a,sigma} c_{b,sigma}, zero on the diagonal
    pair_iv: Optional[np.ndarray] = None
    pair_tau: Optional[np.ndarray] = None
    pair_w: Optional[np.ndarray] = None
    exc_iv: Optional[np.ndarray] = None
    exc_tau: Optional[np.ndarray] = None
    exc_w: Optional[np.ndarray] = None


def assemble(cfg: EDConfig, copt: ChiOptions, iv: np.ndarray, tau: np.ndarray, w: np.ndarray,
             spin: bool = True, dens: bool = True, pair: bool = False, exc: bool = False) -> Chi:
    """The flat component arrays (n_components, L) as a `Chi`: the spin rows as
    they are; the density diagonal from the n_a seeds, the off-diagonal from
    the pair sums, chi[a,b] = chi[b,a] = (chi[n_a+n_b] - chi[n_a] - chi[n_b]) / 2;
    the pair rows and the inter-orbital block of the components behind them."""
    No = cfg.Norb
    out = Chi(bosonic_matsubara(copt.beta, copt.Lmats), tau_grid(copt.beta, copt.ltau),
              realaxis(copt.wini, copt.wfin, copt.Lreal))
    if spin:
        out.spin_iv, out.spin_tau, out.spin_w = (np.array(x[:No + 1]) for x in (iv, tau, w))
    if dens:
        d0 = No + 1
        res = []
        for x in (iv, tau, w):
            m = np.zeros((No, No) + x.shape[1:], dtype=x.dtype)
            for a in range(No):
                m[a, a] = x[d0 + a]
            for p, (a, b) in enumerate(dens_pairs(cfg)):
                m[a, b] = 0.5 * (x[d0 + No + p] - x[d0 + a] - x[d0 + b])
                m[b, a] = m[a, b]
            # the total seed is built for Norb > 1 only (ED_GF_CHIDENS.f90:32-60): zero otherwise
            res.append((m, np.array(x[d0 + No + len(dens_pairs(cfg))])))
        (out.dens_iv, out.dens_tot_iv), (out.dens_tau, out.dens_tot_tau), (out.dens_w, out.dens_tot_w) = res
    if pair:
        p0 = pair_component(cfg, 0)
        out.pair_iv, out.pair_tau, out.pair_w = (np.array(x[p0:p0 + No]) for x in (iv, tau, w))
    if exc:
        e0 = exc_component(cfg, 0, 0, pair)
        out.exc_iv, out.exc_tau, out.exc_w = (np.array(x[e0:e0 + No * No]).reshape((No, No) + x.shape[1:])
                                              for x in (iv, tau, w))
    return out


# ------------------------------------------------------------ pair and inter-orbital parts
n_components_ext, assemble_ext = n_components, assemble      # aliases: tests/test_chi_pair_cpu.py calls these names


def pair_component(cfg: EDConfig, a: int) -> int:
    return n_components(cfg) + a


def exc_component(cfg: EDConfig, a: int, b: int, pair: bool = False) -> int:
    return n_components(cfg) + (cfg.Norb if pair else 0) + a * cfg.Norb + b


def exc_pairs(cfg: EDConfig) -> List[Tuple[int, int]]:
    """Ordered pairs a != b: one seed O_ab^+|n> each."""
    return [(a, b) for a in range(cfg.Norb) for b in range(cfg.Norb) if a != b]


def pair_target(cfg: EDConfig, sec, isign: int):
    """The sector of Delta_a|n> (isign -1: one up and one down electron fewer)
    or Delta_a^+|n> (+1); None where it does not exist."""
    step = cdg_sector if isign > 0 else c_sector
    mid = step(cfg, sec, 1)
    return None if mid is None else step(cfg, mid, 0)


def seed_pair_calls(cfg: EDConfig, pair: bool = False, exc: bool = False):
    """The ed_sector_seed_pair calls of one kept state in queue order: a list
    of (target, images, terms, queue).  target: -1 / +1 the pair target sector
    of that sign, 0 the kept state's own; images: rows (lev1, op1, lev2, op2),
    (lev1, op1) acting first; terms: rows (p, q); queue[s]: the fractions of
    seed s as (name, flat component, isign).

      ("pair", a) -1   c_{a,up} c_{a,dw}|n>              ED_GF_CHIPAIR.f90:98-102
      ("pair", a) +1   c^+_{a,dw} c^+_{a,up}|n>          ED_GF_CHIPAIR.f90:144-148
      ("exc", a, b) +1 and ("exc", b, a) -1, one seed
                       sum_sigma c^+_{b,sigma} c_{a,sigma}|n>
                                                          ED_GF_CHIDENS.f90:523-586, :596-659
    """
    No, Ns = cfg.Norb, cfg.Ns
    out = []
    if pair:
        one = [(a, -1) for a in range(No)]
        out.append((-1, [(a + Ns, 0, a, 0) for a in range(No)], one,
                    [[(("pair", a), pair_component(cfg, a), -1)] for a in range(No)]))
        out.append((+1, [(a, 1, a + Ns, 1) for a in range(No)], one,
                    [[(("pair", a), pair_component(cfg, a), +1)] for a in range(No)]))
    if exc and No > 1:
        images, terms, queue = [], [], []
        for a, b in exc_pairs(cfg):
            terms.append((len(images), len(images) + 1))
            images += [(a, 0, b, 1), (a + Ns, 0, b + Ns, 1)]
            queue.append([(("exc", a, b), exc_component(cfg, a, b, pair), +1),
                          (("exc", b, a), exc_component(cfg, b, a, pair), -1)])
        out.append((0, images, terms, queue))
    return out


# ------------------------------------------------------------ the pole sums
class ChiPoleSums:
    """Device side of add_to_lanczos_spinChi (ED_GF_CHISPIN.f90:254-323), the
    counterpart of gf.PoleSums: the three grids are uploaded once, the arrays
    iv (ncomp, Lmats+1) complex, tau (ncomp, Ltau+1) real and w (ncomp, Lreal)
    complex live in HBM, `add` queues one tridiagonalisation's poles for a
    flat component and `flush` sums every queued fraction in one launch of
    ed_chi_add_poles_signed, in queue order (within a fraction every pole with
    isign = +1, then every pole with -1; a fraction added with isign = +-1
    takes that branch alone)."""

    def __init__(self, ncomp: int, vm: np.ndarray, tau: np.ndarray, wr: np.ndarray, beta: float, eps: float,
                 device: int):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("the susceptibility pole sum runs on the GPU (no host fallback)")
        self.dev = torch.device("cuda", device)
        self.ncomp, self.beta, self.eps = ncomp, float(beta), float(eps)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)   # noqa: E731
        self.vm, self.tg, self.wr = up(vm), up(tau), up(wr)
        self.iv = torch.zeros((ncomp, len(vm)), dtype=torch.complex128, device=self.dev)
        self.tau = torch.zeros((ncomp, len(tau)), dtype=torch.float64, device=self.dev)
        self.w = torch.zeros((ncomp, len(wr)), dtype=torch.complex128, device=self.dev)
        self._q = []

    def add(self, comp: int, peso: float, Ei: float, E: np.ndarray, z: np.ndarray, isign: int = 0) -> None:
        assert 0 <= int(comp) < self.ncomp and int(isign) in (0, 1, -1)
        self._q.append((int(comp), float(peso), float(Ei), np.asarray(E, np.float64), np.asarray(z, np.float64),
                        int(isign)))

    def flush(self) -> None:
        import torch

        if not self._q:
            return
        q, self._q = self._q, []
        npole = np.array([len(t[3]) for t in q], dtype=np.int32)
        E = np.ascontiguousarray(np.concatenate([t[3] for t in q]))
        z = np.ascontiguousarray(np.concatenate([t[4] for t in q]))
        peso = np.array([t[1] for t in q], dtype=np.float64)
        ei = np.array([t[2] for t in q], dtype=np.float64)
        comp = np.array([t[0] for t in q], dtype=np.int32)
        isign = np.array([t[5] for t in q], dtype=np.int32)
        st = torch.cuda.current_stream(self.dev)
        P = ctypes.c_void_p
        check(_lib.load().ed_chi_add_poles_signed(
            len(q), P(npole.ctypes.data), P(E.ctypes.data), P(z.ctypes.data), P(peso.ctypes.data), P(ei.ctypes.data),
            P(comp.ctypes.data), P(isign.ctypes.data), self.beta, P(self.vm.data_ptr()), self.vm.numel() - 1,
            P(self.tg.data_ptr()), self.tg.numel() - 1, P(self.wr.data_ptr()), self.wr.numel(), self.eps,
            P(self.iv.data_ptr()), P(self.tau.data_ptr()), P(self.w.data_ptr()), P(st.cuda_stream)),
            "ed_chi_add_poles_signed")

    def to_host(self):
        return self.iv.cpu().numpy(), self.tau.cpu().numpy(), self.w.cpu().numpy()


# ------------------------------------------------------------ the build
def _check(cfg: EDConfig, states: StateList, copt: ChiOptions, pair: bool = False, exc: bool = False) -> None:
    if (pair or exc) and cfg.ed_mode == "nonsu2" and cfg.Jz_basis:
        raise NotImplementedError("build_chi: " + " and ".join(n for n, on in (("pair", pair), ("exc", exc)) if on)
                                  + " in the Jz_basis is not built: the seeds of one call reach different "
                                  "(n, twoJz) sectors")
    if cfg.ed_mode == "superc":
        raise NotImplementedError("build_chi: ed_mode='superc' is not built: a superc twin vector needs "
                                  "superc_twin_sign and no susceptibility test covers it")
    dist = _dist()
    if dist and dist.get_world_size() > 1:
        raise NotImplementedError("build_chi: no rank split of the susceptibility jobs is built "
                                  f"(torch.distributed world size {dist.get_world_size()})")
    if states.finite_t and copt.beta != states.beta:
        raise ValueError(f"build_chi: ChiOptions.beta = {copt.beta} but the state list was weighted at "
                         f"beta = {states.beta}")


def build_chi(cfg: EDConfig, states: StateList, copt: Optional[ChiOptions] = None, device: int = 0,
              spin: bool = True, dens: bool = True, record: Optional[list] = None, pair: bool = False,
              exc: bool = False) -> Chi:
    """spinChi and densChi of buildChi_impurity (ED_GREENS_FUNCTIONS.f90:72-106)
    on the three grids and, with `pair` / `exc`, its pair and inter-orbital
    density parts, as a `Chi`; see the module docstring.  `record` gets one
    dict per fraction (name, component, kept state, isector, norm2, alfa,
    beta, nlanc, isign) in queue order: per kept state the spin and density
    seeds, the pair -1 seeds by orbital, the pair +1 seeds, the inter-orbital
    seeds (each queued with +1 and then -1).  Refused: ed_mode superc, a
    torch.distributed world larger than 1, and pair / exc in the Jz_basis."""
    import torch

    copt = copt or ChiOptions()
    _check(cfg, states, copt, pair, exc)
    table = seed_table(cfg, spin, dens)
    calls = seed_pair_calls(cfg, pair, exc)
    vm, tg = bosonic_matsubara(copt.beta, copt.Lmats), tau_grid(copt.beta, copt.ltau)
    wr = realaxis(copt.wini, copt.wfin, copt.Lreal)
    poles = ChiPoleSums(n_components(cfg, pair, exc), vm, tg, wr, copt.beta, copt.eps, device)
    zeta = states.zeta if states.finite_t else float(states.size)
    levels = seed_levels(cfg)
    secs = setup_pointers(cfg)
    torch.cuda.set_device(device)
    cache = _SectorCache(cfg, copt, device)
    try:
        for k, isec in enumerate(states.sectors if table or calls else []):
            sec = secs[isec - 1]
            vec = state_vector(cfg, states, k, device, lambda s: cache.get(s, False))
            if vec is None:
                raise ValueError("the susceptibilities need the state vectors (keep_vectors=True)")
            cplx = (not cfg.is_real()) or is_complex_vector(vec)
            S = cache.get(sec, True)
            x = _device_vec(vec, cplx, device)

            def run(St, make, queue):
                """The seeds make(rows) of sector St; queue[s]: the fractions of seed s as (name, comp, isign)."""
                for s, norm2, a, b, nl, E, z in seed_fractions(St, make, len(queue), cplx,
                                                               min(St.dim, copt.lanc_nGFiter), copt.threshold,
                                                               lockstep=copt.lockstep):
                    for name, comp, isign in queue[s]:
                        if record is not None:
                            record.append(dict(name=name, comp=comp, state=k, isector=isec, norm2=norm2, alfa=a,
                                               beta=b, nlanc=nl, isign=isign))
                        poles.add(comp, _peso_bz(states, k, 1.0, norm2, zeta), states.energies[k], E, z, isign)

            run(S, lambda rows: S.seed_diag(x, levels, np.array([table[q][2] for q in rows])),
                [[(name, comp, 0)] for name, comp, _ in table])
            for target, images, terms, queue in calls:
                tsec = sec if target == 0 else pair_target(cfg, sec, target)
                if tsec is None:                                          # no such sector: no seed
                    continue
                St = cache.get(tsec, True)
                run(St, lambda rows: S.seed_pair(x, St, images, [terms[q] for q in rows]), queue)
    finally:
        cache.close()
    poles.flush()
    return assemble(cfg, copt, *poles.to_host(), spin=spin, dens=dens, pair=pair, exc=exc)
