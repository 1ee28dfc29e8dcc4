"""Dense truth of the superconducting Green's function tests (test
infrastructure only).

Three ed_mode="superc" models small enough (<= 256 Fock states) for the
full-Fock Jordan-Wigner Hamiltonian of oracle.jw_dense: its blocks by
sz = popcount(up) - popcount(down) give every sector's spectrum and
eigenvectors by numpy.linalg.eigh; no Lanczos and no Nambu seeds.  For state
weights w_n, orbital a, D = E_m - E_n and m over the whole spectrum of the
target block:

  G(z) = sum_n w_n sum_m [ |<m|c+_{a,up}|n>|^2 / (z - D) + |<m|c_{a,up}|n>|^2 / (z + D) ]
  F(z) = 1/2 sum_n w_n sum_m [
           (<n|c_{a,up}|m><m|c_{a,dw}|n> + <n|c+_{a,dw}|m><m|c+_{a,up}|n>) / (z - D)
         + (<n|c+_{a,up}|m><m|c+_{a,dw}|n> + <n|c_{a,dw}|m><m|c_{a,up}|n>) / (z + D) ]

F is the cross terms of |<m|psi|n>|^2 written out directly, not the
1/2 (A - G - barG) recombination of build_gf_superc (ED_GF_SUPERC.f90:39-44)
that the code under test runs.  barG (the c_dw / c+_dw channel) is returned
too, so that a test can show G != barG.

  S1  Norb=1, Nbath=2, deltasc=0.3, random bath, xmu=0.2: Ns=3, 64 Fock
      states, sector dims 1..20; the end sectors sz = +-3 have one target only.
  S2  Norb=2, Nbath=1, normal bath, interactions of cases.superc_2orb: Ns=4,
      256 Fock states, 4 impurity levels, unequal orbitals.
  SH  Norb=2, Nbath=2, hybrid bath: Ns=4, 256 Fock states.

A T = 0 ground state can be degenerate, so `gf_of_list` takes the states and
weights (1/size) from the list under test; `gf_thermal` sums the dense thermal
set {exp(-beta (E - E0)) > cutoff} with w_n = exp(-beta (E_n - E0)) / zeta.
Everything is computed once per model and shared (never modified) by the CPU
and GPU tests.
"""
from functools import lru_cache

import numpy as np

BETA, CUTOFF, NTOTAL = 8.0, 1e-4, 40     # the thermal case (S1)
# Broadening of the real-axis checks, per model: the smallest of 0.01, 0.1,
# 0.2, 0.3, 0.5 at which the CPU oracle-runner replay holds 1e-5 (the table is
# in test_superc_gf_cpu's docstring)
EPS = {"S1": 0.01, "S2": 0.01, "SH": 0.1}


def config(name):
    import cases
    from edgpu.params import make_config

    if name == "S1":
        return make_config(Norb=1, Nbath=2, ed_mode="superc", deltasc=0.3, bath="random", xmu=0.2, seed=8)
    if name == "S2":
        cfg = make_config(Norb=2, Nbath=1, Nspin=1, ed_mode="superc", Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.3, Jx=0.3,
                          Jp=0.3, deltasc=0.3, bath="random", seed=19)
        cfg.impHloc = cases._hloc(1, 2, 20)
        return cfg
    assert name == "SH"
    cfg = make_config(Norb=2, Nbath=2, Nspin=1, ed_mode="superc", bath_type="hybrid", Uloc=(2.0, 1.6, 0.0), Ust=1.0,
                      Jh=0.2, deltasc=0.3, xmu=0.3, bath="random", seed=31)
    cfg.impHloc = cases._hloc(1, 2, 32)
    return cfg


class Truth:
    def __init__(self, name):
        from edgpu.sectors import setup_pointers
        from oracle.jw_dense import _ops, full_hamiltonian

        self.cfg = cfg = config(name)
        Ns = cfg.Ns
        self.H = H = full_hamiltonian(cfg).tocsr()
        self.c = [m.tocsr() for m in _ops(2 * Ns)]
        x = np.arange(1 << (2 * Ns))
        pc = lambda v: np.array([bin(int(t)).count("1") for t in v])   # noqa: E731
        sz = pc(x & ((1 << Ns) - 1)) - pc(x >> Ns)
        self.secs = setup_pointers(cfg)
        self.by_sz = {s.q1: s.isector for s in self.secs}
        self.sz_of = {s.isector: s.q1 for s in self.secs}
        self.maps, self.w, self.v = {}, {}, {}
        for s in self.secs:
            idx = x[sz == s.q1]                              # ascending: the sector's row order
            assert len(idx) == s.dim
            blk = H[idx][:, idx].toarray()
            assert np.max(np.abs(blk - blk.conj().T)) < 1e-14
            w, v = np.linalg.eigh(blk.real if np.max(np.abs(blk.imag)) == 0.0 else blk)
            self.maps[s.isector], self.w[s.isector], self.v[s.isector] = idx, w, v
        self.e0 = min(w[0] for w in self.w.values())

    def sector_results(self, nkeep=6, ed_twin=False):
        """SectorResults with the nkeep lowest dense eigenpairs of every
        sector ed_diag would visit (as finite_t_truth.Truth.sector_results)."""
        from edgpu.diag import SectorResult
        from edgpu.sectors import diag_sectors

        out = []
        for s in diag_sectors(self.cfg, ed_twin):
            n = min(s.dim, nkeep)
            out.append(SectorResult(s.isector, (s.q1, s.q2), s.dim, self.w[s.isector][:n].copy(), n,
                                    self.v[s.isector][:, :n].copy(), "dense"))
        return out

    def thermal_states(self, beta=BETA, cutoff=CUTOFF):
        """(energy, isector, index in the sector's spectrum) of the dense thermal set."""
        return sorted((float(e), i, k) for i, w in self.w.items() for k, e in enumerate(w)
                      if np.exp(-beta * (e - self.e0)) > cutoff)

    def _sum(self, rows, wm, wr, eps):
        """rows: (weight, energy, isector, vector in the sector's row order).
        Returns {"G","Gbar","F"} -> (mats, real), each (Norb, L)."""
        cfg = self.cfg
        Ns, No = cfg.Ns, cfg.Norb
        zs = [1j * np.asarray(wm), np.asarray(wr) + 1j * eps]
        out = {k: [np.zeros((No, len(z)), dtype=np.complex128) for z in zs] for k in ("G", "Gbar", "F")}
        for wt, e, isec, vec in rows:
            psi = np.zeros(self.H.shape[0], dtype=np.complex128)
            psi[self.maps[isec]] = vec
            for sign in (+1, -1):
                j = self.by_sz.get(self.sz_of[isec] + sign)
                if j is None:
                    continue
                de = self.w[j] - e
                proj = lambda op: self.v[j].conj().T @ np.asarray(op @ psi).ravel()[self.maps[j]]   # noqa: E731
                for a in range(No):
                    cu, cd = self.c[a], self.c[a + Ns]
                    # sign +1: U = <m|c+_up|n>, D = <m|c_dw|n>; sign -1: U = <m|c_up|n>, D = <m|c+_dw|n>
                    U, D = (proj(cu.getH()), proj(cd)) if sign > 0 else (proj(cu), proj(cd.getH()))
                    amps = {"G": np.abs(U) ** 2, "Gbar": np.abs(D) ** 2,
                            "F": 0.5 * (np.conj(U) * D + np.conj(D) * U)}
                    for key, amp in amps.items():
                        for g, z in zip(out[key], zs):
                            g[a] += wt * np.sum(amp[None, :] / (z[:, None] - sign * de[None, :]), axis=1)
        return out

    def gf_of_list(self, states, wm, wr, eps):
        """T = 0: the states of the list under test, w_n = 1/size."""
        from edgpu.diag import to_host

        assert not states.finite_t and all(p is None for p in states.twin_of)
        rows = [(1.0 / states.size, e, i, np.asarray(to_host(v))) for e, i, v in
                zip(states.energies, states.sectors, states.vectors)]
        return self._sum(rows, wm, wr, eps)

    def gf_thermal(self, wm, wr, eps, beta=BETA, cutoff=CUTOFF):
        kept = self.thermal_states(beta, cutoff)
        b = np.exp(-beta * (np.array([t[0] for t in kept]) - self.e0))
        rows = [(bk / b.sum(), e, i, self.v[i][:, k]) for (e, i, k), bk in zip(kept, b)]
        return self._sum(rows, wm, wr, eps)


@lru_cache(maxsize=None)
def truth(name) -> Truth:
    return Truth(name)


def distances(T, got, wm, wr, eps):
    """(dm, dr, ratio): max over G and F of |got - truth| / max(|G|, |F|) on
    the two axes, and max|F| / max|G| of the truth on the Matsubara axis.
    got = (Gm, Gr, Fm, Fr) of build_gf_superc; T: a dict of Truth._sum."""
    Gm, Gr, Fm, Fr = got
    No = Gm.shape[2]
    d = []
    for ax, G, F in ((0, Gm, Fm), (1, Gr, Fr)):
        scale = max(np.max(np.abs(T["G"][ax])), np.max(np.abs(T["F"][ax])))
        d.append(max(max(np.max(np.abs(G[0, 0, a, a] - T["G"][ax][a])), np.max(np.abs(F[0, 0, a, a] - T["F"][ax][a])))
                     for a in range(No)) / scale)
    return d[0], d[1], np.max(np.abs(T["F"][0])) / np.max(np.abs(T["G"][0]))
