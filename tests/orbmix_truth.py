"""Dense truth of the orbital off-diagonal Green's function tests (test
infrastructure only).

Three hybrid / replica models small enough (<= 4,096 Fock states) for the
full-Fock Jordan-Wigner Hamiltonian of oracle.jw_dense: its blocks by
(popcount up, popcount down) give every sector's spectrum and eigenvectors by
dense eigh, the ground-state set {E : E - E0 < 1e-9} (or, for the thermal
test, {E : exp(-beta (E - E0)) > cutoff}), and G as the DIRECT Lehmann sum

  G_ab(z) = sum_n w_n [ <n|c_a (z - (H - E_n))^-1 c+_b|n>
                      + <n|c+_b (z + (H - E_n))^-1 c_a|n> ],

w_n = 1/N_gs or exp(-beta (E_n - E0))/zeta — not the four-seed recombination
of lanc_build_gf_normal_mix_c (ED_GF_NORMAL.f90:279-553) that the code under
test runs.  Everything is computed once per model and shared (never modified)
by the CPU and GPU tests.

  H2  cases.hybrid(): Norb=2, Nbath=4, Nspin=1, Ns=6; ground states: the twin
      pair in (2,3) and (3,2), both kept.
  H3  Norb=3, Nbath=2, Nspin=2 hybrid, Ns=5; one ground state, in (1,3); three
      orbital pairs per spin.
  RC  cases.replica_cplx(): Norb=2, Nbath=2 replica with a complex impHloc,
      Ns=6; one ground state, in (3,3).
"""
from functools import lru_cache

import numpy as np

BETA, CUTOFF = 8.0, 1e-4      # the thermal test (H2)
# Broadening of the real-axis checks, per model: the smallest of 0.1, 0.2, 0.3,
# 0.5 at which a 1e-15 relative perturbation of the seeds moves G(w) by less
# than 1e-9 of max|G| (measured with the oracle pipeline; the table is in
# test_orbmix_cpu's docstring)
EPS = {"H2": 0.2, "H3": 0.3, "RC": 0.2}


def config(name):
    import cases
    from edgpu.params import make_config

    if name == "H2":
        return cases.hybrid()
    if name == "RC":
        return cases.replica_cplx()
    assert name == "H3"
    cfg = make_config(Norb=3, Nbath=2, Nspin=2, bath_type="hybrid", Uloc=(2.0, 1.8, 1.6), Ust=1.0, Jh=0.2,
                      xmu=0.3, bath="random", seed=21)
    cfg.impHloc = cases._hloc(2, 3, 22)
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
        nup, ndw = pc(x & ((1 << Ns) - 1)), pc(x >> Ns)
        self.secs = setup_pointers(cfg)
        self.by_q = {(s.q1, s.q2): s.isector for s in self.secs}
        self.q_of = {s.isector: (s.q1, s.q2) for s in self.secs}
        self.maps, self.w, self.v = {}, {}, {}
        for s in self.secs:
            idx = x[(nup == s.q1) & (ndw == s.q2)]          # ascending: the sector's row order
            assert len(idx) == s.dim
            blk = H[idx][:, idx].toarray()
            assert np.max(np.abs(blk - blk.conj().T)) < 1e-14
            w, v = np.linalg.eigh(blk.real if np.max(np.abs(blk.imag)) == 0.0 else blk)
            self.maps[s.isector], self.w[s.isector], self.v[s.isector] = idx, w, v
        self.e0 = min(w[0] for w in self.w.values())

    def ground_states(self):
        """(energy, isector, index in the sector's spectrum) with E - E0 < 1e-9."""
        return sorted((float(e), i, k) for i, w in self.w.items() for k, e in enumerate(w) if e - self.e0 < 1e-9)

    def thermal_states(self, beta=BETA, cutoff=CUTOFF):
        return sorted((float(e), i, k) for i, w in self.w.items() for k, e in enumerate(w)
                      if np.exp(-beta * (e - self.e0)) > cutoff)

    def embed(self, isector, k):
        full = np.zeros(self.H.shape[0], dtype=np.complex128)
        full[self.maps[isector]] = self.v[isector][:, k]
        return full

    def gf(self, wm, wr, eps, beta=None, cutoff=CUTOFF):
        """(Gm, Gr), each (Nspin, Norb, Norb, L): every G_ab of every spin, by
        the direct Lehmann sum over the ground-state set (beta None) or the
        Boltzmann-weighted thermal set."""
        cfg = self.cfg
        Ns, No, Nsp = cfg.Ns, cfg.Norb, cfg.Nspin
        kept = self.ground_states() if beta is None else self.thermal_states(beta, cutoff)
        wts = np.ones(len(kept)) if beta is None else np.exp(-beta * (np.array([t[0] for t in kept]) - self.e0))
        wts = wts / wts.sum()
        zs = [1j * np.asarray(wm), np.asarray(wr) + 1j * eps]
        G = [np.zeros((Nsp, No, No, len(z)), dtype=np.complex128) for z in zs]
        for (e, isec, k), wt in zip(kept, wts):
            q = self.q_of[isec]
            psi = self.embed(isec, k)
            for s in range(Nsp):
                d = (1, 0) if s == 0 else (0, 1)
                for sign in (+1, -1):
                    tq = (q[0] + sign * d[0], q[1] + sign * d[1])
                    if tq not in self.by_q:
                        continue
                    j = self.by_q[tq]
                    # A[a][m] = <m| c+_a |n> (sign +1) or <m| c_a |n> (sign -1)
                    A = []
                    for a in range(No):
                        op = self.c[a + s * Ns]
                        op = op.getH() if sign > 0 else op
                        A.append(self.v[j].conj().T @ np.asarray(op @ psi).ravel()[self.maps[j]])
                    de = self.w[j] - e
                    for a in range(No):
                        for b in range(No):
                            # particle: <n|c_a|m><m|c+_b|n>; hole: <n|c+_b|m><m|c_a|n>
                            amp = np.conj(A[a]) * A[b] if sign > 0 else np.conj(A[b]) * A[a]
                            for g, z in zip(G, zs):
                                g[s, a, b] += wt * np.sum(amp[None, :] / (z[:, None] - sign * de[None, :]), axis=1)
        return G


@lru_cache(maxsize=None)
def truth(name) -> Truth:
    return Truth(name)
