"""Dense truth of the finite-temperature tests (test infrastructure only).

The Ns = 5 model make_config(Norb=1, Nbath=4, bath="random", seed=23) is small
enough (1,024 Fock states) for the full-Fock Jordan-Wigner Hamiltonian of
oracle.jw_dense: its blocks by (popcount up, popcount down) give every
sector's spectrum and eigenvectors, the thermal state set
{E : exp(-beta (E - E0)) > cutoff}, and the thermal Green's function and
observables as plain sums over those states.  Everything is computed once and
shared (never modified) by the CPU and GPU tests.
"""
from functools import lru_cache

import numpy as np

BETA, CUTOFF, NTOTAL = 8.0, 1e-4, 40


def config():
    from edgpu.params import make_config

    return make_config(Norb=1, Nbath=4, bath="random", seed=23)


class Truth:
    def __init__(self):
        from edgpu.sectors import setup_pointers
        from oracle.jw_dense import full_hamiltonian

        self.cfg = cfg = config()
        Ns = cfg.Ns
        self.H = H = full_hamiltonian(cfg).tocsr()
        x = np.arange(1 << (2 * Ns))
        pc = lambda v: np.array([bin(int(t)).count("1") for t in v])   # noqa: E731
        nup, ndw = pc(x & ((1 << Ns) - 1)), pc(x >> Ns)
        self.secs = setup_pointers(cfg)
        self.maps, self.w, self.v = {}, {}, {}
        for s in self.secs:
            idx = x[(nup == s.q1) & (ndw == s.q2)]          # ascending: the sector's row order
            assert len(idx) == s.dim
            blk = H[idx][:, idx].toarray()
            assert np.max(np.abs(blk.imag)) == 0.0
            w, v = np.linalg.eigh(blk.real)
            self.maps[s.isector], self.w[s.isector], self.v[s.isector] = idx, w, v
        self.e0 = min(w[0] for w in self.w.values())
        # the thermal set: (energy, isector, index in the sector's spectrum)
        self.kept = sorted((float(e), i, k) for i, w in self.w.items() for k, e in enumerate(w)
                           if np.exp(-BETA * (e - self.e0)) > CUTOFF)
        self.energies = np.array([t[0] for t in self.kept])
        self.boltz = np.exp(-BETA * (self.energies - self.e0))
        self.zeta = float(self.boltz.sum())

    def sector_results(self, nkeep=6, ed_twin=False, vectors=False):
        """SectorResults with the nkeep lowest dense eigenpairs of every
        sector ed_diag would visit."""
        from edgpu.diag import SectorResult
        from edgpu.sectors import diag_sectors

        out = []
        for s in diag_sectors(self.cfg, ed_twin):
            n = min(s.dim, nkeep)
            out.append(SectorResult(s.isector, (s.q1, s.q2), s.dim, self.w[s.isector][:n].copy(), n,
                                    self.v[s.isector][:, :n].copy() if vectors else None, "dense"))
        return out

    def embed(self, isector, k):
        full = np.zeros(self.H.shape[0])
        full[self.maps[isector]] = self.v[isector][:, k]
        return full

    def gf(self, wm, wr, eps):
        """Thermal G of the impurity orbital, spin up (= spin down, Nspin = 1):
        sum over the kept states n of exp(-beta dE_n)/zeta times
        <n|c (z - (H - E_n))^-1 c+|n> + <n|c+ (z + (H - E_n))^-1 c|n>, from the
        dense eigen-decompositions of the target sectors' blocks."""
        from oracle.jw_dense import _ops

        cfg = self.cfg
        c = _ops(2 * cfg.Ns)[0].tocsr()        # impurity level, spin up: bit 0
        by_q = {(s.q1, s.q2): s.isector for s in self.secs}
        zs = [1j * np.asarray(wm), np.asarray(wr) + 1j * eps]
        G = [np.zeros(len(z), dtype=np.complex128) for z in zs]
        for (e, isec, k), b in zip(self.kept, self.boltz):
            q = [(s.q1, s.q2) for s in self.secs if s.isector == isec][0]
            psi = self.embed(isec, k)
            for op, tq, sign in ((c.getH(), (q[0] + 1, q[1]), +1), (c, (q[0] - 1, q[1]), -1)):
                if tq not in by_q:
                    continue
                j = by_q[tq]
                seed = np.asarray(op @ psi).ravel()[self.maps[j]]
                amp2 = (self.v[j].T @ seed) ** 2            # |<m|op|n>|^2
                de = self.w[j] - e
                for g, z in zip(G, zs):
                    g += (b / self.zeta) * np.sum(amp2[None, :] / (z[:, None] - sign * de[None, :]), axis=1)
        return G

    def observables(self):
        """Thermal dens_up, dens_dw, docc of the impurity orbital."""
        Ns = self.cfg.Ns
        x = np.arange(self.H.shape[0])
        nu, nd = (x & 1).astype(float), ((x >> Ns) & 1).astype(float)
        out = np.zeros(3)
        for (e, isec, k), b in zip(self.kept, self.boltz):
            p = self.embed(isec, k) ** 2
            out += (b / self.zeta) * np.array([p @ nu, p @ nd, p @ (nu * nd)])
        return out


@lru_cache(maxsize=1)
def truth() -> Truth:
    return Truth()
