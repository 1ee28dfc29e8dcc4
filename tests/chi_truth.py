"""Dense truth of the susceptibility tests (test infrastructure only).

Models of <= 256 Fock states, small enough for the full-Fock Jordan-Wigner
Hamiltonian of oracle.jw_dense: its blocks by sector give every sector's
spectrum and eigenvectors by numpy.linalg.eigh; no Lanczos and no seeds.  For
state weights w_n, a diagonal operator O, D = E_m - E_n and m over the whole
spectrum of n's own block:

  tau_i : sum_n w_n sum_m |<m|O|n>|^2 [exp(-tau_i D) + exp(-(beta - tau_i) D)]
  iv_0  : sum_n w_n sum_m |<m|O|n>|^2 2 s(D),  s(D) = -expm1(-beta D) / D, s(0) = beta
  iv_i  : sum_n w_n sum_m |<m|O|n>|^2 (-expm1(-beta D)) [1/(i v_i + D) - 1/(i v_i - D)]
  w_i   : the same with i v_i -> wr_i + i eps

The orbital off-diagonal density is the cross term
sum_m Re(<n|n_a|m><m|n_b|n>) K(D) written out directly, not the
(chi[n_a+n_b] - chi[n_a] - chi[n_b]) / 2 recombination that the code under
test runs.

  C1  Norb=1, Nbath=2, normal, random bath, xmu=0.2: Ns=3, 64 Fock states.
  C2  Norb=2, Nbath=1, normal, unequal orbitals, Jx = Jp != 0 and an orbital
      off-diagonal impHloc (the interactions of cases.superc_2orb): Ns=4, 256.
  CN  nonSU2, Norb=1, Nbath=2, complex spin-flip impHloc: Ns=3, 64 Fock
      states, complex eigenvectors.
  thermal: C1 at beta = 8, cutoff 1e-4.

A T = 0 ground state can be degenerate, so `chi_of_list` takes the states and
weights (1/size) from the list under test; `chi_thermal` sums the dense thermal
set {exp(-beta (E - E0)) > cutoff} with w_n = exp(-beta (E_n - E0)) / zeta.
The T = 0 tests also run at beta = 8 (the reference uses beta for its grids at
T = 0 too).

A max-relative bar is only worth something if the static pole at D ~ 0 does
not swamp the arrays, so every truth asserts, for every component a test
compares, that the part of each array that comes from poles with |D| > 1e-6
is at least 1e-3 of that array's maximum (`Truth._sum`).

Everything is computed once per model and shared (never modified) by the CPU
and GPU tests.
"""
from functools import lru_cache

import numpy as np

BETA, CUTOFF, NTOTAL = 8.0, 1e-4, 40
LMATS, LTAU, LREAL = 32, 24, 32          # the grids of the build_chi tests
# Broadening of the real-axis checks, per model: the smallest of 0.01, 0.1,
# 0.2, 0.3, 0.5 at which the CPU replay holds 1e-5 (the table is in
# test_chi_cpu's docstring)
EPS = {"C1": 0.01, "C2": 0.01, "CN": 0.01}
DYNAMIC_D, DYNAMIC_SHARE = 1e-6, 1e-3


def config(name):
    import cases
    from edgpu.params import make_config

    if name == "C1":
        return make_config(Norb=1, Nbath=2, bath="random", xmu=0.2, seed=8)
    if name == "C2":
        # xmu = 0.8: at 0 .. 0.4 the static pole leaves the density cross term's dynamic share of iv
        # at 2e-4 .. 8e-4, under the 1e-3 this module asks for; here it is 2.3e-3
        cfg = make_config(Norb=2, Nbath=1, Nspin=1, Uloc=(2.0, 2.0, 0.0), Ust=1.0, Jh=0.3, Jx=0.3, Jp=0.3, xmu=0.8,
                          bath="random", seed=19)
        cfg.impHloc = cases._hloc(1, 2, 20)
        return cfg
    assert name == "CN"
    cfg = make_config(Norb=1, Nbath=2, Nspin=2, ed_mode="nonsu2", bath="random", xmu=0.15, seed=27)
    cfg.impHloc = cases._hloc(2, 1, 12, cplx=True, spinflip=True)
    return cfg


def options(name, **kw):
    from edgpu.chi import ChiOptions

    return ChiOptions(Lmats=LMATS, Ltau=LTAU, Lreal=LREAL, beta=BETA, eps=EPS[name], **kw)


class Truth:
    def __init__(self, name):
        from edgpu.sectors import setup_pointers
        from oracle.jw_dense import full_hamiltonian

        self.name = name
        self.cfg = cfg = config(name)
        Ns = cfg.Ns
        self.H = H = full_hamiltonian(cfg).tocsr()
        x = np.arange(1 << (2 * Ns))
        pc = lambda v: np.array([bin(int(t)).count("1") for t in v])   # noqa: E731
        nup, ndw = pc(x & ((1 << Ns) - 1)), pc(x >> Ns)
        self.secs = setup_pointers(cfg)
        self.maps, self.w, self.v = {}, {}, {}
        for s in self.secs:
            sel = (nup + ndw == s.q1) if cfg.ed_mode == "nonsu2" else (nup == s.q1) & (ndw == s.q2)
            idx = x[sel]                                     # ascending: the sector's row order
            assert len(idx) == s.dim
            blk = H[idx][:, idx].toarray()
            assert np.max(np.abs(blk - blk.conj().T)) < 1e-14
            w, v = np.linalg.eigh(blk.real if np.max(np.abs(blk.imag)) == 0.0 else blk)
            self.maps[s.isector], self.w[s.isector], self.v[s.isector] = idx, w, v
        self.e0 = min(w[0] for w in self.w.values())

    # -------------------------------------------------------- state sets
    def sector_results(self, nkeep=6, ed_twin=False):
        """SectorResults with the nkeep lowest dense eigenpairs of every
        sector ed_diag would visit."""
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

    # -------------------------------------------------------- the Lehmann sums
    def operators(self, isec):
        """Occupations of the impurity levels on the sector's rows: (nup[a], ndw[a]) as float arrays."""
        m, Ns = self.maps[isec], self.cfg.Ns
        return ([((m >> a) & 1).astype(float) for a in range(self.cfg.Norb)],
                [((m >> (a + Ns)) & 1).astype(float) for a in range(self.cfg.Norb)])

    def _sum(self, rows, copt):
        """rows: (weight, energy, isector, vector in the sector's row order).
        Returns {"spin": (iv, tau, w) with leading (Norb+1,), "dens": (Norb,
        Norb), "dens_tot": ()} on copt's grids."""
        from edgpu.chi import bosonic_matsubara, tau_grid
        from edgpu.gf import realaxis

        No, beta = self.cfg.Norb, copt.beta
        vm, tg = bosonic_matsubara(beta, copt.Lmats), tau_grid(beta, copt.ltau)
        zr = realaxis(copt.wini, copt.wfin, copt.Lreal) + 1j * copt.eps
        shapes = {"spin": (No + 1,), "dens": (No, No), "dens_tot": ()}
        mk = lambda: {k: [np.zeros(s + (len(vm),), complex), np.zeros(s + (len(tg),)), np.zeros(s + (len(zr),), complex)]   # noqa: E731
                      for k, s in shapes.items()}
        full, dyn = mk(), mk()

        def kernels(D):
            f = -np.expm1(-beta * D)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(D == 0.0, beta, f / np.where(D == 0.0, 1.0, D))
            iv = np.empty((len(vm), len(D)), complex)
            iv[0] = 2.0 * s
            iv[1:] = f[None] * (1.0 / (1j * vm[1:, None] + D[None]) - 1.0 / (1j * vm[1:, None] - D[None]))
            tau = np.exp(-tg[:, None] * D[None]) + np.exp(-(beta - tg[:, None]) * D[None])
            w = f[None] * (1.0 / (zr[:, None] + D[None]) - 1.0 / (zr[:, None] - D[None]))
            return iv, tau, w

        for wt, e, isec, vec in rows:
            nu, nd = self.operators(isec)
            V, D = self.v[isec], self.w[isec] - e
            K = kernels(D)
            far = np.abs(D) > DYNAMIC_D
            amp = lambda o: V.conj().T @ (o * vec)          # noqa: E731   <m|O|n>
            A = {"n": [amp(nu[a] + nd[a]) for a in range(No)], "s": [amp(0.5 * (nu[a] - nd[a])) for a in range(No)]}
            terms = [("spin", (a,), np.abs(A["s"][a]) ** 2) for a in range(No)]
            terms += [("dens", (a, b), np.real(np.conj(A["n"][a]) * A["n"][b])) for a in range(No) for b in range(No)]
            if No > 1:        # the totals are built for Norb > 1 only (zero otherwise, as the reference)
                terms.append(("spin", (No,), np.abs(sum(A["s"])) ** 2))
                terms.append(("dens_tot", (), np.abs(sum(A["n"])) ** 2))
            for key, at, a2 in terms:
                for g in range(3):
                    full[key][g][at] += wt * (K[g] @ a2)
                    dyn[key][g][at] += wt * (K[g][:, far] @ a2[far])
        # the static pole must not swamp any compared array
        self.shares = {}
        for key, shape in shapes.items():
            for at in np.ndindex(*shape):
                if No == 1 and (key == "dens_tot" or (key == "spin" and at == (No,))):
                    continue
                for g, grid in enumerate(("iv", "tau", "w")):
                    share = np.max(np.abs(dyn[key][g][at])) / np.max(np.abs(full[key][g][at]))
                    self.shares[(key, at, grid)] = share
                    assert share >= DYNAMIC_SHARE, (self.name, key, at, grid, share)
        return {k: tuple(v) for k, v in full.items()}

    def chi_of_list(self, states, copt, vector_of=None):
        """T = 0: the states of the list under test, w_n = 1/size.
        vector_of(k): host vector of entry k (default: the list's own)."""
        from edgpu.diag import to_host

        assert not states.finite_t
        get = vector_of or (lambda k: np.asarray(to_host(states.vectors[k])))
        rows = [(1.0 / states.size, states.energies[k], states.sectors[k], get(k)) for k in range(states.size)]
        return self._sum(rows, copt)

    def chi_thermal(self, copt, cutoff=CUTOFF):
        kept = self.thermal_states(copt.beta, cutoff)
        b = np.exp(-copt.beta * (np.array([t[0] for t in kept]) - self.e0))
        rows = [(bk / b.sum(), e, i, self.v[i][:, k]) for (e, i, k), bk in zip(kept, b)]
        return self._sum(rows, copt)


@lru_cache(maxsize=None)
def truth(name) -> Truth:
    return Truth(name)


def distances(T, got, norb):
    """(d_iv, d_tau, d_w): over every compared component, max |got - truth| over
    that array's own maximum.  got: a `Chi`; T: a dict of Truth._sum."""
    d = [0.0, 0.0, 0.0]
    pairs = [(T["spin"], (got.spin_iv, got.spin_tau, got.spin_w), [(a,) for a in range(norb + (norb > 1))]),
             (T["dens"], (got.dens_iv, got.dens_tau, got.dens_w), [(a, b) for a in range(norb) for b in range(norb)])]
    if norb > 1:
        pairs.append((T["dens_tot"], (got.dens_tot_iv, got.dens_tot_tau, got.dens_tot_w), [()]))
    for tr, arrs, comps in pairs:
        for g in range(3):
            if arrs[g] is None:
                continue
            for at in comps:
                d[g] = max(d[g], np.max(np.abs(arrs[g][at] - tr[g][at])) / np.max(np.abs(tr[g][at])))
    return tuple(d)
