"""build_gf_normal with the orbital off-diagonal components, from the oracle
pieces (test infrastructure): the reference's own algorithm, seed by seed —
lanc_build_gf_normal_c for G_aa, then for every pair a < b the four seeds of
lanc_build_gf_normal_mix_c (ED_GF_NORMAL.f90:279-553) with their weights
norm2, norm2, -xi*norm2, -xi*norm2, and the recombination and the G_ba copy of
build_gf_normal (ED_GF_NORMAL.f90:61-68).  Seeds by oracle_gf.seed_combo,
tridiagonalisation by the oracle's plain Lanczos, poles by LAPACK dstev.

`perturb` multiplies every element of every normalised seed by (1 + perturb *
N(0,1)) from `rng`: the round-off sensitivity measurement quoted in
test_orbmix_cpu's docstring.
"""
import numpy as np

from edgpu.diag import to_host
from edgpu.gf import matsubara, realaxis
from edgpu.sectors import c_sector, cdg_sector, setup_pointers
from oracle.oracle import Oracle, lanc_tridiag
from oracle_gf import seed_combo, tridiag_poles


def pairs(cfg):
    """ED_GF_NORMAL.f90:35-42: hybrid all a < b; replica where impHloc(s,s,a,b) is set."""
    if cfg.bath_type == "normal":
        return []
    return [(s, a, b) for s in range(cfg.Nspin) for a in range(cfg.Norb) for b in range(a + 1, cfg.Norb)
            if cfg.bath_type != "replica" or abs(cfg.impHloc[s, s, a, b].real) > 1e-6
            or abs(cfg.impHloc[s, s, a, b].imag) > 1e-6]


def build_gf_orbmix_oracle(cfg, states, gopt, perturb=0.0, rng=None):
    orc = Oracle(cfg)
    Ns, No, Nsp = cfg.Ns, cfg.Norb, cfg.Nspin
    wm = matsubara(gopt.beta, gopt.Lmats)
    wr = realaxis(gopt.wini, gopt.wfin, gopt.Lreal)
    Gm = np.zeros((Nsp, Nsp, No, No, gopt.Lmats), dtype=np.complex128)
    Gr = np.zeros((Nsp, Nsp, No, No, gopt.Lreal), dtype=np.complex128)
    secs = setup_pointers(cfg)
    zeta = float(len(states.energies))
    vecs = [np.asarray(to_host(v)).astype(np.complex128) for v in states.vectors]

    def channel(idx, ispin, specs):
        for e_i, isec, vec in zip(states.energies, states.sectors, vecs):
            sec = secs[isec - 1]
            hmap_i = orc.build_sector(sec.q1, sec.q2)
            for op, isign, terms, weight in specs:
                jsec = cdg_sector(cfg, sec, ispin) if op == 1 else c_sector(cfg, sec, ispin)
                if jsec is None:
                    continue
                hmap_j, v = seed_combo(orc, hmap_i, jsec, op, terms, vec)
                norm2 = float(np.vdot(v, v).real)
                if norm2 == 0.0:
                    continue
                v = v / np.sqrt(norm2)
                if perturb:
                    v = v * (1.0 + perturb * rng.normal(size=len(v)))
                nlanc = min(len(hmap_j), gopt.lanc_nGFiter)
                a, b, n = lanc_tridiag(orc.build_csr(hmap_j), v, nlanc, gopt.threshold)
                E, z2 = tridiag_poles(a, b, nlanc)
                de = E - e_i
                peso = weight * norm2 / zeta * z2
                Gm[idx] += (peso[None] / ((1j * wm)[:, None] - isign * de[None])).sum(1)
                Gr[idx] += (peso[None] / ((wr + 1j * gopt.eps)[:, None] - isign * de[None])).sum(1)

    site = lambda o, s: o + s * Ns      # noqa: E731
    for s in range(Nsp):
        for a in range(No):
            i = site(a, s)
            channel((s, s, a, a), s, [(1, 1, [(i, 1)], 1.0), (0, -1, [(i, 1)], 1.0)])
    P = pairs(cfg)
    for s, a, b in P:
        i, j = site(a, s), site(b, s)
        channel((s, s, a, b), s, [(1, 1, [(i, 1), (j, 1)], 1.0), (0, -1, [(i, 1), (j, 1)], 1.0),
                                  (1, 1, [(i, 1), (j, 1j)], -1j), (0, -1, [(i, 1), (j, -1j)], -1j)])
    for s, a, b in P:
        for G in (Gm, Gr):
            G[s, s, a, b] = 0.5 * (G[s, s, a, b] - (1 - 1j) * G[s, s, a, a] - (1 - 1j) * G[s, s, b, b])
            G[s, s, b, a] = G[s, s, a, b]
    return Gm, Gr
